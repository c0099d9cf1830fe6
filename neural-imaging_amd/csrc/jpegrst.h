// The sequential core of writing restart intervals: the bit-offset functions the coder's offset scan composes,
// and where the markers stand in the un-stuffed stream.  jpegc.h scans the functions over a workgroup and jpegc.hip's scatter pass
// writes the markers; everything here is `__host__ __device__` under hipcc and plain C++ otherwise, so that a host compiler can
// build it into a stand-alone program (tests/jpegrst_host.cpp) and hold it to sanitizers.
#pragma once
#include <stdint.h>

#include "jpeg_geo.h"

// BitFn is x -> round ? roundup8(x + a) + b : x + a.  A block of a bits is (a, 0, 0); a block that ends a restart interval a marker
// follows is (a, 16, 1): its byte is filled up, then 16 bits are left free for the marker.  a + b = "a, then b" has the same form,
// so the offsets of an image with markers are still one exclusive scan.
struct BitFn {
    uint32_t a, b, round;
    JPEG_GEO_HD uint32_t at(uint32_t x) const { return round ? ((x + a + 7u) & ~7u) + b : x + a; }
};
JPEG_GEO_HD inline BitFn operator+(const BitFn& f, const BitFn& g) {
    if (!f.round) return BitFn{f.a + g.a, g.b, g.round};
    return BitFn{f.a, g.at(f.b), 1u};                  // roundup8(x + f.a) is a multiple of 8: what follows adds to f.b alone
}
JPEG_GEO_HD inline BitFn jpegrst_block_fn(uint32_t len, const JpegGeo& g, int s) {
    return jpeg_marker_follows(g, s) ? BitFn{len, 16u, 1u} : BitFn{len, 0u, 0u};
}

// the 1-bits behind scan block s, whose bits end at bit `end`: the last block of the image, and of a restart interval a marker
// follows, fills its byte up
JPEG_GEO_HD inline int jpegrst_pad_bits(const JpegGeo& g, int s, uint32_t end) {
    return (s == g.SB - 1 || jpeg_marker_follows(g, s)) ? (int)((0u - end) & 7u) : 0;
}

// Marker k (0 ..) of an image stands in the 16 free bits in front of interval k + 1, whose first block is (k + 1) * g.ri * g.per:
// the bytes off[that block] / 8 - 2 and - 1 of the un-stuffed stream (off: the image's bit offsets).
// the first marker that ends behind byte `pos`
JPEG_GEO_HD inline int jpegrst_first_marker(const uint32_t* off, const JpegGeo& g, unsigned pos) {
    const int stride = g.ri * g.per;
    int lo = 0, hi = jpeg_markers(g);
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((off[(long)(mid + 1) * stride] >> 3) > pos) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// what byte `pos` is: 0 = data, 0xff = a marker's first byte, 0xd0 .. 0xd7 = its second.  k0 = jpegrst_first_marker of a position
// at most 3 bytes before `pos`: a word of 4 bytes meets two markers, three where an interval is empty.
JPEG_GEO_HD inline uint32_t jpegrst_marker_byte(const uint32_t* off, const JpegGeo& g, int k0, unsigned pos) {
    const int stride = g.ri * g.per, markers = jpeg_markers(g);
    for (int k = k0; k < markers && k < k0 + 3; ++k) {
        const unsigned end = off[(long)(k + 1) * stride] >> 3;
        if (pos + 2u == end) return 0xffu;
        if (pos + 1u == end) return 0xd0u | (unsigned)(k & 7);
    }
    return 0u;
}
