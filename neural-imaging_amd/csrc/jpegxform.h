// The sequential core of the lossless transforms: jpegtran's flips, transposition, rotations and aligned crop on
// the quantised coefficients of a file - which output block comes from which source block, where each of its 64 coefficients comes
// from and which of them change sign, and the geometry of the file that results (what jtransform.c derives, restated on the source).
// jpegx.hip runs it eight lanes per block; everything here is `__host__ __device__` under hipcc and plain C++ otherwise, so that a host
// compiler can build it into a stand-alone program (tests/jpegxform_host.cpp) and hold it to sanitizers.
//
// A block is C[v][u] in natural order, v vertical.  Mirroring the samples of a block left to right negates the coefficients of odd u,
// top to bottom those of odd v; transposing them transposes the coefficients (and every quantisation table, on the host).  With the
// blocks of every component reordered the same way that is the whole transform: a permutation with sign changes.  Every operation is
//     transpose first (T), then mirror left to right (FH), then top to bottom (FV)
// with the flags jpegxform_flags names, and is carried out as ONE gather: output block (r, c) of a component names its source block, and
// output coefficient k its source coefficient.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "jpeg_geo.h"

// jpegtran's names, in the order of the C ABI (include/nimg.h nimg_jpeg_lossless) and of ops.JPEG_LOSSLESS_OPS
enum { JPEGXFORM_NONE = 0, JPEGXFORM_HFLIP = 1, JPEGXFORM_VFLIP = 2, JPEGXFORM_TRANSPOSE = 3, JPEGXFORM_TRANSVERSE = 4,
       JPEGXFORM_ROT90 = 5, JPEGXFORM_ROT180 = 6, JPEGXFORM_ROT270 = 7, JPEGXFORM_OPS = 8 };
enum { JPEGXFORM_T = 1, JPEGXFORM_FH = 2, JPEGXFORM_FV = 4 };

// rot90 (clockwise) = transpose then hflip, rot270 = transpose then vflip, rot180 = hflip then vflip, transverse = transpose then rot180
JPEG_GEO_HD constexpr int jpegxform_flags(int op) {
    return op == JPEGXFORM_HFLIP        ? JPEGXFORM_FH
           : op == JPEGXFORM_VFLIP      ? JPEGXFORM_FV
           : op == JPEGXFORM_TRANSPOSE  ? JPEGXFORM_T
           : op == JPEGXFORM_TRANSVERSE ? JPEGXFORM_T | JPEGXFORM_FH | JPEGXFORM_FV
           : op == JPEGXFORM_ROT90      ? JPEGXFORM_T | JPEGXFORM_FH
           : op == JPEGXFORM_ROT180     ? JPEGXFORM_FH | JPEGXFORM_FV
           : op == JPEGXFORM_ROT270     ? JPEGXFORM_T | JPEGXFORM_FV
                                        : 0;
}

// ---- inside a block: zig-zag positions ---------------------------------------------------------------------------------------------------
// the natural index 8 v + u of zig-zag position k: the scan walks the anti-diagonals d = v + u, odd ones with v ascending
JPEG_GEO_HD constexpr int jpegxform_natural(int k) {
    int at = 0;
    for (int d = 0; d < 15; ++d) {
        const int lo = d < 8 ? 0 : d - 7, hi = d < 8 ? d : 7;          // the range of v on this diagonal
        const int len = hi - lo + 1;
        if (k < at + len) {
            const int j = k - at;
            const int v = (d & 1) ? lo + j : hi - j;
            return 8 * v + (d - v);
        }
        at += len;
    }
    return 63;
}

// the zig-zag position of the transposed coefficient: C[v][u] -> C[u][v] reverses every anti-diagonal
JPEG_GEO_HD constexpr int jpegxform_transposed(int k) {
    int at = 0;
    for (int d = 0; d < 15; ++d) {
        const int len = (d < 8 ? d : 14 - d) + 1;
        if (k < at + len) return at + (len - 1) - (k - at);
        at += len;
    }
    return 63;
}

// bit k set: the coefficient at zig-zag position k has an odd u (odd_v: an odd v).  The DC, position 0, is in neither.
JPEG_GEO_HD constexpr uint64_t jpegxform_odd_mask(bool odd_v) {
    uint64_t m = 0;
    for (int k = 0; k < 64; ++k) {
        const int nat = jpegxform_natural(k);
        if ((odd_v ? nat >> 3 : nat) & 1) m |= (uint64_t)1 << k;
    }
    return m;
}

// the positions of the OUTPUT block whose coefficients are negated: mirrored both ways, a coefficient of odd u and odd v keeps its sign
JPEG_GEO_HD constexpr uint64_t jpegxform_negated(int flags) {
    return ((flags & JPEGXFORM_FH) ? jpegxform_odd_mask(false) : 0) ^ ((flags & JPEGXFORM_FV) ? jpegxform_odd_mask(true) : 0);
}

// the eight source positions of output positions 8 j .. 8 j + 7 of a transposed block, one byte each, the first in the low byte
JPEG_GEO_HD constexpr uint64_t jpegxform_transposed_octet(int j) {
    uint64_t m = 0;
    for (int i = 0; i < 8; ++i) m |= (uint64_t)jpegxform_transposed(8 * j + i) << (8 * i);
    return m;
}

// two's complement on 16 bits, as jtransform.c's plain -x on a JCOEF: -(-32768) stays -32768
JPEG_GEO_HD inline int16_t jpegxform_negate(int16_t x) { return (int16_t)(uint16_t)(0u - (uint16_t)x); }

// ---- between blocks: the geometry ---------------------------------------------------------------------------------------------------------
// why a transform is refused (jpegxform_make); the Python layer words them
enum { JPEGXFORM_OK = 0, JPEGXFORM_E_OP = 1, JPEGXFORM_E_GEOMETRY = 2, JPEGXFORM_E_CROP_ALIGN = 3, JPEGXFORM_E_CROP_OUTSIDE = 4,
       JPEGXFORM_E_PARTIAL_WIDTH = 5, JPEGXFORM_E_PARTIAL_HEIGHT = 6, JPEGXFORM_E_EMPTY = 7 };

struct JpegXform {
    int op, flags, nc;
    int h, w, hs, vs;                      // the file that results; (hs, vs) = (1, 1) with nc = 1
    int rows[2], cols[2];                  // its real blocks, [0] luma and [1] one chroma component
    int nbY, nbC, NB;                      // and their counts per image
    int srows[2], scols[2];                // the source's real blocks
    int snbY, snbC, sNB;
    int oy[2], ox[2];                      // the block of the source that the region begins at, per component kind
};

// The file an operation makes of a source h x w with luma factors (hs, vs) - nc = 1: a grey-scale file, whose iMCU is 8 x 8 whatever it
// declares, given as hs = vs = 1 - after the region (crop_x, crop_y, crop_w, crop_h) is cut from it; crop_w == 0: no crop.  A transform
// moves whole iMCUs, so an operation that mirrors the source's width (FH without T, FV with T) needs it to be a multiple of 8 hs, one
// that mirrors its height a multiple of 8 vs - jtransform.c's trim_right_edge / trim_bottom_edge on the output, restated on the source.
// trim: cut the dimension down to that multiple (jpegtran -trim) instead of refusing (-perfect).  The crop origin must be a multiple of
// the iMCU.  Returns JPEGXFORM_OK or the reason.
inline int jpegxform_make(JpegXform* x, int h, int w, int hs, int vs, int nc, int op, int crop_x, int crop_y, int crop_w, int crop_h,
                          int trim, int factors = JPEG_FACTORS_WIDE) {
    if (op < 0 || op >= JPEGXFORM_OPS) return JPEGXFORM_E_OP;
    JpegGeo s;
    if (!make_geo(&s, 1, h, w, hs, vs, nc, factors)) return JPEGXFORM_E_GEOMETRY;
    const int flags = jpegxform_flags(op), T = flags & JPEGXFORM_T;
    int rh = h, rw = w, x0 = 0, y0 = 0;
    if (crop_w != 0 || crop_h != 0 || crop_x != 0 || crop_y != 0) {
        if (crop_w < 1 || crop_h < 1 || crop_x < 0 || crop_y < 0 || crop_x > w - crop_w || crop_y > h - crop_h) return JPEGXFORM_E_CROP_OUTSIDE;
        if (crop_x % (8 * hs) || crop_y % (8 * vs)) return JPEGXFORM_E_CROP_ALIGN;
        rh = crop_h; rw = crop_w; x0 = crop_x; y0 = crop_y;
    }
    const bool mirror_w = T ? (flags & JPEGXFORM_FV) != 0 : (flags & JPEGXFORM_FH) != 0;
    const bool mirror_h = T ? (flags & JPEGXFORM_FH) != 0 : (flags & JPEGXFORM_FV) != 0;
    if (mirror_w && rw % (8 * hs)) {
        if (!trim) return JPEGXFORM_E_PARTIAL_WIDTH;
        rw -= rw % (8 * hs);
    }
    if (mirror_h && rh % (8 * vs)) {
        if (!trim) return JPEGXFORM_E_PARTIAL_HEIGHT;
        rh -= rh % (8 * vs);
    }
    if (rw < 1 || rh < 1) return JPEGXFORM_E_EMPTY;
    JpegGeo o;
    if (!make_geo(&o, 1, T ? rw : rh, T ? rh : rw, T ? vs : hs, T ? hs : vs, nc, factors)) return JPEGXFORM_E_GEOMETRY;
    x->op = op; x->flags = flags; x->nc = nc;
    x->h = o.h; x->w = o.w; x->hs = o.hs; x->vs = o.vs;
    x->rows[0] = o.bhY; x->cols[0] = o.bwY; x->rows[1] = o.bhC; x->cols[1] = o.bwC;
    x->nbY = o.nbY; x->nbC = o.nbC; x->NB = o.NB;
    x->srows[0] = s.bhY; x->scols[0] = s.bwY; x->srows[1] = s.bhC; x->scols[1] = s.bwC;
    x->snbY = s.nbY; x->snbC = s.nbC; x->sNB = s.NB;
    x->oy[0] = y0 / 8; x->ox[0] = x0 / 8;                              // the chroma origin is (x / hs, y / vs) samples
    x->oy[1] = y0 / (8 * vs); x->ox[1] = x0 / (8 * hs);
    // every output block has its source inside the source's real blocks (the region lies inside the image): checked, not assumed
    for (int k = 0; k < (nc == 1 ? 1 : 2); ++k) {
        const int need_r = T ? x->cols[k] : x->rows[k], need_c = T ? x->rows[k] : x->cols[k];
        if (x->oy[k] + need_r > x->srows[k] || x->ox[k] + need_c > x->scols[k]) return JPEGXFORM_E_GEOMETRY;
    }
    return JPEGXFORM_OK;
}

// block b of one output image, 0 <= b < x.NB -> its component and its place in it
JPEG_GEO_HD inline void jpegxform_locate(const JpegXform& x, int b, int& comp, int& r, int& c) {
    comp = b < x.nbY ? 0 : 1 + (b - x.nbY) / x.nbC;
    const int kind = comp ? 1 : 0, within = comp ? (b - x.nbY) - (comp - 1) * x.nbC : b;
    r = within / x.cols[kind];
    c = within - r * x.cols[kind];
}

// the block of one source image, 0 <= result < x.sNB, that output block (comp, r, c) is made of: undo FV and FH, then T, then the crop
JPEG_GEO_HD inline int jpegxform_source_block(const JpegXform& x, int comp, int r, int c) {
    const int kind = comp ? 1 : 0;
    const int ri = (x.flags & JPEGXFORM_FV) ? x.rows[kind] - 1 - r : r;
    const int ci = (x.flags & JPEGXFORM_FH) ? x.cols[kind] - 1 - c : c;
    const int sr = ((x.flags & JPEGXFORM_T) ? ci : ri) + x.oy[kind], sc = ((x.flags & JPEGXFORM_T) ? ri : ci) + x.ox[kind];
    return (comp ? x.snbY + (comp - 1) * x.snbC : 0) + sr * x.scols[kind] + sc;
}

// one block, sequentially: out[k] = +- in[k or its transposed position]
JPEG_GEO_HD inline void jpegxform_block(int flags, const int16_t* in, int16_t* out) {
    const uint64_t neg = jpegxform_negated(flags);
    for (int k = 0; k < 64; ++k) {
        const int16_t v = in[(flags & JPEGXFORM_T) ? jpegxform_transposed(k) : k];
        out[k] = (neg >> k & 1) ? jpegxform_negate(v) : v;
    }
}

// n images, sequentially: coef (n, x.sNB, 64) -> out (n, x.NB, 64).  The form the host program runs and the kernel is held to.
inline void jpegxform_run(const JpegXform& x, const int16_t* coef, int n, int16_t* out) {
    for (int i = 0; i < n; ++i)
        for (int b = 0; b < x.NB; ++b) {
            int comp, r, c;
            jpegxform_locate(x, b, comp, r, c);
            jpegxform_block(x.flags, coef + ((size_t)i * x.sNB + jpegxform_source_block(x, comp, r, c)) * 64, out + ((size_t)i * x.NB + b) * 64);
        }
}
