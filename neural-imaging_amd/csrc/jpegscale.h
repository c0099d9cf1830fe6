// The sequential core of scaled decoding: libjpeg's scale_num / scale_denom = 1 / s for s = 2, 4, 8 - the
// block size every component's inverse DCT writes (jdmaster.c), the geometry of the scaled sample planes, where a chroma sample of an
// output pixel comes from (jdsample.c) and the reduced inverse DCTs (jidctred.c).  jpegd_scaled.hip runs it one thread per block and
// per pixel; everything here is `__host__ __device__` under hipcc and plain C++ otherwise, so that a host compiler can build it into a
// stand-alone program (tests/jpegscale_host.cpp) and hold it to sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "jpeg_geo.h"

#if defined(__HIPCC__)
#define JPEGSCALE_UNROLL _Pragma("unroll")        // the device keeps a block in registers: every index must be a constant
#else
#define JPEGSCALE_UNROLL
#endif

enum { JPEGSCALE_UP_NONE = 0, JPEGSCALE_UP_REPLICATE = 1, JPEGSCALE_UP_FANCY = 2 };
// the up-sampler of any sampling: none, the h2v1 or the h1v2 triangle filter, replication by (rx, ry)
enum { JPEGSCALE_MODE_NONE = 0, JPEGSCALE_MODE_REPLICATE = 1, JPEGSCALE_MODE_H2V1 = 2, JPEGSCALE_MODE_H1V2 = 3 };

// The planes of one image lie [Y | Cb | Cr], every plane over the component's real blocks at its own block size (rows of
// stride = block columns * N samples), and every plane begins at a multiple of 16 bytes.
struct JpegScaleGeo {
    int s, m;                          // the denominator, and 8 / s: the scaled block size of the frame
    int oh, ow;                        // the output image: ceil(h / s), ceil(w / s)
    int nY, nC;                        // the side of a luma and of a chroma block: m, and m doubled while jpegscale_block lets it (up to 8)
    int ehY, ewY, ehC, ewC;            // a component's scaled extent in samples: ceil(h vc N / (8 vmax)), ceil(w hc N / (8 hmax))
    int strideY, strideC;              // samples from one plane row to the next
    int up;                            // JPEGSCALE_UP_*: how a chroma row becomes an output row (2 : 1 horizontally, 4:2:2 only) - the
                                       // form of section 4q, which says "as wide or half as wide": it holds for 1x1, 2x1 and 2x2 alone
    int rx, ry, mode;                  // any sampling (section 4r): output samples per chroma sample along a row and down a column,
                                       // hmax m / nC and vmax m / nC, and the JPEGSCALE_MODE_* that brings the chroma up by them
    size_t planeY, planeC, per;        // bytes of the luma plane, of one chroma plane, of an image's planes
};

JPEG_GEO_HD inline bool jpegscale_ok(int scale) { return scale == 1 || scale == 2 || scale == 4 || scale == 8; }

// jdmaster.c: a component's block is doubled while that still divides what the largest factors make of the frame's block
JPEG_GEO_HD inline int jpegscale_block(int m, int hc, int vc, int hmax, int vmax) {
    int N = m;
    while (N < 8 && (hmax * m) % (hc * N * 2) == 0 && (vmax * m) % (vc * N * 2) == 0) N *= 2;
    return N;
}

JPEG_GEO_HD inline int jpegscale_ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// false: not a reduced scale (scale 1 is the full-size reconstruction, whose chroma may be up-sampled both ways)
JPEG_GEO_HD inline bool make_scale_geo(JpegScaleGeo* sg, const JpegGeo& g, int scale) {
    if (!jpegscale_ok(scale) || scale == 1) return false;
    const int m = 8 / scale;
    const int hmax = g.nc == 1 ? 1 : g.hs, vmax = g.nc == 1 ? 1 : g.vs;        // a one-component file: N = m whatever it declares
    sg->s = scale; sg->m = m;
    sg->oh = jpegscale_ceil_div(g.h, scale); sg->ow = jpegscale_ceil_div(g.w, scale);
    sg->nY = jpegscale_block(m, hmax, vmax, hmax, vmax);
    sg->nC = g.nc == 1 ? 0 : jpegscale_block(m, 1, 1, hmax, vmax);
    sg->ehY = jpegscale_ceil_div((long)g.h * sg->nY, 8); sg->ewY = jpegscale_ceil_div((long)g.w * sg->nY, 8);
    sg->ehC = g.nc == 1 ? 0 : jpegscale_ceil_div((long)g.h * sg->nC, 8L * vmax);
    sg->ewC = g.nc == 1 ? 0 : jpegscale_ceil_div((long)g.w * sg->nC, 8L * hmax);
    sg->strideY = g.bwY * sg->nY; sg->strideC = g.bwC * sg->nC;
    // jdsample.c: the chroma is as wide as the output (nothing to do) or half as wide; then the triangle filter, unless the frame's
    // block is one sample (do_fancy needs min_DCT_scaled_size > 1) or the row has at most two samples
    sg->up = (g.nc == 1 || sg->ewC == sg->ow) ? JPEGSCALE_UP_NONE : (scale < 8 && sg->ewC > 2) ? JPEGSCALE_UP_FANCY : JPEGSCALE_UP_REPLICATE;
    // jdsample.c's choice by the ratios, in its order: none; h2v1, h1v2 and h2v2 with the triangle filter where do_fancy holds (and, for
    // the two that widen, the row has more than two samples), else replication.  (2, 2) cannot arise over 1x1 chroma: the block of such a
    // component would have been doubled once more - it is refused, not guessed at.
    sg->rx = g.nc == 1 ? 1 : hmax * m / sg->nC; sg->ry = g.nc == 1 ? 1 : vmax * m / sg->nC;
    if (sg->rx == 2 && sg->ry == 2) return false;
    sg->mode = (sg->rx == 1 && sg->ry == 1) ? JPEGSCALE_MODE_NONE
               : (sg->rx == 2 && sg->ry == 1 && m > 1 && sg->ewC > 2) ? JPEGSCALE_MODE_H2V1
               : (sg->rx == 1 && sg->ry == 2 && m > 1) ? JPEGSCALE_MODE_H1V2 : JPEGSCALE_MODE_REPLICATE;
    sg->planeY = ((size_t)g.nbY * sg->nY * sg->nY + 15) & ~(size_t)15;
    sg->planeC = ((size_t)g.nbC * sg->nC * sg->nC + 15) & ~(size_t)15;
    sg->per = sg->planeY + (size_t)(g.nc - 1) * sg->planeC;
    return true;
}

JPEG_GEO_HD inline size_t jpegscale_plane_offset(const JpegScaleGeo& sg, int img, int comp) {
    return (size_t)img * sg.per + (comp ? sg.planeY + (size_t)(comp - 1) * sg.planeC : 0);
}

// Output column x of a chroma row that is half as wide: the sample under the pixel, and the neighbour on the pixel's side that the
// triangle filter weighs in (the edge sample is its own neighbour, which is libjpeg's special case of the first and last column).
JPEG_GEO_HD inline void jpegscale_chroma_columns(const JpegScaleGeo& sg, int x, int& near, int& nb) {
    near = x >> 1;
    nb = (x & 1) ? (near + 1 < sg.ewC ? near + 1 : sg.ewC - 1) : (near > 0 ? near - 1 : 0);
}

// The chroma sample under output pixel (y, x) for any sampling: p = the component's scaled plane.  The arithmetic of the two triangle
// filters is jpegc.h's (fancy_h2v1, chroma_h1v2_at); a neighbour beyond the component's extent is the edge sample itself.
JPEG_GEO_HD inline int jpegscale_chroma_at(const uint8_t* p, const JpegScaleGeo& sg, int y, int x) {
    if (sg.mode == JPEGSCALE_MODE_NONE) return p[(size_t)y * sg.strideC + x];
    if (sg.mode == JPEGSCALE_MODE_H2V1) {
        int near, nb;
        jpegscale_chroma_columns(sg, x, near, nb);
        const uint8_t* row = p + (size_t)y * sg.strideC;
        return (3 * row[near] + row[nb] + 1 + (x & 1)) >> 2;
    }
    if (sg.mode == JPEGSCALE_MODE_H1V2) {
        const int j = y >> 1, nb = (y & 1) ? (j + 1 < sg.ehC ? j + 1 : sg.ehC - 1) : (j > 0 ? j - 1 : 0);
        return (3 * p[(size_t)j * sg.strideC + x] + p[(size_t)nb * sg.strideC + x] + 1 + (y & 1)) >> 2;
    }
    return p[(size_t)(y / sg.ry) * sg.strideC + x / sg.rx];
}

// ---- the reduced inverse DCTs -------------------------------------------------------------------------------------------------
// scan position of natural index 8 * row + col
JPEG_GEO_HD constexpr int jpegscale_zz_of_nat(int nat) {
    constexpr int zz[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                            10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    return zz[nat];
}

JPEG_GEO_HD inline int jpegscale_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
JPEG_GEO_HD inline int jpegscale_limit(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// one pass of jpeg_idct_4x4 over the inputs i[0..7] (i[4] is not read): four outputs, descaled by n
JPEG_GEO_HD inline void jpegscale_pass4(const int* i, int n, int* o) {
    const int t0 = i[0] * 16384;
    const int t2 = 15137 * i[2] - 6270 * i[6];
    const int a0 = -1730 * i[7] + 11893 * i[5] - 17799 * i[3] + 8697 * i[1];
    const int a2 = -4176 * i[7] - 4926 * i[5] + 7373 * i[3] + 20995 * i[1];
    o[0] = jpegscale_descale(t0 + t2 + a2, n); o[1] = jpegscale_descale(t0 - t2 + a0, n);
    o[2] = jpegscale_descale(t0 - t2 - a0, n); o[3] = jpegscale_descale(t0 + t2 - a2, n);
}

// one pass of jpeg_idct_2x2 over the inputs i[0], i[1], i[3], i[5], i[7]: two outputs, descaled by n
JPEG_GEO_HD inline void jpegscale_pass2(const int* i, int n, int* o) {
    const int t10 = i[0] * 32768;
    const int t0 = -5906 * i[7] + 6967 * i[5] - 10426 * i[3] + 29692 * i[1];
    o[0] = jpegscale_descale(t10 + t0, n); o[1] = jpegscale_descale(t10 - t0, n);
}

// A block's N x N samples (0..255, row-major in out) from its quantised coefficients: coef(k) is the coefficient at scan position k,
// q the table in natural order.  Only the coefficients the transform uses are asked for: all but row and column 4 for N = 4, rows and
// columns 0, 1, 3, 5, 7 for N = 2, the DC for N = 1.  Columns first, then rows, as libjpeg orders them; products and sums are `int`,
// as in jpegc.h's idct8.
template <int N, class Coef>
JPEG_GEO_HD inline void jpegscale_idct(const Coef& coef, const uint16_t* q, int* out) {
    static_assert(N == 1 || N == 2 || N == 4, "the reduced transforms; N = 8 is jpegc.h's idct8");
    if constexpr (N == 1) {
        out[0] = jpegscale_limit(jpegscale_descale(coef(0) * (int)q[0], 3) + 128);
    } else {
        int ws[N * 8] = {};
        JPEGSCALE_UNROLL
        for (int c = 0; c < 8; ++c) {
            if (N == 4 ? c == 4 : (c != 0 && !(c & 1))) continue;
            int i[8] = {}, o[N];
            JPEGSCALE_UNROLL
            for (int r = 0; r < 8; ++r) {
                if (N == 4 ? r == 4 : (r != 0 && !(r & 1))) continue;
                i[r] = coef(jpegscale_zz_of_nat(8 * r + c)) * (int)q[8 * r + c];
            }
            if constexpr (N == 4) jpegscale_pass4(i, 12, o);
            else jpegscale_pass2(i, 13, o);
            JPEGSCALE_UNROLL
            for (int r = 0; r < N; ++r) ws[8 * r + c] = o[r];
        }
        JPEGSCALE_UNROLL
        for (int r = 0; r < N; ++r) {
            int o[N];
            if constexpr (N == 4) jpegscale_pass4(ws + 8 * r, 19, o);
            else jpegscale_pass2(ws + 8 * r, 20, o);
            JPEGSCALE_UNROLL
            for (int c = 0; c < N; ++c) out[N * r + c] = jpegscale_limit(o[c] + 128);
        }
    }
}
