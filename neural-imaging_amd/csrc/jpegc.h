// What the units of the JPEG family share (jpegc.hip: one quality per batch and the entropy coder; jpegc_items.hip: one quality per
// image; jpegc_tables.hip: the caller's quantisation tables per item; jpegd.hip: the tables of each file; jpegc_opt.hip: the coder with
// the caller's Huffman tables): the workspace layout, the
// quantisation tables, the bit sink of the two coders, and the forward-transform and inverse-DCT kernels as templates over where their
// quantisation table comes from - a unit instantiates them with its own table source, so each instantiation knows the address space it
// reads.  Everything here has internal linkage - each unit compiles its own copy.
#pragma once
#include "common.h"
#include "jpeg_geo.h"
#include "jpegrst.h"

namespace {

constexpr int SCAN_THREADS = 1024;

using nimg::align256;

// ---- geometry and workspace ---------------------------------------------------------------------------------------------
// The longest block with the Annex K tables: DC 9 + 11, 63 x (AC 16 + 10).  JPEGOPT_BLOCK_BITS_MAX, the bound with a caller's tables, is
// 7 bits larger because a DC code may then have 16 bits where Annex K's longest has 9; an AC code has up to 16 bits in both.
constexpr int BLOCK_BITS_MAX = 1658;

struct Workspace {
    uint32_t* flag;                    // transform: non-zero = some float sample exceeds 1
    uint32_t* codes;                   // coder with the caller's tables: [n][code_words] symbol -> code << 5 | length
    uint32_t* off;                     // [n][SB] bit lengths, then (in place) bit offsets
    uint32_t* total;                   // [n] bits of an image before the final padding
    unsigned long long* dst;           // [n] first byte of an image's segment in the output
    uint32_t* raw;                     // [n][raw_words] the un-stuffed bits, MSB first in every word
    unsigned raw_words;                // capacity of one image's slot of `raw`: SB blocks of block_bits bits and the restart markers' 23
                                       // each, a multiple of 4 words
    uint8_t* planes;                   // reconstruct: [n][Y | Cb | Cr] sample planes over the real blocks
    size_t bytes;
};

// code_words = 0: the workspace of the baseline codec.  Otherwise that of the coder with the caller's tables, which keeps code_words code
// words per image, never transforms or reconstructs, and so has neither flag nor planes.
inline Workspace carve(const JpegGeo& g, void* base, int block_bits = BLOCK_BITS_MAX, int code_words = 0) {
    Workspace ws{};
    uint8_t* p = (uint8_t*)base;
    // a restart marker (section 4i) costs its interval up to 7 bits of padding and its own 16
    const unsigned long words = ((unsigned long)g.SB * block_bits + 23ul * (unsigned long)jpeg_markers(g) + 31) / 32 + 1;
    ws.raw_words = (unsigned)((words + 3) & ~3ul);
    if (code_words) { ws.codes = (uint32_t*)p; p += align256((size_t)g.n * code_words * 4); }
    else { ws.flag = (uint32_t*)p; p += 256; }
    ws.off = (uint32_t*)p; p += align256((size_t)g.n * g.SB * 4);
    ws.total = (uint32_t*)p; p += align256((size_t)g.n * 4);
    ws.dst = (unsigned long long*)p; p += align256((size_t)g.n * 8);
    ws.raw = (uint32_t*)p; p += align256((size_t)g.n * ws.raw_words * 4);
    if (!code_words) { ws.planes = p; p += align256((size_t)g.n * g.NB * 64); }
    ws.bytes = (size_t)(p - (uint8_t*)base);
    return ws;
}

// ---- tables -----------------------------------------------------------------------------------------------------------
// natural index (8 * row + col) of scan position k
__constant__ const unsigned char c_nat_of_zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                                    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                                    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct QTabs { uint16_t q[2][64]; };        // [luma | chroma], natural order

// A table source is what the transform and the inverse-DCT kernel are templates over:
//   table(g, t, item, comp)   the 64 divisors, natural order, of component `comp` of image `item`; t = the thread's block in the batch
//   source(item)              the image whose pixels item `item` transforms
//   divisor(q, nat)           entry `nat` of the table q that table() returned, as the transform divides by it: the entry itself where
//                             the tables are the library's own, clamped to 1..255 where they are a caller's (jpegc_tables.hip)
// This one passes the tables of one quality for the whole batch by value in the kernel arguments.
struct BatchTables {
    QTabs qt;
    __device__ __forceinline__ const uint16_t* table(const JpegGeo&, long, int, int comp) const { return qt.q[comp ? 1 : 0]; }
    __device__ __forceinline__ int source(int item) const { return item; }
    __device__ __forceinline__ int divisor(const uint16_t* q, int nat) const { return q[nat]; }
};

// The tables of each file, for the two units that reconstruct what was read (jpegd.hip, jpegd_scaled.hip): qtabs[image][component][64],
// natural order, in global memory.  Nothing transforms with it, so it has no source() and no divisor().
struct FileTables {
    const uint16_t* qtabs;
    __device__ __forceinline__ const uint16_t* table(const JpegGeo& g, long, int img, int comp) const {
        return qtabs + ((size_t)img * g.nc + comp) * 64;
    }
};

constexpr int Q_BASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
     100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// libjpeg's tables: jpeg_quality_scaling + jpeg_add_quant_table in integers (5000 / quality is an integer division there).
// constexpr: nimg_jpeg_transform / _reconstruct pass one quality's tables by value, jpegc_items.hip builds its bank of all 100 from it
constexpr QTabs make_qtabs(int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    QTabs t{};
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 64; ++k) {
            const int v = (Q_BASE[c][k] * scale + 50) / 100;
            t.q[c][k] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    return t;
}

// ---- scans over a workgroup of SCAN_THREADS ------------------------------------------------------------------------------
// What a scan combines is a + b = "a, then b": integers, and jpegrst.h's bit-offset functions of a scan with restart markers.
__device__ __forceinline__ BitFn lane_up(const BitFn& v, int o) {
    return BitFn{__shfl_up(v.a, o, 64), __shfl_up(v.b, o, 64), __shfl_up(v.round, o, 64)};
}
template <typename T>
__device__ __forceinline__ T lane_up(T v, int o) { return __shfl_up(v, o, 64); }

// the exclusive scan of a wave from its inclusive one: integers have an inverse, functions take their neighbour's
template <typename T>
__device__ __forceinline__ T wave_excl_of(T incl, T v, int) { return incl - v; }
__device__ __forceinline__ BitFn wave_excl_of(const BitFn& incl, const BitFn&, int lane) {
    const BitFn u = lane_up(incl, 1);
    return lane ? u : BitFn{};
}

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = lane_up(v, o);
        if (lane >= o) v = u + v;
    }
    return v;
}

// exclusive scan over the NT threads of a workgroup; wtot: NT / 64 words of LDS; total = the sum of all
template <typename T, int NT = SCAN_THREADS>
__device__ __forceinline__ T block_excl_scan(T v, T* wtot, T& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const T incl = wave_incl_scan(v, lane);
    __syncthreads();                                   // the previous round's readers are done with wtot
    if (lane == 63) wtot[wv] = incl;
    __syncthreads();
    T before{}, tot{};
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) {
        const T s = wtot[k];
        if (k < wv) before = before + s;
        tot = tot + s;
    }
    total = tot;
    return before + wave_excl_of(incl, v, lane);
}

// ---- transform --------------------------------------------------------------------------------------------------------
// the reference's conversion: (255 * x).astype(uint8) in float32 after an optional x / 255; clamped where numpy would wrap
__device__ __forceinline__ int byte_of(float v, bool div) {
    if (div) v = __fdiv_rn(v, 255.0f);
    const int i = (int)__fmul_rn(255.0f, v);
    return min(max(i, 0), 255);
}

template <bool U8>
__device__ __forceinline__ void load_rgb(const void* img, int w, int y, int x, bool div, int& r, int& g, int& b) {
    const long i = ((long)y * w + x) * 3;
    if (U8) {
        const uint8_t* p = (const uint8_t*)img + i;
        r = p[0]; g = p[1]; b = p[2];
    } else {
        const float* p = (const float*)img + i;
        r = byte_of(p[0], div); g = byte_of(p[1], div); b = byte_of(p[2], div);
    }
}

// the one sample of a pixel of a grey-scale image: the byte itself, no colour conversion
template <bool U8>
__device__ __forceinline__ int load_grey(const void* img, int w, int y, int x, bool div) {
    const long i = (long)y * w + x;
    return U8 ? (int)((const uint8_t*)img)[i] : byte_of(((const float*)img)[i], div);
}

// libjpeg's fixed-point RGB -> YCbCr (jccolor.c), one sample: the luma, and Cb (comp = 1) or Cr (comp = 2)
__device__ __forceinline__ int luma_of(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int chroma_of(int comp, int r, int g, int b) {
    return comp == 1 ? (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
                     : (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// libjpeg's h2v1 / h2v2 down-sampling (jcsample.c): the sum of the 2 x vs chroma samples under reduced column x -> their mean, with
// the bias that alternates 0, 1 (h2v1) or 1, 2 (h2v2) from column to column
__device__ __forceinline__ int downsample_of(int sum, int vs, int x) { return vs == 2 ? (sum + 1 + (x & 1)) >> 2 : (sum + (x & 1)) >> 1; }

// sample (y, x) of component `comp` as the forward DCT sees it: the right edge replicated at full resolution, the bottom row up
// to a multiple of the vertical factor, chroma down-sampled, then the component's last row replicated downwards.  GREY: the one
// component of a grey-scale image - its edges replicated, nothing else
template <bool U8, bool GREY>
__device__ __forceinline__ int sample(const void* img, const JpegGeo& g, int comp, int y, int x, bool div) {
    int r, gg, b;
    if (GREY) return load_grey<U8>(img, g.w, min(y, g.h - 1), min(x, g.w - 1), div);
    if (comp == 0) {
        load_rgb<U8>(img, g.w, min(y, g.h - 1), min(x, g.w - 1), div, r, gg, b);
        return luma_of(r, gg, b);
    }
    const int cy = min(y, g.ceh - 1);
    int sum = 0;
    for (int dy = 0; dy < g.vs; ++dy)
        for (int dx = 0; dx < g.hs; ++dx) {
            load_rgb<U8>(img, g.w, min(cy * g.vs + dy, g.h - 1), min(x * g.hs + dx, g.w - 1), div, r, gg, b);
            sum += chroma_of(comp, r, gg, b);
        }
    if (g.hs == 1) return sum;
    return downsample_of(sum, g.vs, x);
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jfdctint over 8 values S apart; FIRST = the row pass (n = 11, scaled up by 2 bits), else the column pass (n = 15)
template <int S, bool FIRST>
__device__ __forceinline__ void fdct8(int* d) {
    constexpr int n = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S], t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
    const int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S], t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    d[4 * S] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    d[2 * S] = descale(z1 + t13 * 6270, n);
    d[6 * S] = descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7 * S] = descale(a4 + z1 + z3, n);
    d[5 * S] = descale(a5 + z2 + z4, n);
    d[3 * S] = descale(a6 + z2 + z3, n);
    d[S] = descale(a7 + z1 + z4, n);
}

// one pass of jidctint; n = 11 for the column pass, 18 for the row pass
template <int S>
__device__ __forceinline__ void idct8(int* d, int n) {
    int z1 = (d[2 * S] + d[6 * S]) * 4433;
    const int t2 = z1 - d[6 * S] * 15137, t3 = z1 + d[2 * S] * 6270;
    const int t0 = (d[0] + d[4 * S]) * 8192, t1 = (d[0] - d[4 * S]) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a0 = d[7 * S], a1 = d[5 * S], a2 = d[3 * S], a3 = d[S];
    z1 = a0 + a3;
    int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int z5 = (z3 + z4) * 9633;
    a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    d[0] = descale(t10 + a3, n); d[7 * S] = descale(t10 - a3, n);
    d[S] = descale(t11 + a2, n); d[6 * S] = descale(t11 - a2, n);
    d[2 * S] = descale(t12 + a1, n); d[5 * S] = descale(t12 - a1, n);
    d[3 * S] = descale(t13 + a0, n); d[4 * S] = descale(t13 - a0, n);
}

// jcdctmgr.c's quantisation of one forward-DCT output (scaled up by 8) by the table entry `divisor`: round half away from zero
__device__ __forceinline__ int quantise_coef(int v, int divisor) {
    const int qv = divisor << 3;
    const int m = (int)(((unsigned)abs(v) + (unsigned)(qv >> 1)) / (unsigned)qv);
    return v < 0 ? -m : m;
}

// real block t of the batch -> image, component, block row / column
__device__ __forceinline__ void locate(const JpegGeo& g, long t, int& img, int& comp, int& br, int& bc) {
    img = (int)(t / g.NB);
    int b = (int)(t - (long)img * g.NB);
    if (b < g.nbY) {
        comp = 0; br = b / g.bwY; bc = b - br * g.bwY;
    } else {
        b -= g.nbY;
        comp = b < g.nbC ? 1 : 2;
        b -= (comp - 1) * g.nbC;
        br = b / g.bwC; bc = b - br * g.bwC;
    }
}

// one thread per real block.  GREY (g.nc == 1): x is (n,h,w,1) - a compile-time choice, so that the colour instantiations are the
// code they were before grey-scale files were written
template <bool U8, class Tables, bool GREY = false>
__global__ void __launch_bounds__(256) jpeg_transform_kernel(const void* __restrict__ x, int16_t* __restrict__ coef, JpegGeo g, Tables tabs,
                                                             const uint32_t* __restrict__ flag) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)g.n * g.NB) return;
    int item, comp, br, bc;
    locate(g, t, item, comp, br, bc);
    const bool div = !U8 && *flag != 0;
    const int img = tabs.source(item);
    constexpr int NC = GREY ? 1 : 3;
    const void* base = U8 ? (const void*)((const uint8_t*)x + (long)img * g.h * g.w * NC)
                          : (const void*)((const float*)x + (long)img * g.h * g.w * NC);
    const uint16_t* q = tabs.table(g, t, item, comp);
    int d[64];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) d[8 * r + c] = sample<U8, GREY>(base, g, comp, 8 * br + r, 8 * bc + c, div) - 128;
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct8<1, true>(d + 8 * r);
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct8<8, false>(d + c);
    uint32_t o[32];
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int nat = c_nat_of_zz[k];
        const uint32_t c16 = (uint32_t)quantise_coef(d[nat], tabs.divisor(q, nat)) & 0xffffu;
        if (k & 1) o[k >> 1] |= c16 << 16;
        else o[k >> 1] = c16;
    }
    uint4* dst = reinterpret_cast<uint4*>(coef + t * 64);
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[j] = make_uint4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
}

// ---- reconstruct --------------------------------------------------------------------------------------------------------
// libjpeg's fixed-point YCbCr -> RGB (jdcolor.c) of one pixel, cb and cr with their 128 taken off, BEFORE the range limit
__device__ __forceinline__ int red_of(int yy, int cr) { return yy + ((91881 * cr + 32768) >> 16); }
__device__ __forceinline__ int green_of(int yy, int cb, int cr) { return yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16); }
__device__ __forceinline__ int blue_of(int yy, int cb) { return yy + ((116130 * cb + 32768) >> 16); }
// the range limit of a sample: what the inverse DCT and the colour conversion both end with
__device__ __forceinline__ int limit_byte(int v) { return min(max(v, 0), 255); }

__device__ __forceinline__ uint8_t* plane_of(uint8_t* planes, const JpegGeo& g, int img, int comp) {
    return planes + (size_t)img * g.NB * 64 + (comp ? (size_t)g.nbY * 64 + (size_t)(comp - 1) * g.nbC * 64 : 0);
}

// The arithmetic of libjpeg's "fancy" up-sampling (jdsample.c) at full-resolution column x, from the sample under the pixel (`near`)
// and its neighbour on the pixel's side (`nb`).  h2v1: (3 near + nb + 1) >> 2 at even x, + 2 at odd x.  h2v2: the column sums
// 3 near + far of both rows first, then (3 si + sn + 8) >> 4 at even x, + 7 at odd x.
__device__ __forceinline__ int fancy_h2v1(int near, int nb, int x) { return (3 * near + nb + 1 + (x & 1)) >> 2; }
__device__ __forceinline__ int fancy_column(int near, int far) { return 3 * near + far; }
__device__ __forceinline__ int fancy_h2v2(int si, int sn, int x) { return (3 * si + sn + 8 - (x & 1)) >> 4; }

// chroma sample at full-resolution (y, x): libjpeg's "fancy" triangle filter over the component's real extent; with at most two
// chroma columns libjpeg replicates instead
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, const JpegGeo& g, int y, int x) {
    const int stride = 8 * g.bwC;
    if (g.hs == 1) return p[(size_t)y * stride + x];
    const int i = x >> 1, j = g.vs == 2 ? y >> 1 : y;
    if (g.cew <= 2) return p[(size_t)j * stride + i];
    const int nb = (x & 1) ? min(i + 1, g.cew - 1) : max(i - 1, 0);
    const uint8_t* near = p + (size_t)j * stride;
    if (g.vs == 1) return fancy_h2v1(near[i], near[nb], x);
    const uint8_t* far = p + (size_t)((y & 1) ? min(j + 1, g.ceh - 1) : max(j - 1, 0)) * stride;
    const int si = fancy_column(near[i], far[i]), sn = fancy_column(near[nb], far[nb]);
    return fancy_h2v2(si, sn, x);
}

// The up-sampler of the colour pass, a compile-time choice per launch so that the instantiation that serves 1x1,
// 2x1 and 2x2 is the code it was before the other samplings were read.  jpeg_chroma_mode names libjpeg's choice (jdsample.c) for a
// geometry: 1x2 is its h1v2 triangle filter, every other integral ratio plain replication.
enum { CHROMA_FANCY = 0, CHROMA_H1V2 = 1, CHROMA_REPLICATE = 2 };
inline int jpeg_chroma_mode(const JpegGeo& g) {
    if (g.hs <= 2 && g.vs <= g.hs) return CHROMA_FANCY;
    return g.hs == 1 && g.vs == 2 ? CHROMA_H1V2 : CHROMA_REPLICATE;
}

// h1v2 "fancy": rows 2j and 2j + 1 are (3 p[j] + p[j - 1] + 1) >> 2 and (3 p[j] + p[j + 1] + 2) >> 2, the neighbour row clamped to the
// component's real extent, whatever the width
__device__ __forceinline__ int chroma_h1v2_at(const uint8_t* __restrict__ p, const JpegGeo& g, int y, int x) {
    const int stride = 8 * g.bwC, j = y >> 1;
    const int nb = (y & 1) ? min(j + 1, g.ceh - 1) : max(j - 1, 0);
    return (3 * p[(size_t)j * stride + x] + p[(size_t)nb * stride + x] + 1 + (y & 1)) >> 2;
}

// int_upsample: the sample is repeated hs times along its row and vs times down its column (both powers of two)
__device__ __forceinline__ int chroma_replicated_at(const uint8_t* __restrict__ p, const JpegGeo& g, int y, int x) {
    return p[(size_t)(y >> (g.vs == 4 ? 2 : g.vs - 1)) * (8 * g.bwC) + (x >> g.hsh)];
}

template <int UP>
__device__ __forceinline__ int chroma_sample(const uint8_t* __restrict__ p, const JpegGeo& g, int y, int x) {
    if (UP == CHROMA_H1V2) return chroma_h1v2_at(p, g, y, x);
    if (UP == CHROMA_REPLICATE) return chroma_replicated_at(p, g, y, x);
    return chroma_at(p, g, y, x);
}

// one thread per real block: dequantise, inverse DCT (columns, then rows), + 128, clamp -> the component's sample plane
template <class Tables>
__global__ void __launch_bounds__(256) jpeg_idct_kernel(const int16_t* __restrict__ coef, uint8_t* __restrict__ planes, JpegGeo g, Tables tabs) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)g.n * g.NB) return;
    int img, comp, br, bc;
    locate(g, t, img, comp, br, bc);
    const uint16_t* q = tabs.table(g, t, img, comp);
    const uint4* src = reinterpret_cast<const uint4*>(coef + t * 64);
    uint32_t wds[32];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint4 v = src[j];
        wds[4 * j] = v.x; wds[4 * j + 1] = v.y; wds[4 * j + 2] = v.z; wds[4 * j + 3] = v.w;
    }
    int d[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int nat = c_nat_of_zz[k];
        d[nat] = (int)(short)(wds[k >> 1] >> (16 * (k & 1))) * (int)q[nat];
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) idct8<8>(d + c, 11);
#pragma unroll
    for (int r = 0; r < 8; ++r) idct8<1>(d + 8 * r, 18);
    const int stride = 8 * (comp ? g.bwC : g.bwY);
    uint8_t* p = plane_of(planes, g, img, comp) + (size_t)(8 * br) * stride + 8 * bc;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            lo |= (uint32_t)limit_byte(d[8 * r + c] + 128) << (8 * c);
            hi |= (uint32_t)limit_byte(d[8 * r + 4 + c] + 128) << (8 * c);
        }
        *reinterpret_cast<uint2*>(p + (size_t)r * stride) = make_uint2(lo, hi);
    }
}

// ---- entropy coding -----------------------------------------------------------------------------------------------------
// bit sink: EMIT = false only counts.  Bits are MSB first; word j of the image's buffer holds bits 32 j .. 32 j + 31.  The first
// and the last word a block touches may be shared with its neighbours: OR-ed into zeroed memory; the words in between are its own.
// A coder derives from it and adds symbol(table, symbol, value bits, their number), which jpegopt_walk_block calls.
template <bool EMIT>
struct BitSink {
    uint32_t* base;
    unsigned widx, cap, count;
    unsigned long long acc;
    int nacc;
    bool first;
    __device__ __forceinline__ void init(uint32_t* b, unsigned cap_words, unsigned bit0) {
        base = b; cap = cap_words; widx = bit0 >> 5; nacc = (int)(bit0 & 31u); acc = 0; first = true; count = 0;
    }
    __device__ __forceinline__ void put(uint32_t v, int len) {          // len <= 27 (a code of 16 bits + 11 value bits), v < 2^len
        count += (unsigned)len;
        if (!EMIT) return;
        acc = (acc << len) | v;
        nacc += len;
        if (nacc >= 32) {
            const uint32_t word = (uint32_t)(acc >> (nacc - 32));
            if (widx < cap) {
                if (first) atomicOr(base + widx, word);
                else base[widx] = word;
            }
            first = false;
            ++widx;
            nacc -= 32;
            acc &= (1ull << nacc) - 1ull;
        }
    }
    __device__ __forceinline__ void finish() {
        if (EMIT && nacc > 0 && widx < cap) atomicOr(base + widx, (uint32_t)(acc << (32 - nacc)));
    }
};

// what an emitter adds behind scan block s, whose bits began at bit `begin`: behind the last block of the image, and of a restart
// interval that a marker follows, the byte is filled up with 1-bits
template <class Sink>
__device__ __forceinline__ void pad_interval(Sink& sink, const JpegGeo& g, int s, uint32_t begin) {
    const int pad = jpegrst_pad_bits(g, s, begin + sink.count);
    if (pad) sink.put((1u << pad) - 1u, pad);
}

inline bool grid_ok(long items, int per_block) { return (items + per_block - 1) / per_block <= 0x7fffffffL; }

}  // namespace

// ---- launches of jpegc.hip's kernels for the other units: not part of the ABI, and hidden - libnimg.so does not export them -------------
#define NIMG_HIDDEN __attribute__((visibility("hidden")))
// *flag |= 1 if any of the `count` floats at x exceeds 1 (flag zeroed here); 0 or NIMG_ERR_LAUNCH
NIMG_HIDDEN int nimg_internal_jpeg_above_one(const float* x, long count, uint32_t* flag, hipStream_t stream);
// the sample planes of g.n images (as the inverse DCT leaves them) -> y (n,h,w,g.nc): float32 k / 255, or the bytes themselves if u8
NIMG_HIDDEN int nimg_internal_jpeg_colour(uint8_t* planes, void* y, bool u8, const JpegGeo& g, hipStream_t stream);
// jpegd.hip's reconstruction with the tables of each file (what nimg_jpeg_[grey_ | sampling_]reconstruct_tables call): coef -> y
// (n,h,w,nc) as nimg_internal_jpeg_colour leaves it; the workspace is carve(g, nullptr).bytes
NIMG_HIDDEN int nimg_internal_jpeg_reconstruct_tables(const int16_t* coef, int n, int h, int w, int hs, int vs, int nc, const uint16_t* qtabs,
                                                      void* y, int out_u8, void* workspace, size_t workspace_bytes, void* stream,
                                                      int factors = JPEG_FACTORS_THREE);
// the coder's passes around its bit-length and its emit pass (a raw buffer of raw_words words per image):
// off[n][SB] bit lengths -> offsets in place, total[n]; the words of raw the bits will be OR-ed into zeroed.  With g.ri the end of an
// interval that a marker follows is rounded up to a byte and 16 bits are left free behind it.
NIMG_HIDDEN int nimg_internal_jpeg_offsets(uint32_t* off, uint32_t* total, uint32_t* raw, const JpegGeo& g, unsigned raw_words,
                                           hipStream_t stream);
// raw -> lengths[n], dst[n], and the stuffed bytes of all images back to back in out, none at or beyond capacity.  With g.ri the
// 16 free bits in front of every interval but the first (found through off) go out as FF D0 .. FF D7, unstuffed.
NIMG_HIDDEN int nimg_internal_jpeg_pack(const uint32_t* raw, const uint32_t* total, const uint32_t* off, uint32_t* lengths,
                                        unsigned long long* dst, uint8_t* out, size_t capacity, const JpegGeo& g, unsigned raw_words,
                                        hipStream_t stream);
