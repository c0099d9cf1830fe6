// What the two units of the baseline JPEG codec share (jpegc.hip: one quality per batch and the entropy coder; jpegc_items.hip: one
// quality per image): geometry and workspace layout, the quantisation tables, and the device functions of the forward and inverse
// transform.  Everything here has internal linkage - each unit compiles its own copy.
#pragma once
#include "common.h"

namespace {

constexpr int BLOCK_BITS_MAX = 1658;        // DC 9 + 11, 63 x (AC 16 + 10): the longest block with the Annex K tables
constexpr int SCAN_THREADS = 1024;

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- geometry ---------------------------------------------------------------------------------------------------------
struct Geo {
    int n, h, w, hs, vs, hsh;          // hsh = log2(hs)
    int bhY, bwY, bhC, bwC;            // real extent in blocks: ceil(ceil(W * h / hmax) / 8), the same for the height
    int ceh, cew;                      // chroma extent in samples: ceil(H / vs), ceil(W / hs)
    int my, mx, per;                   // MCU grid; blocks per MCU = hs * vs + 2
    int nbY, nbC, NB;                  // real blocks per image: Y, one chroma component, all three
    int SB;                            // blocks per image in scan order, dummies included
    unsigned raw_words;                // capacity of one image's un-stuffed bit buffer, in 32-bit words
};

bool make_geo(Geo* g, int n, int h, int w, int hs, int vs) {
    if (n < 1 || n > 65535 || h < 1 || w < 1 || h > 4096 || w > 4096) return false;
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
    g->n = n; g->h = h; g->w = w; g->hs = hs; g->vs = vs; g->hsh = hs - 1;
    g->bhY = (h + 7) / 8; g->bwY = (w + 7) / 8;
    g->ceh = (h + vs - 1) / vs; g->cew = (w + hs - 1) / hs;
    g->bhC = (g->ceh + 7) / 8; g->bwC = (g->cew + 7) / 8;
    g->my = (h + 8 * vs - 1) / (8 * vs); g->mx = (w + 8 * hs - 1) / (8 * hs);
    g->per = hs * vs + 2;
    g->nbY = g->bhY * g->bwY; g->nbC = g->bhC * g->bwC; g->NB = g->nbY + 2 * g->nbC;
    g->SB = g->my * g->mx * g->per;
    const unsigned long words = ((unsigned long)g->SB * BLOCK_BITS_MAX + 31) / 32 + 1;
    g->raw_words = (unsigned)((words + 3) & ~3ul);
    return (long)n * g->SB < 0x7fffffffL;
}

struct Workspace {
    uint32_t* flag;                    // transform: non-zero = some float sample exceeds 1
    uint32_t* off;                     // [n][SB] bit lengths, then (in place) bit offsets
    uint32_t* total;                   // [n] bits of an image before the final padding
    unsigned long long* dst;           // [n] first byte of an image's segment in the output
    uint32_t* raw;                     // [n][raw_words] the un-stuffed bits, MSB first in every word
    uint8_t* planes;                   // reconstruct: [n][Y | Cb | Cr] sample planes over the real blocks
    size_t bytes;
};

Workspace carve(const Geo& g, void* base) {
    Workspace ws;
    uint8_t* p = (uint8_t*)base;
    ws.flag = (uint32_t*)p; p += 256;
    ws.off = (uint32_t*)p; p += align256((size_t)g.n * g.SB * 4);
    ws.total = (uint32_t*)p; p += align256((size_t)g.n * 4);
    ws.dst = (unsigned long long*)p; p += align256((size_t)g.n * 8);
    ws.raw = (uint32_t*)p; p += align256((size_t)g.n * g.raw_words * 4);
    ws.planes = p; p += align256((size_t)g.n * g.NB * 64);
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
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
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
    T run = incl - v, tot = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) {
        const T s = wtot[k];
        if (k < wv) run += s;
        tot += s;
    }
    total = tot;
    return run;
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

// sample (y, x) of component `comp` as the forward DCT sees it: the right edge replicated at full resolution, the bottom row up
// to a multiple of the vertical factor, chroma down-sampled, then the component's last row replicated downwards
template <bool U8>
__device__ __forceinline__ int sample(const void* img, const Geo& g, int comp, int y, int x, bool div) {
    int r, gg, b;
    if (comp == 0) {
        load_rgb<U8>(img, g.w, min(y, g.h - 1), min(x, g.w - 1), div, r, gg, b);
        return (19595 * r + 38470 * gg + 7471 * b + 32768) >> 16;
    }
    const int cy = min(y, g.ceh - 1);
    int sum = 0;
    for (int dy = 0; dy < g.vs; ++dy)
        for (int dx = 0; dx < g.hs; ++dx) {
            load_rgb<U8>(img, g.w, min(cy * g.vs + dy, g.h - 1), min(x * g.hs + dx, g.w - 1), div, r, gg, b);
            sum += comp == 1 ? (-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16
                             : (32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
        }
    if (g.hs == 1) return sum;
    return g.vs == 2 ? (sum + 1 + (x & 1)) >> 2 : (sum + (x & 1)) >> 1;
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

// real block t of the batch -> image, component, block row / column
__device__ __forceinline__ void locate(const Geo& g, long t, int& img, int& comp, int& br, int& bc) {
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

// ---- reconstruct --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint8_t* plane_of(uint8_t* planes, const Geo& g, int img, int comp) {
    return planes + (size_t)img * g.NB * 64 + (comp ? (size_t)g.nbY * 64 + (size_t)(comp - 1) * g.nbC * 64 : 0);
}

// chroma sample at full-resolution (y, x): libjpeg's "fancy" triangle filter over the component's real extent; with at most two
// chroma columns libjpeg replicates instead
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, const Geo& g, int y, int x) {
    const int stride = 8 * g.bwC;
    if (g.hs == 1) return p[(size_t)y * stride + x];
    const int i = x >> 1, j = g.vs == 2 ? y >> 1 : y;
    if (g.cew <= 2) return p[(size_t)j * stride + i];
    const int nb = (x & 1) ? min(i + 1, g.cew - 1) : max(i - 1, 0);
    const uint8_t* near = p + (size_t)j * stride;
    if (g.vs == 1) return (3 * near[i] + near[nb] + 1 + (x & 1)) >> 2;
    const uint8_t* far = p + (size_t)((y & 1) ? min(j + 1, g.ceh - 1) : max(j - 1, 0)) * stride;
    const int si = 3 * near[i] + far[i], sn = 3 * near[nb] + far[nb];
    return (3 * si + sn + 8 - (x & 1)) >> 4;
}

inline bool grid_ok(long items, int per_block) { return (items + per_block - 1) / per_block <= 0x7fffffffL; }

}  // namespace

// ---- launches of jpegc.hip's kernels for jpegc_items.hip: not part of the ABI, and hidden - libnimg.so does not export them -------------
#define NIMG_HIDDEN __attribute__((visibility("hidden")))
// *flag |= 1 if any of the `count` floats at x exceeds 1 (flag zeroed here); 0 or NIMG_ERR_LAUNCH
NIMG_HIDDEN int nimg_internal_jpeg_above_one(const float* x, long count, uint32_t* flag, hipStream_t stream);
// the sample planes of n images (as nimg_jpeg_reconstruct's inverse DCT leaves them) -> y (n,h,w,3)
NIMG_HIDDEN int nimg_internal_jpeg_colour(uint8_t* planes, float* y, int n, int h, int w, int hs, int vs, hipStream_t stream);
// nimg_jpeg_encode's passes around the bit-length and the emit pass, for jpegc_opt.hip (a raw buffer of raw_words words per image):
// off[n][SB] bit lengths -> offsets in place, total[n]; the words of raw the bits will be OR-ed into zeroed
NIMG_HIDDEN int nimg_internal_jpeg_offsets(uint32_t* off, uint32_t* total, uint32_t* raw, int n, int SB, unsigned raw_words,
                                           hipStream_t stream);
// raw -> lengths[n], dst[n], and the stuffed bytes of all images back to back in out, none at or beyond capacity
NIMG_HIDDEN int nimg_internal_jpeg_pack(const uint32_t* raw, const uint32_t* total, uint32_t* lengths, unsigned long long* dst, uint8_t* out,
                                        size_t capacity, int n, unsigned raw_words, hipStream_t stream);
