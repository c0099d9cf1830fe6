// Pieces the differentiable JPEG translation units share - djpeg.hip (4:4:4, one kernel per direction) and djpeg_sub.hip
// (4:2:2 / 4:2:0, a chroma and a luma pass per direction): the reference's matrices, the 8-point DCT passes in the canonical
// float32 order, the rounding approximations and their gradients, the table staging, and the 8 x 64 pixel strip a wave moves
// between global memory, its private LDS rows and the registers of lane (b = lane >> 3, r = lane & 7).
//
// Both units are compiled with -ffp-contract=off (csrc/Makefile NOCONTRACT): the explicit fmaf()s are the only fused operations.
#pragma once
#include <type_traits>
#include "common.h"

namespace nimg {
namespace dj {

constexpr int STRIP_PX = 64;              // pixels per wave strip
constexpr int ROW_STRIDE = 196;           // padded LDS row stride (floats), 16-byte aligned
constexpr int STAGE_F = 8 * ROW_STRIDE;   // staging floats per wave

// Every LDS region of these kernels (staging rows, transpose tiles) is PRIVATE to one wave, and a wave's LDS operations
// complete in issue order: what has to be prevented is only the compiler moving reads above writes.  A workgroup barrier here
// would make four independent waves wait for each other twice per 8x8 transpose.
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_wave_barrier(); }

// 4-decimal DCT matrix, literal (models/jpeg.py:78-85)
__device__ constexpr float kF[8][8] = {
    {0.3536f, 0.3536f, 0.3536f, 0.3536f, 0.3536f, 0.3536f, 0.3536f, 0.3536f},
    {0.4904f, 0.4157f, 0.2778f, 0.0975f, -0.0975f, -0.2778f, -0.4157f, -0.4904f},
    {0.4619f, 0.1913f, -0.1913f, -0.4619f, -0.4619f, -0.1913f, 0.1913f, 0.4619f},
    {0.4157f, -0.0975f, -0.4904f, -0.2778f, 0.2778f, 0.4904f, 0.0975f, -0.4157f},
    {0.3536f, -0.3536f, -0.3536f, 0.3536f, 0.3536f, -0.3536f, -0.3536f, 0.3536f},
    {0.2778f, -0.4904f, 0.0975f, 0.4157f, -0.4157f, -0.0975f, 0.4904f, -0.2778f},
    {0.1913f, -0.4619f, 0.4619f, -0.1913f, -0.1913f, 0.4619f, -0.4619f, 0.1913f},
    {0.0975f, -0.2778f, 0.4157f, -0.4904f, 0.4904f, -0.4157f, 0.2778f, -0.0975f}};

// colour matrices, bias in column 0 (models/jpeg.py:74-75)
__device__ constexpr float kCF[3][4] = {{0.0f, 0.299f, 0.587f, 0.114f},
                                        {128.0f, -0.168736f, -0.331264f, 0.5f},
                                        {128.0f, 0.5f, -0.418688f, -0.081312f}};
__device__ constexpr float kCI[3][4] = {{(float)(-1.402 * 128), 1.0f, 0.0f, 1.402f},
                                        {(float)(1.058272 * 128), 1.0f, -0.344136f, -0.714136f},
                                        {(float)(-1.772 * 128), 1.0f, 1.772f, 0.0f}};

// out[k] = sum_m in[m] * F[k][m]      (forward DCT along the register axis)
__device__ __forceinline__ void dct_fwd8(const float (&in)[8], float (&out)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float acc = in[0] * kF[k][0];
#pragma unroll
        for (int m = 1; m < 8; ++m) acc = __builtin_fmaf(in[m], kF[k][m], acc);
        out[k] = acc;
    }
}
// out[m] = sum_k in[k] * F[k][m]      (inverse DCT along the register axis)
__device__ __forceinline__ void dct_inv8(const float (&in)[8], float (&out)[8]) {
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        float acc = in[0] * kF[0][m];
#pragma unroll
        for (int k = 1; k < 8; ++k) acc = __builtin_fmaf(in[k], kF[k][m], acc);
        out[m] = acc;
    }
}

struct Task {
    int n, by, x0;     // image, block row, first pixel of the strip
    bool valid;
};

__device__ __forceinline__ Task decode_task(long task, long n_tasks, int hb, int strips) {
    Task t;
    t.valid = task < n_tasks;
    const long tt = t.valid ? task : 0;
    t.x0 = (int)(tt % strips) * STRIP_PX;
    t.by = (int)((tt / strips) % hb);
    t.n = (int)(tt / ((long)strips * hb));
    return t;
}

// One strip of a task, global <-> registers: 8 rows x up to 64 px x 3 ch as 6 float4 per lane (w % 8 == 0 => 24-float = 96-byte
// block granules, always 16-byte aligned); item it * 64 + lane = (row, float4 column) of the strip.
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void fetch_strip(const float* __restrict__ src, f32x4 (&pre)[6], const Task& t, int h, int w,
                                            int lane) {
    const int strip_f = min(STRIP_PX, w - t.x0) * 3;      // valid floats per row
#pragma unroll
    for (int it = 0; it < 6; ++it) {
        const int idx = it * 64 + lane;                   // 0..383 float4 slots
        const int row = idx / 48, c4 = idx % 48;
        if (t.valid && c4 * 4 < strip_f)
            pre[it] = *reinterpret_cast<const f32x4*>(src + (((long)t.n * h + t.by * 8 + row) * w + t.x0) * 3 + c4 * 4);
    }
}
// registers -> LDS staging rows (every slot is written: lanes beyond a ragged strip stage stale values nobody reads back)
__device__ __forceinline__ void commit_strip(float* lds, const f32x4 (&pre)[6], int lane) {
#pragma unroll
    for (int it = 0; it < 6; ++it) {
        const int idx = it * 64 + lane;
        *reinterpret_cast<f32x4*>(lds + (idx / 48) * ROW_STRIDE + (idx % 48) * 4) = pre[it];
    }
}

__device__ __forceinline__ void store_strip(float* __restrict__ dst, const float* lds, const Task& t, int h, int w,
                                            int lane) {
    const int strip_f = min(STRIP_PX, w - t.x0) * 3;
#pragma unroll
    for (int it = 0; it < 6; ++it) {
        const int idx = it * 64 + lane;
        const int row = idx / 48, c4 = idx % 48;
        if (t.valid && c4 * 4 < strip_f) {
            const float4 v = *reinterpret_cast<const float4*>(lds + row * ROW_STRIDE + c4 * 4);
            *reinterpret_cast<float4*>(dst + (((long)t.n * h + t.by * 8 + row) * w + t.x0) * 3 + c4 * 4) = v;
        }
    }
}

// lane (b,r): read its 8 pixels x 3 channels from the staging rows
__device__ __forceinline__ void read_row24(const float* lds, int b, int r, float (&px)[24]) {
    const float4* p = reinterpret_cast<const float4*>(lds + r * ROW_STRIDE + b * 24);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float4 v = p[k];
        px[4 * k + 0] = v.x; px[4 * k + 1] = v.y; px[4 * k + 2] = v.z; px[4 * k + 3] = v.w;
    }
}
__device__ __forceinline__ void write_row24(float* lds, int b, int r, const float (&px)[24]) {
    float4* p = reinterpret_cast<float4*>(lds + r * ROW_STRIDE + b * 24);
#pragma unroll
    for (int k = 0; k < 6; ++k) p[k] = make_float4(px[4 * k], px[4 * k + 1], px[4 * k + 2], px[4 * k + 3]);
}

// 8x8 transposes among the 8 lanes of a block through LDS tiles [ch][block][8][9], NC channels at once
// "rows -> cols": lane (b,r) holds v[c][k] = M_c[r][k]; afterwards lane (b,r) holds M_c[k][r]  (its column r)
// T: float, or int for the integer codec's kernels (jpeg_ste.hip)
template <int NC, typename T>
__device__ __forceinline__ void transpose_tiles(T* tile, int b, int r, T (&v)[NC][8]) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int k = 0; k < 8; ++k) tile[((c * 8 + b) * 8 + r) * 9 + k] = v[c][k];
    wave_sync();
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int k = 0; k < 8; ++k) v[c][k] = tile[((c * 8 + b) * 8 + k) * 9 + r];
    wave_sync();
}

// Rounding approximations (models/jpeg.py:40-52 / 133-149).  QMODE of the forward: ROUND and SOFT both round to nearest.
enum { Q_RINT = 0, Q_SIN = 1, Q_HARMONIC = 2, Q_IDENTITY = 3 };
__host__ __device__ constexpr int fwd_mode(int rounding) {
    return rounding == NIMG_ROUND_SIN ? Q_SIN : rounding == NIMG_ROUND_HARMONIC ? Q_HARMONIC
         : rounding == NIMG_ROUND_IDENTITY ? Q_IDENTITY : Q_RINT;
}
template <int QMODE>
__device__ __forceinline__ float quantise(float u) {
    if constexpr (QMODE == Q_RINT) return rintf(u);                                     // half-to-even == tf.round
    else if constexpr (QMODE == Q_SIN) return u - sinpif(2.0f * (u - rintf(u))) * 0.15915494309189535f;   // sin(2 pi u)/(2 pi)
    else if constexpr (QMODE == Q_HARMONIC) return u - sinpif(2.0f * (u - rintf(u))) * 0.3183098861837907f;   // sin(2 pi u)/pi
    else return u;
}
// gradient modes of the backward: ROUND has none, SOFT and SIN share 1 - cos(2 pi u)
enum { G_ZERO = 0, G_SOFT = 1, G_HARMONIC = 2, G_ONE = 3 };
__host__ __device__ constexpr int bwd_mode(int rounding) {
    return rounding == NIMG_ROUND_ROUND ? G_ZERO : rounding == NIMG_ROUND_HARMONIC ? G_HARMONIC
         : rounding == NIMG_ROUND_IDENTITY ? G_ONE : G_SOFT;
}
template <int GMODE>
__device__ __forceinline__ float quantise_grad(float u) {
    if constexpr (GMODE == G_ZERO) return 0.0f;
    else if constexpr (GMODE == G_ONE) return 1.0f;
    else {
        const float c = __builtin_amdgcn_cosf(__builtin_amdgcn_fractf(u));   // v_cos_f32 takes revolutions
        return GMODE == G_SOFT ? 1.0f - c : 1.0f - 2.0f * c;
    }
}

// x / q.  EXACT = IEEE division.  Otherwise Markstein's correction of x * rc with rc = RN(1 / q): y0 = RN(x rc), r = RN(x - q y0)
// (exact in an fma), y = RN(y0 + r rc) - equal to RN(x / q) for every float x (no underflow) and every INTEGER q in 1 .. 255,
// which is checked exhaustively on the CPU (tools/probe/div_markstein_check.c: 255 divisors x 2^23 mantissas, the identity is
// invariant under scaling x by powers of two); 3 VALU instructions instead of hipcc's 11-instruction division.  x = -0 gives
// +0 (IEEE: -0): invisible in the indices, the image and the mask.  A table with any other entry takes the EXACT path.
template <bool EXACT>
__device__ __forceinline__ float div_q(float x, float q, float rc) {
    if constexpr (EXACT) return x / q;
    const float y0 = x * rc;
    const float r = __builtin_fmaf(-y0, q, x);
    return __builtin_fmaf(r, rc, y0);
}

// rgb (x255) -> ycbcr - 127, for the 8 pixels of this lane's row; out[c][j]
__device__ __forceinline__ void colour_fwd(const float (&px)[24], float (&ycc)[3][8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float r = 255.0f * px[3 * j], g = 255.0f * px[3 * j + 1], bb = 255.0f * px[3 * j + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float acc = kCF[c][0];
            acc = __builtin_fmaf(r, kCF[c][1], acc);
            acc = __builtin_fmaf(g, kCF[c][2], acc);
            acc = __builtin_fmaf(bb, kCF[c][3], acc);
            ycc[c][j] = acc - 127.0f;
        }
    }
}

// The quantisation tables of a workgroup in LDS, transposed to [c][r][u] so that lane (b, r) reads the 8 entries of its column
// with two 16-byte reads (8 distinct addresses per wave), next to their reciprocals; returns whether every entry is an integer
// in 1 .. 255 (the IJG tables: always; trainable tables: not after the first update), i.e. whether div_q<false> is exact.
// qT: 384 floats, flag: one word behind them.
__device__ __forceinline__ bool stage_tables(const float* __restrict__ qtab, float* qT, int* flag) {
    const int tid = threadIdx.x;
    if (tid == 0) *flag = 1;
    __syncthreads();
    if (tid < 192) {
        const float q = qtab[tid];
        const int c = tid >> 6, u = (tid >> 3) & 7, r = tid & 7;
        qT[(c * 8 + r) * 8 + u] = q;
        qT[192 + (c * 8 + r) * 8 + u] = 1.0f / q;
        if (!(q >= 1.0f && q <= 255.0f && q == rintf(q))) *flag = 0;
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(*flag) != 0;
}
__device__ __forceinline__ void read_tables(const float* qT, int c, int r, float (&q)[8], float (&rc)[8]) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float4 a = *reinterpret_cast<const float4*>(qT + (c * 8 + r) * 8 + 4 * k);
        const float4 b = *reinterpret_cast<const float4*>(qT + 192 + (c * 8 + r) * 8 + 4 * k);
        q[4 * k] = a.x; q[4 * k + 1] = a.y; q[4 * k + 2] = a.z; q[4 * k + 3] = a.w;
        rc[4 * k] = b.x; rc[4 * k + 1] = b.y; rc[4 * k + 2] = b.z; rc[4 * k + 3] = b.w;
    }
}

}  // namespace dj
}  // namespace nimg
