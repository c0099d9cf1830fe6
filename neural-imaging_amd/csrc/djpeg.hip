// Fused differentiable JPEG for gfx950 (CDNA4): colour transform, 8x8 block DCT, quantise, IDCT, inverse colour
// and clip in ONE kernel per direction.  Replaces models/jpeg.py:91-159 (about 25 TensorFlow ops with >=12
// materialised intermediates).  HBM-bound: forward reads 12 B + writes 12 B (+1 B mask) per pixel.
//
// Work decomposition (wave64-native):
//   one wavefront = one strip of 8 image rows x 64 pixels = 8 JPEG blocks x 3 channels
//   lane (b = lane>>3, r = lane&7) owns row r of block b for all three channels (24 values in registers)
//   pass 1 (along the row, in registers) -> 8x8 transpose through LDS (stride-9 tiles, conflict-free)
//   pass 2 (along the column, in registers) -> quantise -> inverse pass 2 -> transpose back -> inverse pass 1
//   global <-> LDS staging moves whole 768-byte row segments as float4 (coalesced), 6 per lane.
//
// CANONICAL float32 ORDER (shared with oracle/djpeg_ref.c, compared bit-for-bit on the index tensor):
//   every dot product is an fmaf chain in ascending index order starting from the first product;
//   row pass first (T = b * F^T), column pass second (X = F * T); IDCT column pass first, row pass second.
//   Compiled with -ffp-contract=off so the explicit fmaf()s are the only fused operations.
//
// The matrices, DCT passes, rounding approximations, table staging and strip movers live in djpeg.h, shared with djpeg_sub.hip.
#include "djpeg.h"

namespace {

using namespace nimg;
using namespace nimg::dj;

constexpr int TILE_F = 3 * 8 * 72;        // transpose tiles: [ch][block][8][9]
constexpr int WAVE_LDS_F = (STAGE_F > TILE_F ? STAGE_F : TILE_F);
constexpr int WAVES_PER_BLOCK = 4;
// workgroups per CU the register allocation aims at (LDS holds 5): A/B builds override these (csrc/Makefile EXTRA=)
#ifndef DJ_FWD_WGS
#define DJ_FWD_WGS 4
#endif
#ifndef DJ_BWD_WGS
#define DJ_BWD_WGS 3
#endif

__device__ __forceinline__ void transpose24(float* tile, int b, int r, float (&v)[3][8]) { transpose_tiles<3>(tile, b, r, v); }

// column pass, quantisation, inverse column pass of one wave task (v: T columns in, S columns out)
template <int QMODE, bool EXACT>
__device__ __forceinline__ void quantise_columns(float (&v)[3][8], const float* qT, const Task& t, int b, int r, int hb, int wb,
                                                 int16_t* __restrict__ idx, float* __restrict__ xdq) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float X[8], q[8], rc[8];
        dct_fwd8(v[c], X);                                       // X[u][col r] = sum_i F[u][i] T[i][r]
        read_tables(qT, c, r, q, rc);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float qi = quantise<QMODE>(div_q<EXACT>(X[u], q[u], rc[u]));
            X[u] = qi * q[u];
            if (idx || xdq) {
                const long o = ((((long)t.n * 3 + c) * hb + t.by) * wb + (t.x0 / 8 + b)) * 64 + u * 8 + r;
                if (idx) idx[o] = (int16_t)qi;
                if (xdq) xdq[o] = X[u];
            }
        }
        dct_inv8(X, v[c]);                                       // S[i][col r] = sum_u F[u][i] Xd[u][r]
    }
}

// One task per wave; the 5 workgroups a CU holds (LDS) overlap one wave's memory round trip with the others' arithmetic.
template <int QMODE>
__global__ __launch_bounds__(256, DJ_FWD_WGS) void djpeg_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                        const float* __restrict__ qtab, uint8_t* __restrict__ mask,
                                                        int16_t* __restrict__ idx, float* __restrict__ xdq, int n,
                                                        int h, int w) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = lane >> 3, r = lane & 7;
    float* lds = smem + wave * WAVE_LDS_F;
    float* qT = smem + WAVES_PER_BLOCK * WAVE_LDS_F;
    const int hb = h / 8, wb = w / 8, strips = (w + STRIP_PX - 1) / STRIP_PX;
    const long n_tasks = (long)n * hb * strips;
    const Task t = decode_task((long)blockIdx.x * WAVES_PER_BLOCK + wave, n_tasks, hb, strips);
    const bool active = t.valid && (t.x0 + b * 8 < w);
    constexpr float kRc255 = 1.0f / 255.0f;

    f32x4 pre[6] = {};
    fetch_strip(x, pre, t, h, w, lane);                              // in flight while the tables are staged
    const bool fast = stage_tables(qtab, qT, reinterpret_cast<int*>(qT + 384));
    commit_strip(lds, pre, lane);
    wave_sync();
    float px[24];
    float v[3][8];
    read_row24(lds, b, r, px);
    wave_sync();
    {
        float ycc[3][8];
        colour_fwd(px, ycc);
#pragma unroll
        for (int c = 0; c < 3; ++c) dct_fwd8(ycc[c], v[c]);          // T[r][k] = sum_j b[r][j] F[k][j]
    }
    transpose24(lds, b, r, v);                                       // lane now holds T[0..7][col r]
    if (active) {
        if (fast) quantise_columns<QMODE, false>(v, qT, t, b, r, hb, wb, idx, xdq);
        else quantise_columns<QMODE, true>(v, qT, t, b, r, hb, wb, idx, xdq);
    }
    transpose24(lds, b, r, v);                                       // lane holds S[row r][0..7]
    {
        float q3[3][8];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            dct_inv8(v[c], q3[c]);                                   // xi[r][j] = sum_v S[r][v] F[v][j]
#pragma unroll
            for (int j = 0; j < 8; ++j) q3[c][j] += 127.0f;
        }
        uint32_t mlo = 0, mhi = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            uint32_t m = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float acc = kCI[c][0];
                acc = __builtin_fmaf(q3[0][j], kCI[c][1], acc);
                acc = __builtin_fmaf(q3[1][j], kCI[c][2], acc);
                acc = __builtin_fmaf(q3[2][j], kCI[c][3], acc);
                acc = div_q<false>(acc, 255.0f, kRc255);
                const float cl = __builtin_amdgcn_fmed3f(acc, 0.0f, 1.0f);          // = fminf(fmaxf(acc, 0), 1)
                m |= cl == acc ? (1u << c) : 0u;                                    // inside [0, 1]: the clip passes the gradient
                px[3 * j + c] = cl;
            }
            if (j < 4) mlo |= m << (8 * j); else mhi |= m << (8 * (j - 4));
        }
        write_row24(lds, b, r, px);
        if (mask && active)
            *reinterpret_cast<uint2*>(mask + ((long)t.n * h + t.by * 8 + r) * w + t.x0 + b * 8) = make_uint2(mlo, mhi);
    }
    wave_sync();
    store_strip(y, lds, t, h, w, lane);
}

// DQ: also the gradient of the quantisation tables (trainable=True, models/jpeg.py:57-62; X' = quant(X / Q) * Q at :129-131):
// d X' / d Q = quant(z) - z quant'(z) with z = X / Q, summed over every block of the luma / of both chroma channels.  A lane
// holds column r of its block, so it accumulates 2 x 8 table entries (u, r); the 8 blocks of the wave are folded with three
// shuffles and lanes 0..7 write the wave's 128 partial sums (dq_partial[task][cls][u][r]); a fixed-order reduction finishes.
// Always the IEEE division (trained tables are not integers).
template <int RND, bool DQ>
__global__ __launch_bounds__(256, DQ ? 3 : DJ_BWD_WGS) void djpeg_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                        const uint8_t* __restrict__ mask,
                                                        const float* __restrict__ qtab, float* __restrict__ gx,
                                                        float* __restrict__ dq_partial, int n, int h, int w) {
    constexpr int GMODE = bwd_mode(RND), QMODE = fwd_mode(RND);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = lane >> 3, r = lane & 7;
    float* lds = smem + wave * WAVE_LDS_F;
    float* qT = smem + WAVES_PER_BLOCK * WAVE_LDS_F;
    const int hb = h / 8, strips = (w + STRIP_PX - 1) / STRIP_PX;
    const long n_tasks = (long)n * hb * strips;
    const Task t = decode_task((long)blockIdx.x * WAVES_PER_BLOCK + wave, n_tasks, hb, strips);
    const bool active = t.valid && (t.x0 + b * 8 < w);
    f32x4 pre[6] = {};
    fetch_strip(x, pre, t, h, w, lane);                              // in flight while the tables are staged
    const bool fast = stage_tables(qtab, qT, reinterpret_cast<int*>(qT + 384)) && !DQ;

    float px[24];
    float tx[3][8];    // forward coefficients path (from x)
    float tg[3][8];    // gradient path (from gy)
    // ---- recompute the forward row pass from x
    commit_strip(lds, pre, lane);
    fetch_strip(gy, pre, t, h, w, lane);                             // the gradient strip arrives under the first row pass
    uint2 mm = make_uint2(0u, 0u);
    if (active) mm = *reinterpret_cast<const uint2*>(mask + ((long)t.n * h + t.by * 8 + r) * w + t.x0 + b * 8);
    wave_sync();
    read_row24(lds, b, r, px);
    wave_sync();
    {
        float ycc[3][8];
        colour_fwd(px, ycc);
#pragma unroll
        for (int c = 0; c < 3; ++c) dct_fwd8(ycc[c], tx[c]);
    }
    // ---- gradient: clip mask, /255, transpose(colour_I), row pass (d xi = F^T dXd F  =>  dXd = F g F^T)
    commit_strip(lds, pre, lane);
    wave_sync();
    read_row24(lds, b, r, px);
    wave_sync();
    {
#pragma clang fp contract(fast)       // gradient arithmetic carries no bit-exact contract (the recomputed forward above does)
        float gq[3][8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t m = ((j < 4 ? mm.x >> (8 * j) : mm.y >> (8 * (j - 4)))) & 0xffu;
            float g[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] = (m >> c) & 1u ? px[3 * j + c] * (1.0f / 255.0f) : 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c)       // d/d(q_c) = sum_c' g_c' * CI[c'][1+c]
                gq[c][j] = g[0] * kCI[0][1 + c] + g[1] * kCI[1][1 + c] + g[2] * kCI[2][1 + c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dct_fwd8(gq[c], tg[c]);
    }
    transpose24(lds, b, r, tx);
    transpose24(lds, b, r, tg);
    float dqa[DQ ? 2 : 1][8];
    if constexpr (DQ) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int u = 0; u < 8; ++u) dqa[k][u] = 0.0f;
    }
    if (active) {
        auto columns = [&](auto exact) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float X[8], G[8], q[8], rc[8];
                dct_fwd8(tx[c], X);
                dct_fwd8(tg[c], G);
                read_tables(qT, c, r, q, rc);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float z = div_q<decltype(exact)::value>(X[u], q[u], rc[u]);
                    const float qg = quantise_grad<GMODE>(z);
                    if constexpr (DQ) dqa[c == 0 ? 0 : 1][u] += G[u] * (quantise<QMODE>(z) - z * qg);
                    G[u] *= qg;                                      // (X/Q -> quant -> *Q): the Q factors cancel
                }
                dct_inv8(G, tg[c]);                                  // d b = F^T gX F : column pass
            }
        };
        if (fast) columns(std::false_type{});
        else columns(std::true_type{});
    }
    if constexpr (DQ) {
        const long task = (long)blockIdx.x * WAVES_PER_BLOCK + wave;
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                float v = dqa[k][u];
                v += __shfl_xor(v, 8, 64);
                v += __shfl_xor(v, 16, 64);
                v += __shfl_xor(v, 32, 64);
                if (lane < 8) dq_partial[task * 128 + (k * 8 + u) * 8 + r] = v;
            }
    }
    transpose24(lds, b, r, tg);
    {
#pragma clang fp contract(fast)
        float gb[3][8];
#pragma unroll
        for (int c = 0; c < 3; ++c) dct_inv8(tg[c], gb[c]);          // row pass
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c)       // d/d(x_c) = 255 * sum_c' gycc_c' * CF[c'][1+c]
                px[3 * j + c] =
                    255.0f * (gb[0][j] * kCF[0][1 + c] + gb[1][j] * kCF[1][1 + c] + gb[2][j] * kCF[2][1 + c]);
        write_row24(lds, b, r, px);
    }
    wave_sync();
    store_strip(gx, lds, t, h, w, lane);
}

inline int persistent_grid(long tasks) { return (int)((tasks + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK); }   // one task per wave
constexpr size_t kLds = ((size_t)WAVES_PER_BLOCK * WAVE_LDS_F + 384 + 4) * sizeof(float);

template <bool DQ, typename... A>
void launch_bwd(int rounding, int grid, hipStream_t s, A... a) {
    const dim3 g(grid), b(256);
    switch (rounding) {
        case NIMG_ROUND_ROUND: hipLaunchKernelGGL((djpeg_bwd_kernel<NIMG_ROUND_ROUND, DQ>), g, b, kLds, s, a...); break;
        case NIMG_ROUND_SIN:                               // without the table gradient SIN and SOFT are one kernel
            if constexpr (DQ) { hipLaunchKernelGGL((djpeg_bwd_kernel<NIMG_ROUND_SIN, DQ>), g, b, kLds, s, a...); break; }
            [[fallthrough]];
        case NIMG_ROUND_SOFT: hipLaunchKernelGGL((djpeg_bwd_kernel<NIMG_ROUND_SOFT, DQ>), g, b, kLds, s, a...); break;
        case NIMG_ROUND_HARMONIC: hipLaunchKernelGGL((djpeg_bwd_kernel<NIMG_ROUND_HARMONIC, DQ>), g, b, kLds, s, a...); break;
        default: hipLaunchKernelGGL((djpeg_bwd_kernel<NIMG_ROUND_IDENTITY, DQ>), g, b, kLds, s, a...); break;
    }
}

}  // namespace

extern "C" {

int nimg_djpeg_fwd(const float* x, float* y, const float* qtab, uint8_t* mask, int16_t* idx, float* xdq, int n,
                   int h, int w, int rounding, void* stream) {
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    if (!x || !y || !qtab || n < 0 || h <= 0 || w <= 0 || (h % 8) || (w % 8)) return NIMG_ERR_ARG;
    if (rounding < NIMG_ROUND_ROUND || rounding > NIMG_ROUND_IDENTITY) return NIMG_ERR_ARG;
    const long tasks = (long)n * (h / 8) * ((w + STRIP_PX - 1) / STRIP_PX);
    const dim3 grid(persistent_grid(tasks)), block(256);
    hipStream_t s = (hipStream_t)stream;
    switch (fwd_mode(rounding)) {
        case Q_RINT: hipLaunchKernelGGL(djpeg_fwd_kernel<Q_RINT>, grid, block, kLds, s, x, y, qtab, mask, idx, xdq, n, h, w); break;
        case Q_SIN: hipLaunchKernelGGL(djpeg_fwd_kernel<Q_SIN>, grid, block, kLds, s, x, y, qtab, mask, idx, xdq, n, h, w); break;
        case Q_HARMONIC:
            hipLaunchKernelGGL(djpeg_fwd_kernel<Q_HARMONIC>, grid, block, kLds, s, x, y, qtab, mask, idx, xdq, n, h, w);
            break;
        default: hipLaunchKernelGGL(djpeg_fwd_kernel<Q_IDENTITY>, grid, block, kLds, s, x, y, qtab, mask, idx, xdq, n, h, w); break;
    }
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_djpeg_bwd(const float* x, const float* gy, const uint8_t* mask, const float* qtab, float* gx, int n, int h,
                   int w, int rounding, void* stream) {
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    if (!x || !gy || !mask || !qtab || !gx || n < 0 || h <= 0 || w <= 0 || (h % 8) || (w % 8)) return NIMG_ERR_ARG;
    if (rounding < NIMG_ROUND_ROUND || rounding > NIMG_ROUND_IDENTITY) return NIMG_ERR_ARG;
    const long tasks = (long)n * (h / 8) * ((w + STRIP_PX - 1) / STRIP_PX);
    launch_bwd<false>(rounding, persistent_grid(tasks), (hipStream_t)stream, x, gy, mask, qtab, gx, (float*)nullptr, n, h, w);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

size_t nimg_djpeg_dq_workspace_bytes(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    const long tasks = (long)n * (h / 8) * ((w + STRIP_PX - 1) / STRIP_PX);
    return (size_t)nimg::cdiv(tasks, WAVES_PER_BLOCK) * WAVES_PER_BLOCK * 128 * sizeof(float);
}

int nimg_djpeg_bwd_dq(const float* x, const float* gy, const uint8_t* mask, const float* qtab, float* gx, float* dq,
                      int n, int h, int w, int rounding, int accumulate, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (n == 0) return NIMG_OK;
    if (!x || !gy || !mask || !qtab || !gx || !dq || !workspace || n < 0 || h <= 0 || w <= 0 || (h % 8) || (w % 8))
        return NIMG_ERR_ARG;
    if (rounding < NIMG_ROUND_ROUND || rounding > NIMG_ROUND_IDENTITY) return NIMG_ERR_ARG;
    if (workspace_bytes < nimg_djpeg_dq_workspace_bytes(n, h, w)) return NIMG_ERR_WORKSPACE;
    const long tasks = (long)n * (h / 8) * ((w + STRIP_PX - 1) / STRIP_PX);
    const int grid = persistent_grid(tasks);
    launch_bwd<true>(rounding, grid, (hipStream_t)stream, x, gy, mask, qtab, gx, (float*)workspace, n, h, w);
    NIMG_CHECK_LAUNCH();
    nimg::launch_reduce2((const float*)workspace, dq, 128, grid * WAVES_PER_BLOCK, nullptr, nullptr, 0, 0, accumulate,
                         (hipStream_t)stream);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

// IJG quality scaling (compression/jpeg_helpers.py:264-305), host side
int nimg_jpeg_qtable(int quality, int channel, float* out64) {
    static const float luma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
                                   14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
    static const float chroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                                     24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
    if (!out64) return NIMG_ERR_ARG;
    quality = quality > 100 ? 100 : (quality < 1 ? 1 : quality);
    const float s = quality < 50 ? (float)(5000.0 / quality) : (float)(200 - 2 * quality);
    const float* t = channel == 0 ? luma : chroma;
    for (int k = 0; k < 64; ++k) {
        float v = __builtin_floorf((t[k] * s + 50.0f) / 100.0f);
        out64[k] = v < 1.0f ? 1.0f : (v > 255.0f ? 255.0f : v);
    }
    return NIMG_OK;
}

}  // extern "C"
