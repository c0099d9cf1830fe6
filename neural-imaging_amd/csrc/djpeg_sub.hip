// Differentiable JPEG with chroma sub-sampling (4:2:2 = 2x1, 4:2:0 = 2x2) for gfx950 (CDNA4): the float, differentiable form
// of what csrc/jpegc.hip / jpegd.hip do in integers - box down-sampling of Cb / Cr, the 8x8 block path of djpeg.hip on the
// reduced planes, libjpeg's "fancy" triangle up-sampling - forward and backward, two launches per direction.
//
//   forward   chroma pass: a wave owns 8 chroma blocks of one block row (64 x 8 reduced samples = 128 x 8 VS pixels); lane
//                          (b, r) owns row r of block b: reads the 16 x VS pixels under it, Cb / Cr, mean, row DCT, transpose,
//                          column DCT, quantise, inverse passes, and writes its 8 reconstructed samples of both reduced planes
//                          to the workspace [n][2][h / VS][w / 2] (plus the chroma idx / xdq blocks)
//             luma pass:   the 8 x 64 pixel strip of djpeg.hip; the Y path in registers; lane (b, r) reads the 4 reduced
//                          samples under its 8 pixels with a one-sample halo (clamped at the component's edge = libjpeg's edge
//                          rule), up-samples down the columns, then along the rows, inverse colour, clip, mask, store
//   backward  chroma pass: lane (b, r) gathers gy and the mask over the 18 x (VS == 2 ? 4 : 1) pixel window of its 8 reduced
//                          samples (clamped indices: the edge samples collect the replicated taps), applies mask, / 255, the
//                          inverse-colour transpose and the filter adjoint, recomputes the chroma DCT from x, runs the block
//                          backward and writes g / (2 VS) to the reduced gradient planes; chroma half of dq per wave
//             luma pass:   per strip the Y backward in registers, + the reduced gradient under each pixel, colour transpose,
//                          gx; luma half of dq per wave
//
// Every LDS region is private to a wave (djpeg.h wave_sync).  The workspace is the caller's: no allocation, capturable.
// Compiled with -ffp-contract=off like djpeg.hip: the forward shares its canonical fmaf order through djpeg.h.
#include "djpeg.h"

namespace {

using namespace nimg;
using namespace nimg::dj;

constexpr int WAVES_PER_BLOCK = 4;
constexpr int CTILE_F = 2 * 8 * 72;       // chroma passes: transpose tiles [Cb, Cr][block][8][9] per wave
constexpr int LWAVE_F = STAGE_F;          // luma passes: the staging rows of a strip (the one transpose tile fits inside)
constexpr size_t kLdsChroma = ((size_t)WAVES_PER_BLOCK * CTILE_F + 384 + 4) * sizeof(float);
constexpr size_t kLdsLuma = ((size_t)WAVES_PER_BLOCK * LWAVE_F + 384 + 4) * sizeof(float);

// geometry of one call; h % (8 vs) == 0 and w % 16 == 0
struct Geo {
    int h, w, hc, wc;          // image and reduced-plane extent
    int hb, wb, hcb, wcb;      // blocks
    int strips, cstrips;       // wave strips per block row: luma (64 px), chroma (64 reduced samples)
    long blocks_img;           // blocks per image: Y | Cb | Cr
};
__host__ __device__ inline Geo make_geo(int h, int w, int vs) {
    Geo g;
    g.h = h; g.w = w; g.hc = h / vs; g.wc = w / 2;
    g.hb = h / 8; g.wb = w / 8; g.hcb = g.hc / 8; g.wcb = g.wc / 8;
    g.strips = (w + STRIP_PX - 1) / STRIP_PX;
    g.cstrips = (g.wc + STRIP_PX - 1) / STRIP_PX;
    g.blocks_img = (long)g.hb * g.wb + 2L * g.hcb * g.wcb;
    return g;
}

// column pass, quantisation, inverse column pass of one block column (v: T column in, S column out); `o` is the block's
// first element in idx / xdq, `c` the table
template <int QMODE, bool EXACT>
__device__ __forceinline__ void quantise_block(float (&v)[8], const float* qT, int c, int r, int16_t* __restrict__ idx,
                                               float* __restrict__ xdq, long o) {
    float X[8], q[8], rc[8];
    dct_fwd8(v, X);
    read_tables(qT, c, r, q, rc);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const float qi = quantise<QMODE>(div_q<EXACT>(X[u], q[u], rc[u]));
        X[u] = qi * q[u];
        if (idx) idx[o + u * 8 + r] = (int16_t)qi;
        if (xdq) xdq[o + u * 8 + r] = X[u];
    }
    dct_inv8(X, v);
}

// lane (b, r) of a chroma task: Cb and Cr of the 16 x VS pixels under its 8 reduced samples, averaged (libjpeg's h2v1 / h2v2
// without the integer bias); cc[c][j].  12 float4 per pixel row: w % 16 == 0 keeps every 48-float granule 16-byte aligned.
template <int VS>
__device__ __forceinline__ void reduced_chroma(const float* __restrict__ x, const Task& t, const Geo& g, int b, int r, bool active,
                                               float (&cc)[2][8]) {
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) cc[c][j] = 0.0f;
#pragma unroll
    for (int vv = 0; vv < VS; ++vv) {
        f32x4 raw[12] = {};
        if (active) {
            const f32x4* p = reinterpret_cast<const f32x4*>(
                x + (((long)t.n * g.h + (t.by * 8 + r) * VS + vv) * g.w + (t.x0 + b * 8) * 2) * 3);
#pragma unroll
            for (int k = 0; k < 12; ++k) raw[k] = p[k];
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float px[24], ycc[3][8];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                px[4 * k] = raw[half * 6 + k].x; px[4 * k + 1] = raw[half * 6 + k].y;
                px[4 * k + 2] = raw[half * 6 + k].z; px[4 * k + 3] = raw[half * 6 + k].w;
            }
            colour_fwd(px, ycc);
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) cc[c][half * 4 + j] += ycc[1 + c][2 * j] + ycc[1 + c][2 * j + 1];
        }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) cc[c][j] *= (VS == 2 ? 0.25f : 0.5f);
}

template <int QMODE, int VS>
__global__ __launch_bounds__(256) void djs_fwd_chroma_kernel(const float* __restrict__ x, const float* __restrict__ qtab,
                                                             float* __restrict__ planes, int16_t* __restrict__ idx,
                                                             float* __restrict__ xdq, int n, int h, int w) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = lane >> 3, r = lane & 7;
    float* tile = smem + wave * CTILE_F;
    float* qT = smem + WAVES_PER_BLOCK * CTILE_F;
    const Geo g = make_geo(h, w, VS);
    const long n_tasks = (long)n * g.hcb * g.cstrips;
    const Task t = decode_task((long)blockIdx.x * WAVES_PER_BLOCK + wave, n_tasks, g.hcb, g.cstrips);
    const bool active = t.valid && (t.x0 + b * 8 < g.wc);

    float cc[2][8], v[2][8];
    reduced_chroma<VS>(x, t, g, b, r, active, cc);
    const bool fast = stage_tables(qtab, qT, reinterpret_cast<int*>(qT + 384));
#pragma unroll
    for (int c = 0; c < 2; ++c) dct_fwd8(cc[c], v[c]);
    transpose_tiles<2>(tile, b, r, v);
    if (active) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const long o = ((long)t.n * g.blocks_img + (long)g.hb * g.wb + (long)c * g.hcb * g.wcb + (long)t.by * g.wcb +
                            (t.x0 / 8 + b)) * 64;
            if (fast) quantise_block<QMODE, false>(v[c], qT, 1 + c, r, idx, xdq, o);
            else quantise_block<QMODE, true>(v[c], qT, 1 + c, r, idx, xdq, o);
        }
    }
    transpose_tiles<2>(tile, b, r, v);
    if (active) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float o8[8];
            dct_inv8(v[c], o8);
            float4* dst = reinterpret_cast<float4*>(planes + (((long)t.n * 2 + c) * g.hc + t.by * 8 + r) * g.wc + t.x0 + b * 8);
            dst[0] = make_float4(o8[0], o8[1], o8[2], o8[3]);
            dst[1] = make_float4(o8[4], o8[5], o8[6], o8[7]);
        }
    }
}

template <int QMODE, int VS>
__global__ __launch_bounds__(256) void djs_fwd_luma_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                           const float* __restrict__ qtab, const float* __restrict__ planes,
                                                           uint8_t* __restrict__ mask, int16_t* __restrict__ idx,
                                                           float* __restrict__ xdq, int n, int h, int w) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = lane >> 3, r = lane & 7;
    float* lds = smem + wave * LWAVE_F;
    float* qT = smem + WAVES_PER_BLOCK * LWAVE_F;
    const Geo g = make_geo(h, w, VS);
    const long n_tasks = (long)n * g.hb * g.strips;
    const Task t = decode_task((long)blockIdx.x * WAVES_PER_BLOCK + wave, n_tasks, g.hb, g.strips);
    const bool active = t.valid && (t.x0 + b * 8 < w);
    constexpr float kRc255 = 1.0f / 255.0f;
    constexpr int NR = VS == 2 ? 2 : 1;

    f32x4 pre[6] = {};
    fetch_strip(x, pre, t, h, w, lane);
    // the reduced samples under this lane's 8 pixels, with the one-sample halo: [c][own row, neighbour row][-1 .. 4]
    float cs[2][NR][6] = {};
    if (active) {
        const int py = t.by * 8 + r, cc0 = (t.x0 + b * 8) / 2;
        int rows[NR];
        rows[0] = py / VS;
        if constexpr (VS == 2) rows[1] = (py & 1) ? min(rows[0] + 1, g.hc - 1) : max(rows[0] - 1, 0);
        const int left = max(cc0 - 1, 0), right = min(cc0 + 4, g.wc - 1);
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                const float* base = planes + (((long)t.n * 2 + c) * g.hc + rows[k]) * g.wc;
                const float4 m = *reinterpret_cast<const float4*>(base + cc0);
                cs[c][k][0] = base[left];
                cs[c][k][1] = m.x; cs[c][k][2] = m.y; cs[c][k][3] = m.z; cs[c][k][4] = m.w;
                cs[c][k][5] = base[right];
            }
    }
    const bool fast = stage_tables(qtab, qT, reinterpret_cast<int*>(qT + 384));
    commit_strip(lds, pre, lane);
    wave_sync();
    float px[24];
    float v[1][8];
    read_row24(lds, b, r, px);
    wave_sync();
    {
        float ycc[3][8];
        colour_fwd(px, ycc);
        dct_fwd8(ycc[0], v[0]);
    }
    transpose_tiles<1>(lds, b, r, v);
    if (active) {
        const long o = ((long)t.n * g.blocks_img + (long)t.by * g.wb + (t.x0 / 8 + b)) * 64;
        if (fast) quantise_block<QMODE, false>(v[0], qT, 0, r, idx, xdq, o);
        else quantise_block<QMODE, true>(v[0], qT, 0, r, idx, xdq, o);
    }
    transpose_tiles<1>(lds, b, r, v);
    {
        float q3[3][8];
        dct_inv8(v[0], q3[0]);
#pragma unroll
        for (int j = 0; j < 8; ++j) q3[0][j] += 127.0f;
        // triangle filter: down the columns (4:2:0), then along the rows
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float t6[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                if constexpr (VS == 2) t6[k] = 0.75f * cs[c][0][k] + 0.25f * cs[c][1][k];
                else t6[k] = cs[c][0][k];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                q3[1 + c][2 * j] = (0.75f * t6[1 + j] + 0.25f * t6[j]) + 127.0f;
                q3[1 + c][2 * j + 1] = (0.75f * t6[1 + j] + 0.25f * t6[2 + j]) + 127.0f;
            }
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
                const float cl = __builtin_amdgcn_fmed3f(acc, 0.0f, 1.0f);
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

// the block backward of one column: G (gradient, column of F g F^T so far) and X (forward coefficients) in, the gradient before
// the forward column pass out; accumulates d/dQ into dqa when DQ
template <int RND, bool DQ, bool EXACT>
__device__ __forceinline__ void backward_block(float (&tx)[8], float (&tg)[8], const float* qT, int c, int r, float (&dqa)[8]) {
    constexpr int GMODE = bwd_mode(RND), QMODE = fwd_mode(RND);
    float X[8], G[8], q[8], rc[8];
    dct_fwd8(tx, X);
    dct_fwd8(tg, G);
    read_tables(qT, c, r, q, rc);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const float z = div_q<EXACT>(X[u], q[u], rc[u]);
        const float qg = quantise_grad<GMODE>(z);
        if constexpr (DQ) dqa[u] += G[u] * (quantise<QMODE>(z) - z * qg);
        G[u] *= qg;                                      // (X/Q -> quant -> *Q): the Q factors cancel
    }
    dct_inv8(G, tg);
}

// the 8 blocks of a wave folded with three shuffles; lanes 0..7 write the wave's 64 partial sums [u][r]
__device__ __forceinline__ void store_dq_partial(float* __restrict__ part, const float (&dqa)[8], int lane, int r) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        float v = dqa[u];
        v += __shfl_xor(v, 8, 64);
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (lane < 8) part[u * 8 + r] = v;
    }
}

template <int RND, bool DQ, int VS>
__global__ __launch_bounds__(256) void djs_bwd_chroma_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                             const uint8_t* __restrict__ mask, const float* __restrict__ qtab,
                                                             float* __restrict__ gplanes, float* __restrict__ dq_partial, int n,
                                                             int h, int w) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = lane >> 3, r = lane & 7;
    float* tile = smem + wave * CTILE_F;
    float* qT = smem + WAVES_PER_BLOCK * CTILE_F;
    const Geo g = make_geo(h, w, VS);
    const long n_tasks = (long)n * g.hcb * g.cstrips;
    const Task t = decode_task((long)blockIdx.x * WAVES_PER_BLOCK + wave, n_tasks, g.hcb, g.cstrips);
    const bool active = t.valid && (t.x0 + b * 8 < g.wc);

    float tx[2][8], tg[2][8];
    {
        float cc[2][8];
        reduced_chroma<VS>(x, t, g, b, r, active, cc);
#pragma unroll
        for (int c = 0; c < 2; ++c) dct_fwd8(cc[c], tx[c]);
    }
    const bool fast = stage_tables(qtab, qT, reinterpret_cast<int*>(qT + 384)) && !DQ;
    {
#pragma clang fp contract(fast)       // gradient arithmetic carries no bit-exact contract
        // adjoint of the triangle filter = a gather with clamped indices: reduced sample (i, j) collects
        // (1/4, 3/4, 3/4, 1/4) of the pixels 2j - 1 .. 2j + 2 of each row, rows 2i - 1 .. 2i + 2 weighted alike (4:2:0)
        constexpr int NR = VS == 2 ? 4 : 1;
        float gq[2][8];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int j = 0; j < 8; ++j) gq[c][j] = 0.0f;
        if (active) {
            const int ci = t.by * 8 + r, X0 = (t.x0 + b * 8) * 2;
            const int left = max(X0 - 1, 0), right = min(X0 + 16, w - 1);
#pragma nounroll                      // one pixel row in registers at a time: unrolled, the four rows' loads cost the occupancy
            for (int k = 0; k < NR; ++k) {
                const int py = VS == 2 ? min(max(2 * ci - 1 + k, 0), h - 1) : ci;
                const float wgt = VS == 2 ? ((k == 0 || k == 3) ? 0.25f : 0.75f) : 1.0f;
                const long row = ((long)t.n * h + py) * w;
                float gp[18][3];
                uint32_t mb[18];
                {
                    const f32x4* p = reinterpret_cast<const f32x4*>(gy + (row + X0) * 3);
                    float flat[48];
#pragma unroll
                    for (int q4 = 0; q4 < 12; ++q4) {
                        const f32x4 vv = p[q4];
                        flat[4 * q4] = vv.x; flat[4 * q4 + 1] = vv.y; flat[4 * q4 + 2] = vv.z; flat[4 * q4 + 3] = vv.w;
                    }
                    const uint4 mm = *reinterpret_cast<const uint4*>(mask + row + X0);
                    const uint32_t mw[4] = {mm.x, mm.y, mm.z, mm.w};
#pragma unroll
                    for (int p16 = 0; p16 < 16; ++p16) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) gp[1 + p16][c] = flat[3 * p16 + c];
                        mb[1 + p16] = (mw[p16 >> 2] >> (8 * (p16 & 3))) & 0xffu;
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        gp[0][c] = gy[(row + left) * 3 + c];
                        gp[17][c] = gy[(row + right) * 3 + c];
                    }
                    mb[0] = mask[row + left];
                    mb[17] = mask[row + right];
                }
                float gc[2][18];
#pragma unroll
                for (int p = 0; p < 18; ++p) {
                    float gm[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) gm[c] = (mb[p] >> c) & 1u ? gp[p][c] * (1.0f / 255.0f) : 0.0f;
#pragma unroll
                    for (int c = 0; c < 2; ++c)       // d/d(q_c) = sum_c' g_c' * CI[c'][1+c], c = Cb, Cr
                        gc[c][p] = gm[0] * kCI[0][2 + c] + gm[1] * kCI[1][2 + c] + gm[2] * kCI[2][2 + c];
                }
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        gq[c][j] += wgt * (0.25f * (gc[c][2 * j] + gc[c][2 * j + 3]) + 0.75f * (gc[c][2 * j + 1] + gc[c][2 * j + 2]));
            }
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) dct_fwd8(gq[c], tg[c]);
    }
    transpose_tiles<2>(tile, b, r, tx);
    transpose_tiles<2>(tile, b, r, tg);
    float dqa[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) dqa[u] = 0.0f;
    if (active) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (fast) backward_block<RND, DQ, false>(tx[c], tg[c], qT, 1 + c, r, dqa);
            else backward_block<RND, DQ, true>(tx[c], tg[c], qT, 1 + c, r, dqa);
        }
    }
    if constexpr (DQ) store_dq_partial(dq_partial + ((long)blockIdx.x * WAVES_PER_BLOCK + wave) * 64, dqa, lane, r);
    transpose_tiles<2>(tile, b, r, tg);
    if (active) {
#pragma clang fp contract(fast)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float o8[8];
            dct_inv8(tg[c], o8);
#pragma unroll
            for (int j = 0; j < 8; ++j) o8[j] *= (VS == 2 ? 0.25f : 0.5f);         // adjoint of the mean
            float4* dst = reinterpret_cast<float4*>(gplanes + (((long)t.n * 2 + c) * g.hc + t.by * 8 + r) * g.wc + t.x0 + b * 8);
            dst[0] = make_float4(o8[0], o8[1], o8[2], o8[3]);
            dst[1] = make_float4(o8[4], o8[5], o8[6], o8[7]);
        }
    }
}

template <int RND, bool DQ, int VS>
__global__ __launch_bounds__(256) void djs_bwd_luma_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                           const uint8_t* __restrict__ mask, const float* __restrict__ qtab,
                                                           const float* __restrict__ gplanes, float* __restrict__ gx,
                                                           float* __restrict__ dq_partial, int n, int h, int w) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = lane >> 3, r = lane & 7;
    float* lds = smem + wave * LWAVE_F;
    float* qT = smem + WAVES_PER_BLOCK * LWAVE_F;
    const Geo g = make_geo(h, w, VS);
    const long n_tasks = (long)n * g.hb * g.strips;
    const Task t = decode_task((long)blockIdx.x * WAVES_PER_BLOCK + wave, n_tasks, g.hb, g.strips);
    const bool active = t.valid && (t.x0 + b * 8 < w);
    f32x4 pre[6] = {};
    fetch_strip(x, pre, t, h, w, lane);
    const bool fast = stage_tables(qtab, qT, reinterpret_cast<int*>(qT + 384)) && !DQ;

    float px[24];
    float tx[1][8], tg[1][8];
    commit_strip(lds, pre, lane);
    fetch_strip(gy, pre, t, h, w, lane);
    uint2 mm = make_uint2(0u, 0u);
    float4 gcb = make_float4(0.f, 0.f, 0.f, 0.f), gcr = gcb;      // reduced chroma gradients under this lane's 8 pixels
    if (active) {
        mm = *reinterpret_cast<const uint2*>(mask + ((long)t.n * h + t.by * 8 + r) * w + t.x0 + b * 8);
        const long o = ((long)t.n * 2 * g.hc + (t.by * 8 + r) / VS) * g.wc + (t.x0 + b * 8) / 2;
        gcb = *reinterpret_cast<const float4*>(gplanes + o);
        gcr = *reinterpret_cast<const float4*>(gplanes + o + (long)g.hc * g.wc);
    }
    wave_sync();
    read_row24(lds, b, r, px);
    wave_sync();
    {
        float ycc[3][8];
        colour_fwd(px, ycc);
        dct_fwd8(ycc[0], tx[0]);
    }
    commit_strip(lds, pre, lane);
    wave_sync();
    read_row24(lds, b, r, px);
    wave_sync();
    {
#pragma clang fp contract(fast)
        float gq[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t m = ((j < 4 ? mm.x >> (8 * j) : mm.y >> (8 * (j - 4)))) & 0xffu;
            float gm[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) gm[c] = (m >> c) & 1u ? px[3 * j + c] * (1.0f / 255.0f) : 0.0f;
            gq[j] = gm[0] * kCI[0][1] + gm[1] * kCI[1][1] + gm[2] * kCI[2][1];
        }
        dct_fwd8(gq, tg[0]);
    }
    transpose_tiles<1>(lds, b, r, tx);
    transpose_tiles<1>(lds, b, r, tg);
    float dqa[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) dqa[u] = 0.0f;
    if (active) {
        if (fast) backward_block<RND, DQ, false>(tx[0], tg[0], qT, 0, r, dqa);
        else backward_block<RND, DQ, true>(tx[0], tg[0], qT, 0, r, dqa);
    }
    if constexpr (DQ) store_dq_partial(dq_partial + ((long)blockIdx.x * WAVES_PER_BLOCK + wave) * 64, dqa, lane, r);
    transpose_tiles<1>(lds, b, r, tg);
    {
#pragma clang fp contract(fast)
        float gb[8];
        dct_inv8(tg[0], gb);
        const float cb4[4] = {gcb.x, gcb.y, gcb.z, gcb.w}, cr4[4] = {gcr.x, gcr.y, gcr.z, gcr.w};
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c)       // d/d(x_c) = 255 * sum_c' gycc_c' * CF[c'][1+c]
                px[3 * j + c] =
                    255.0f * (gb[j] * kCF[0][1 + c] + cb4[j >> 1] * kCF[1][1 + c] + cr4[j >> 1] * kCF[2][1 + c]);
        write_row24(lds, b, r, px);
    }
    wave_sync();
    store_strip(gx, lds, t, h, w, lane);
}

inline int grid_of(long tasks) { return (int)((tasks + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK); }   // one task per wave

struct Plan {
    Geo g;
    long ltasks, ctasks;
    int lgrid, cgrid;
    size_t plane_floats;       // both reduced planes of the batch
};
inline Plan make_plan(int n, int h, int w, int vs) {
    Plan p;
    p.g = make_geo(h, w, vs);
    p.ltasks = (long)n * p.g.hb * p.g.strips;
    p.ctasks = (long)n * p.g.hcb * p.g.cstrips;
    p.lgrid = grid_of(p.ltasks);
    p.cgrid = grid_of(p.ctasks);
    p.plane_floats = (size_t)2 * n * p.g.hc * p.g.wc;
    return p;
}
inline bool bad_shape(int n, int h, int w, int hs, int vs) {
    return n < 0 || h <= 0 || w <= 0 || hs != 2 || (vs != 1 && vs != 2) || (h % (8 * vs)) || (w % (8 * hs));
}

template <int VS>
void launch_fwd(int rounding, const Plan& p, hipStream_t s, const float* x, float* y, const float* qtab, float* planes,
                uint8_t* mask, int16_t* idx, float* xdq, int n, int h, int w) {
    const dim3 cg(p.cgrid), lg(p.lgrid), b(256);
#define NIMG_DJS_FWD(Q)                                                                                                  \
    hipLaunchKernelGGL((djs_fwd_chroma_kernel<Q, VS>), cg, b, kLdsChroma, s, x, qtab, planes, idx, xdq, n, h, w);        \
    hipLaunchKernelGGL((djs_fwd_luma_kernel<Q, VS>), lg, b, kLdsLuma, s, x, y, qtab, (const float*)planes, mask, idx, xdq, n, h, w)
    switch (fwd_mode(rounding)) {
        case Q_RINT: NIMG_DJS_FWD(Q_RINT); break;
        case Q_SIN: NIMG_DJS_FWD(Q_SIN); break;
        case Q_HARMONIC: NIMG_DJS_FWD(Q_HARMONIC); break;
        default: NIMG_DJS_FWD(Q_IDENTITY); break;
    }
#undef NIMG_DJS_FWD
}

template <int VS, bool DQ>
void launch_bwd(int rounding, const Plan& p, hipStream_t s, const float* x, const float* gy, const uint8_t* mask,
                const float* qtab, float* gplanes, float* gx, float* part_l, float* part_c, int n, int h, int w) {
    const dim3 cg(p.cgrid), lg(p.lgrid), b(256);
#define NIMG_DJS_BWD(R)                                                                                                  \
    hipLaunchKernelGGL((djs_bwd_chroma_kernel<R, DQ, VS>), cg, b, kLdsChroma, s, x, gy, mask, qtab, gplanes, part_c, n, h, w); \
    hipLaunchKernelGGL((djs_bwd_luma_kernel<R, DQ, VS>), lg, b, kLdsLuma, s, x, gy, mask, qtab, (const float*)gplanes, gx,   \
                       part_l, n, h, w)
    switch (rounding) {
        case NIMG_ROUND_ROUND: NIMG_DJS_BWD(NIMG_ROUND_ROUND); break;
        case NIMG_ROUND_SIN:                               // without the table gradient SIN and SOFT are one kernel
            if constexpr (DQ) { NIMG_DJS_BWD(NIMG_ROUND_SIN); break; }
            [[fallthrough]];
        case NIMG_ROUND_SOFT: NIMG_DJS_BWD(NIMG_ROUND_SOFT); break;
        case NIMG_ROUND_HARMONIC: NIMG_DJS_BWD(NIMG_ROUND_HARMONIC); break;
        default: NIMG_DJS_BWD(NIMG_ROUND_IDENTITY); break;
    }
#undef NIMG_DJS_BWD
}

}  // namespace

extern "C" {

size_t nimg_djpeg_sub_workspace_bytes(int n, int h, int w, int hs, int vs, int with_dq) {
    if (n <= 0 || bad_shape(n, h, w, hs, vs)) return 0;
    const Plan p = make_plan(n, h, w, vs);
    size_t f = p.plane_floats;
    if (with_dq) f += ((size_t)p.lgrid + p.cgrid) * WAVES_PER_BLOCK * 64;
    return f * sizeof(float);
}

int nimg_djpeg_sub_fwd(const float* x, float* y, const float* qtab, uint8_t* mask, int16_t* idx, float* xdq, int n, int h,
                       int w, int hs, int vs, int rounding, void* workspace, size_t workspace_bytes, void* stream) {
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    if (bad_shape(n, h, w, hs, vs)) return NIMG_ERR_ARG;
    if (rounding < NIMG_ROUND_ROUND || rounding > NIMG_ROUND_IDENTITY) return NIMG_ERR_ARG;
    if (!x || !y || !qtab || !workspace) return NIMG_ERR_ARG;
    if (workspace_bytes < nimg_djpeg_sub_workspace_bytes(n, h, w, hs, vs, 0)) return NIMG_ERR_WORKSPACE;
    const Plan p = make_plan(n, h, w, vs);
    if (vs == 2) launch_fwd<2>(rounding, p, (hipStream_t)stream, x, y, qtab, (float*)workspace, mask, idx, xdq, n, h, w);
    else launch_fwd<1>(rounding, p, (hipStream_t)stream, x, y, qtab, (float*)workspace, mask, idx, xdq, n, h, w);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_djpeg_sub_bwd(const float* x, const float* gy, const uint8_t* mask, const float* qtab, float* gx, float* dq, int n,
                       int h, int w, int hs, int vs, int rounding, int accumulate, void* workspace, size_t workspace_bytes,
                       void* stream) {
    if (n == 0) return NIMG_OK;
    if (bad_shape(n, h, w, hs, vs)) return NIMG_ERR_ARG;
    if (rounding < NIMG_ROUND_ROUND || rounding > NIMG_ROUND_IDENTITY) return NIMG_ERR_ARG;
    if (!x || !gy || !mask || !qtab || !gx || !workspace) return NIMG_ERR_ARG;
    if (workspace_bytes < nimg_djpeg_sub_workspace_bytes(n, h, w, hs, vs, dq != nullptr)) return NIMG_ERR_WORKSPACE;
    const Plan p = make_plan(n, h, w, vs);
    hipStream_t s = (hipStream_t)stream;
    float* gplanes = (float*)workspace;
    float* part_l = gplanes + p.plane_floats;
    float* part_c = part_l + (size_t)p.lgrid * WAVES_PER_BLOCK * 64;
    if (!dq) {
        if (vs == 2) launch_bwd<2, false>(rounding, p, s, x, gy, mask, qtab, gplanes, gx, nullptr, nullptr, n, h, w);
        else launch_bwd<1, false>(rounding, p, s, x, gy, mask, qtab, gplanes, gx, nullptr, nullptr, n, h, w);
        NIMG_CHECK_LAUNCH();
        return NIMG_OK;
    }
    if (vs == 2) launch_bwd<2, true>(rounding, p, s, x, gy, mask, qtab, gplanes, gx, part_l, part_c, n, h, w);
    else launch_bwd<1, true>(rounding, p, s, x, gy, mask, qtab, gplanes, gx, part_l, part_c, n, h, w);
    NIMG_CHECK_LAUNCH();
    // one launch, two fixed-order reductions: luma partials -> dq[0 .. 63], chroma partials -> dq[64 .. 127]
    nimg::launch_reduce2(part_l, dq, 64, p.lgrid * WAVES_PER_BLOCK, part_c, dq + 64, 64, p.cgrid * WAVES_PER_BLOCK, accumulate, s);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

}  // extern "C"
