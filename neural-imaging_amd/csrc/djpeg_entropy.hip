// Rate term of the differentiable JPEG for gfx950 (CDNA4): the soft entropy of the quantised DCT coefficients.
//
//   z = X / Q      the float32 value djpeg_fwd_kernel forms (same canonical fmaf order, same div_q choice: its idx output is the
//                  bit-exact witness of z under the rounding modes that round)
//   e = quantise<mode>(z)
//   H = entropy(e.ravel(), codebook)   helpers/tf_helpers.py:290-333 with the code book of Quantization(latent_bpf=9),
//                  models/jpeg.py:89: the 512 integers -255 .. 256, t-Student kernel v = 50, gamma = 25, eps = 1e-72; ONE pooled
//                  histogram over the N = 3 n h w values; weights, histogram, clip, re-normalisation and / 0.6931 in float64.
//
// The (N, 512) weight matrix never exists.  A wave recomputes the forward transform of its 8 x 64 pixel strip from x (as
// djpeg_bwd_kernel does), parks the 24 values of every lane in its private LDS rows and walks them in a rolled loop: for
// e inside [-255.5, 256.5] only the five centres around rint(e) are evaluated (latent.hip, above t_weight: a centre 2.5 or more
// away weighs < 2e-33 of the nearest), outside it all 512 - those by the whole wave, 8 centres per lane.  The workgroup's
// histogram is 512 float64 bins in LDS; the window around the ZERO centre - about nine coefficients in ten - is summed in
// registers and folded by one wave reduction per wave, LDS float64 atomics serve the other bins.  Partials -> 32 segment sums ->
// histogram, entropy and g_k = dH / d mean_k in a fixed order.
//
// Compiled with -ffp-contract=off like djpeg.hip (csrc/Makefile NOCONTRACT): z has to be that kernel's z.
#include "djpeg.h"

namespace {

using namespace nimg;
using namespace nimg::dj;

constexpr int TILE_F = 3 * 8 * 72;        // transpose tiles: [ch][block][8][9]
constexpr int WAVE_LDS_F = (STAGE_F > TILE_F ? STAGE_F : TILE_F);
constexpr int WAVES_PER_BLOCK = 4;
constexpr int TABLE_F = 392;              // 384 table floats + the flag word, padded to 8 bytes for the float64 array behind them
constexpr int KC = 512;                   // centres -255 .. 256 (9 bits per feature)
constexpr int K_ZERO = 255;               // index of the centre 0
constexpr double kC0 = -255.0;
constexpr float kLo = -255.5f, kHi = 256.5f;
constexpr double kGamma = 25.0, kInvV = 1.0 / 50.0, kEps = 1e-72;
constexpr int kM = 51;                    // v + 1
constexpr double kDfac = -(double)kM * kInvV * kGamma;       // d w / d u = w * kDfac * t * r^2
constexpr int MAX_GRID = 1024;            // workgroups (4 per CU): a wave takes tasks wave, wave + 4 grid, ...
constexpr int SEGS = 32;                  // segment sums of the partial histograms
constexpr size_t kLds = ((size_t)WAVES_PER_BLOCK * WAVE_LDS_F + TABLE_F) * sizeof(float) + KC * sizeof(double);

// workspace: [g_k 512 f64 | SEGS x 512 f64 segment sums | grid x 512 f64 partial histograms, later grid x 4 x 128 f32 dq partials]
constexpr size_t kOffSeg = KC * sizeof(double);
constexpr size_t kOffPart = kOffSeg + (size_t)SEGS * KC * sizeof(double);

inline long task_count(int n, int h, int w) { return (long)n * (h / 8) * ((w + STRIP_PX - 1) / STRIP_PX); }
inline int grid_of(long tasks) {
    const long g = (tasks + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    return (int)(g > MAX_GRID ? MAX_GRID : g);
}

// copies of latent.hip's rsqrt_refined / pow_fixed<51>: base^-(51/2) with no division, square root or pow()
__device__ __forceinline__ double rsqrt_refined(double x) {
    double r = (double)__builtin_amdgcn_rsqf((float)x);
    r = r * __builtin_fma(-0.5 * x, r * r, 1.5);
    r = r * __builtin_fma(-0.5 * x, r * r, 1.5);
    return r;
}
__device__ __forceinline__ double pow_m(double r) {
    double acc = (kM & 1) ? r : 1.0, b = r;
#pragma unroll
    for (int n = kM >> 1; n > 0; n >>= 1) {
        b *= b;
        if (n & 1) acc *= b;
    }
    return acc;
}
__device__ __forceinline__ double weight0(double u, int k, double& r, double& t) {
    t = kGamma * (u - (kC0 + (double)k));
    r = rsqrt_refined(__builtin_fma(t * t, kInvV, 1.0));
    return pow_m(r);
}
__device__ __forceinline__ bool in_window_range(float e) { return e >= kLo && e <= kHi; }
__device__ __forceinline__ int nearest_centre(float e) {
    const int k0 = (int)rintf(e) + K_ZERO;
    return k0 < 0 ? 0 : (k0 > KC - 1 ? KC - 1 : k0);
}

// the histogram terms wn_k(e) of one value INSIDE the window range: registers for the window of the zero centre, LDS atomics for
// the other bins
__device__ __forceinline__ void hist_add_window(float e, double* sh, double (&acc0)[5]) {
    const double u = (double)e;
    double r, t;
    const int k0 = nearest_centre(e);
    double wgt[5], S = 0.0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int k = k0 + j - 2;
        wgt[j] = (unsigned)k < (unsigned)KC ? weight0(u, k, r, t) + kEps : 0.0;
        S += wgt[j];
    }
    const double inv = 1.0 / S;
    if (k0 == K_ZERO) {
#pragma unroll
        for (int j = 0; j < 5; ++j) acc0[j] = __builtin_fma(wgt[j], inv, acc0[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int k = k0 + j - 2;
            if ((unsigned)k < (unsigned)KC) atomicAdd(&sh[k], wgt[j] * inv);
        }
    }
}

// A value OUTSIDE the range sees all 512 centres.  One lane walking them alone keeps the other 63 waiting for 1024 weights (and 512
// atomics): the WAVE takes such a value together - lane l the centres l, l + 64, ..., a butterfly sum for the normaliser - in 8
// weights per lane.  `e` is wave-uniform; every lane of the wave calls this.
constexpr int CPL = KC / 64;              // centres per lane
__device__ __forceinline__ void hist_add_full_wave(float e, int lane, double* sh) {
    const double u = (double)e;
    double wgt[CPL], S = 0.0, r, t;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        wgt[j] = weight0(u, lane + 64 * j, r, t) + kEps;
        S += wgt[j];
    }
    const double inv = 1.0 / wave_sum_d(S);
#pragma unroll
    for (int j = 0; j < CPL; ++j) atomicAdd(&sh[lane + 64 * j], wgt[j] * inv);
}

// sum_k g_k d wn_k / d e = (A - B dS / S) / S with S = sum w, dS = sum dw, A = sum g dw, B = sum g w over the same centres
struct DdeSums {
    double S = 0.0, dS = 0.0, A = 0.0, B = 0.0;
    __device__ __forceinline__ void centre(double u, int k, const double* sg) {
        double r, t;
        const double w0 = weight0(u, k, r, t);
        const double dw = w0 * (kDfac * t) * (r * r);
        const double wk = w0 + kEps, gk = sg[k];
        S += wk; dS += dw;
        A = __builtin_fma(gk, dw, A);
        B = __builtin_fma(gk, wk, B);
    }
    __device__ __forceinline__ double value() const {
        const double inv = 1.0 / S;
        return (A - B * dS * inv) * inv;
    }
};
__device__ __forceinline__ double entropy_dde_window(float e, const double* sg) {      // e inside the window range
    const double u = (double)e;
    DdeSums a;
    const int k0 = nearest_centre(e);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int k = k0 + j - 2;
        if ((unsigned)k < (unsigned)KC) a.centre(u, k, sg);
    }
    return a.value();
}
// e outside the range, wave-uniform, every lane calls: 8 centres per lane, four butterfly sums; the same value in every lane
__device__ __forceinline__ double entropy_dde_full_wave(float e, int lane, const double* sg) {
    const double u = (double)e;
    DdeSums a;
#pragma unroll
    for (int j = 0; j < CPL; ++j) a.centre(u, lane + 64 * j, sg);
    a.S = wave_sum_d(a.S); a.dS = wave_sum_d(a.dS); a.A = wave_sum_d(a.A); a.B = wave_sum_d(a.B);
    return a.value();
}

// x strip -> T columns in v (lane (b, r): column r of its block, three channels): fetch, colour, row pass, transpose
__device__ __forceinline__ void strip_row_pass(const float* __restrict__ x, float* lds, const Task& t, int h, int w, int lane,
                                               int b, int r, float (&v)[3][8]) {
    f32x4 pre[6] = {};
    fetch_strip(x, pre, t, h, w, lane);
    commit_strip(lds, pre, lane);
    wave_sync();
    float px[24];
    read_row24(lds, b, r, px);
    wave_sync();
    float ycc[3][8];
    colour_fwd(px, ycc);
#pragma unroll
    for (int c = 0; c < 3; ++c) dct_fwd8(ycc[c], v[c]);
    transpose_tiles<3>(lds, b, r, v);
}

// column pass and z = X / Q of the lane's 24 values
template <bool EXACT>
__device__ __forceinline__ void columns_z(const float (&v)[3][8], const float* qT, int r, float (&z)[3][8]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float X[8], q[8], rc[8];
        dct_fwd8(v[c], X);
        read_tables(qT, c, r, q, rc);
#pragma unroll
        for (int u = 0; u < 8; ++u) z[c][u] = div_q<EXACT>(X[u], q[u], rc[u]);
    }
}

template <int QMODE>
__global__ __launch_bounds__(256) void djpeg_entropy_fwd_kernel(const float* __restrict__ x, const float* __restrict__ qtab,
                                                                 double* __restrict__ hist_partial, int n, int h, int w) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = lane >> 3, r = lane & 7;
    float* lds = smem + wave * WAVE_LDS_F;
    float* qT = smem + WAVES_PER_BLOCK * WAVE_LDS_F;
    double* sh = reinterpret_cast<double*>(smem + WAVES_PER_BLOCK * WAVE_LDS_F + TABLE_F);
    for (int k = threadIdx.x; k < KC; k += 256) sh[k] = 0.0;
    const bool fast = stage_tables(qtab, qT, reinterpret_cast<int*>(qT + 384));       // its barriers cover sh
    const int hb = h / 8, strips = (w + STRIP_PX - 1) / STRIP_PX;
    const long n_tasks = (long)n * hb * strips;
    double acc0[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long task = (long)blockIdx.x * WAVES_PER_BLOCK + wave; task < n_tasks; task += (long)gridDim.x * WAVES_PER_BLOCK) {
        const Task t = decode_task(task, n_tasks, hb, strips);
        const bool active = t.x0 + b * 8 < w;
        float v[3][8];
        strip_row_pass(x, lds, t, h, w, lane, b, r, v);
        if (active) {
            float z[3][8];
            if (fast) columns_z<false>(v, qT, r, z);
            else columns_z<true>(v, qT, r, z);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int u = 0; u < 8; ++u) lds[(c * 8 + u) * 64 + lane] = quantise<QMODE>(z[c][u]);
        }
        wave_sync();
#pragma unroll 1
        for (int i = 0; i < 24; ++i) {                       // every lane of the wave: the full loop is a wave's work
            const float e = active ? lds[i * 64 + lane] : 0.0f;
            const bool inside = in_window_range(e);
            if (active && inside) hist_add_window(e, sh, acc0);
            for (unsigned long long m = __ballot(active && !inside); m; m &= m - 1)
                hist_add_full_wave(__shfl(e, __ffsll((long long)m) - 1, 64), lane, sh);
        }
        wave_sync();
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const double s = wave_sum_d(acc0[j]);
        if (lane == 0) atomicAdd(&sh[K_ZERO - 2 + j], s);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < KC; k += 256) hist_partial[(long)blockIdx.x * KC + k] = sh[k];
}

// seg[s][k] = partial[s][k] + partial[s + SEGS][k] + ... : fixed order
__global__ __launch_bounds__(KC) void hist512_reduce_kernel(const double* __restrict__ partial, int nblocks,
                                                            double* __restrict__ seg) {
    const int k = threadIdx.x, s = blockIdx.x;
    double a = 0.0;
    for (int p = s; p < nblocks; p += SEGS) a += partial[(long)p * KC + k];
    seg[s * KC + k] = a;
}

__device__ __forceinline__ double block_sum512(double v, double* red) {      // 8 waves, summed in wave order
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) s += red[i];
    return s;
}

// histogram = segment sums in order / N; clip at 1e-9, re-normalise, H / 0.6931 (tf_helpers.py:326-331); g_k = dH / d mean_k
// through the re-normalisation, zero where the clip is active
__global__ __launch_bounds__(KC) void entropy512_finalize_kernel(const double* __restrict__ seg, double n_total,
                                                                 float* __restrict__ entropy, double* __restrict__ g) {
    __shared__ double red[8];
    const int k = threadIdx.x;
    double hs = 0.0;
    for (int s = 0; s < SEGS; ++s) hs += seg[s * KC + k];
    const double hm = hs / n_total;
    const bool clipped = hm < 1e-9;
    const double hc = clipped ? 1e-9 : hm;
    const double T = block_sum512(hc, red);
    const double q = hc / T, lq = log(q);
    const double H = -block_sum512(q * lq, red);
    const double mean = block_sum512(q * (lq + 1.0), red);
    if (k == 0) entropy[0] = (float)(H / 0.6931);
    g[k] = clipped ? 0.0 : (-(lq + 1.0) + mean) / T / 0.6931;
}

__device__ __forceinline__ void store_strip_add(float* __restrict__ dst, const float* lds, const Task& t, int h, int w, int lane,
                                                bool add) {
    const int strip_f = min(STRIP_PX, w - t.x0) * 3;
#pragma unroll
    for (int it = 0; it < 6; ++it) {
        const int idx = it * 64 + lane;
        const int row = idx / 48, c4 = idx % 48;
        if (c4 * 4 < strip_f) {
            float4 v = *reinterpret_cast<const float4*>(lds + row * ROW_STRIDE + c4 * 4);
            float4* d = reinterpret_cast<float4*>(dst + (((long)t.n * h + t.by * 8 + row) * w + t.x0) * 3 + c4 * 4);
            if (add) { const float4 o = *d; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
            *d = v;
        }
    }
}

// gx (+)= scale * sum_k g_k d wn_k / d e * quantise'(z) / Q back through the column / row DCT, the colour matrix and the 255;
// DQ: the same value times -z into the table gradient partials (dq_partial[wave of the grid][cls][u][r], the layout of
// djpeg_bwd_kernel's; a wave sums its tasks first).  DQ always takes the IEEE division (trained tables are not integers).
template <int RND, bool DQ>
__global__ __launch_bounds__(256) void djpeg_entropy_bwd_kernel(const float* __restrict__ x, const float* __restrict__ qtab,
                                                                 const double* __restrict__ g, double scale,
                                                                 float* __restrict__ gx, int accumulate_gx,
                                                                 float* __restrict__ dq_partial, int n, int h, int w) {
    constexpr int GMODE = bwd_mode(RND), QMODE = fwd_mode(RND);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = lane >> 3, r = lane & 7;
    float* lds = smem + wave * WAVE_LDS_F;
    float* qT = smem + WAVES_PER_BLOCK * WAVE_LDS_F;
    double* sg = reinterpret_cast<double*>(smem + WAVES_PER_BLOCK * WAVE_LDS_F + TABLE_F);
    for (int k = threadIdx.x; k < KC; k += 256) sg[k] = g[k];
    const bool fast = stage_tables(qtab, qT, reinterpret_cast<int*>(qT + 384)) && !DQ;
    const int hb = h / 8, strips = (w + STRIP_PX - 1) / STRIP_PX;
    const long n_tasks = (long)n * hb * strips;
    float dqa[DQ ? 2 : 1][8];
#pragma unroll
    for (int k = 0; k < (DQ ? 2 : 1); ++k)
#pragma unroll
        for (int u = 0; u < 8; ++u) dqa[k][u] = 0.0f;
    for (long task = (long)blockIdx.x * WAVES_PER_BLOCK + wave; task < n_tasks; task += (long)gridDim.x * WAVES_PER_BLOCK) {
        const Task t = decode_task(task, n_tasks, hb, strips);
        const bool active = t.x0 + b * 8 < w;
        float v[3][8], z[3][8];
        strip_row_pass(x, lds, t, h, w, lane, b, r, v);
        if (active) {
            if (fast) columns_z<false>(v, qT, r, z);
            else columns_z<true>(v, qT, r, z);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int u = 0; u < 8; ++u) lds[(c * 8 + u) * 64 + lane] = z[c][u];
        }
        wave_sync();
#pragma unroll 1
        for (int i = 0; i < 24; ++i) {                       // every lane of the wave: the full loop is a wave's work
            const float e = active ? quantise<QMODE>(lds[i * 64 + lane]) : 0.0f;
            const bool inside = in_window_range(e);
            double d = 0.0;
            if (active && inside) d = entropy_dde_window(e, sg);
            for (unsigned long long m = __ballot(active && !inside); m; m &= m - 1) {
                const int src = __ffsll((long long)m) - 1;
                const double full = entropy_dde_full_wave(__shfl(e, src, 64), lane, sg);
                if (lane == src) d = full;
            }
            if (active) lds[i * 64 + lane] = (float)(scale * d);                   // d (coef H) / d e
        }
        wave_sync();
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float G[8];
            if (active) {
                float q[8], rc[8];
                read_tables(qT, c, r, q, rc);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float gz = lds[(c * 8 + u) * 64 + lane] * quantise_grad<GMODE>(z[c][u]);
                    G[u] = gz / q[u];                                        // d z / d X = 1 / Q
                    if constexpr (DQ) dqa[c == 0 ? 0 : 1][u] -= G[u] * z[c][u];   // d z / d Q = -z / Q
                }
            } else {
#pragma unroll
                for (int u = 0; u < 8; ++u) G[u] = 0.0f;
            }
            dct_inv8(G, v[c]);                                               // d b = F^T gX F : column pass
        }
        wave_sync();
        transpose_tiles<3>(lds, b, r, v);
        {
            float gb[3][8], px[24];
#pragma unroll
            for (int c = 0; c < 3; ++c) dct_inv8(v[c], gb[c]);               // row pass
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c)       // d/d(x_c) = 255 * sum_c' gycc_c' * CF[c'][1+c]
                    px[3 * j + c] =
                        255.0f * (gb[0][j] * kCF[0][1 + c] + gb[1][j] * kCF[1][1 + c] + gb[2][j] * kCF[2][1 + c]);
            write_row24(lds, b, r, px);
        }
        wave_sync();
        store_strip_add(gx, lds, t, h, w, lane, accumulate_gx != 0);
        wave_sync();
    }
    if constexpr (DQ) {
        const long slot = (long)blockIdx.x * WAVES_PER_BLOCK + wave;
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                float s = dqa[k][u];
                s += __shfl_xor(s, 8, 64);
                s += __shfl_xor(s, 16, 64);
                s += __shfl_xor(s, 32, 64);
                if (lane < 8) dq_partial[slot * 128 + (k * 8 + u) * 8 + r] = s;
            }
    }
}

template <bool DQ, typename... A>
void launch_bwd(int rounding, int grid, hipStream_t s, A... a) {
    const dim3 g(grid), b(256);
    switch (rounding) {
        case NIMG_ROUND_ROUND: hipLaunchKernelGGL((djpeg_entropy_bwd_kernel<NIMG_ROUND_ROUND, DQ>), g, b, kLds, s, a...); break;
        case NIMG_ROUND_SOFT: hipLaunchKernelGGL((djpeg_entropy_bwd_kernel<NIMG_ROUND_SOFT, DQ>), g, b, kLds, s, a...); break;
        case NIMG_ROUND_SIN: hipLaunchKernelGGL((djpeg_entropy_bwd_kernel<NIMG_ROUND_SIN, DQ>), g, b, kLds, s, a...); break;
        case NIMG_ROUND_HARMONIC: hipLaunchKernelGGL((djpeg_entropy_bwd_kernel<NIMG_ROUND_HARMONIC, DQ>), g, b, kLds, s, a...); break;
        default: hipLaunchKernelGGL((djpeg_entropy_bwd_kernel<NIMG_ROUND_IDENTITY, DQ>), g, b, kLds, s, a...); break;
    }
}

inline bool bad_shape(int n, int h, int w) { return n < 0 || h <= 0 || w <= 0 || (h % 8) || (w % 8); }

}  // namespace

extern "C" {

size_t nimg_djpeg_entropy_workspace_bytes(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return kOffPart + (size_t)grid_of(task_count(n, h, w)) * KC * sizeof(double);
}

int nimg_djpeg_entropy_fwd(const float* x, const float* qtab, int n, int h, int w, int rounding, float* entropy,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (n == 0) return NIMG_OK;
    if (!x || !qtab || !entropy || !workspace || bad_shape(n, h, w)) return NIMG_ERR_ARG;
    if (rounding < NIMG_ROUND_ROUND || rounding > NIMG_ROUND_IDENTITY) return NIMG_ERR_ARG;
    if (workspace_bytes < nimg_djpeg_entropy_workspace_bytes(n, h, w)) return NIMG_ERR_WORKSPACE;
    const int grid = grid_of(task_count(n, h, w));
    hipStream_t s = (hipStream_t)stream;
    double* g = (double*)workspace;
    double* seg = (double*)((char*)workspace + kOffSeg);
    double* part = (double*)((char*)workspace + kOffPart);
    const dim3 gr(grid), bl(256);
    switch (fwd_mode(rounding)) {
        case Q_RINT: hipLaunchKernelGGL(djpeg_entropy_fwd_kernel<Q_RINT>, gr, bl, kLds, s, x, qtab, part, n, h, w); break;
        case Q_SIN: hipLaunchKernelGGL(djpeg_entropy_fwd_kernel<Q_SIN>, gr, bl, kLds, s, x, qtab, part, n, h, w); break;
        case Q_HARMONIC: hipLaunchKernelGGL(djpeg_entropy_fwd_kernel<Q_HARMONIC>, gr, bl, kLds, s, x, qtab, part, n, h, w); break;
        default: hipLaunchKernelGGL(djpeg_entropy_fwd_kernel<Q_IDENTITY>, gr, bl, kLds, s, x, qtab, part, n, h, w); break;
    }
    NIMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(hist512_reduce_kernel, dim3(SEGS), dim3(KC), 0, s, (const double*)part, grid, seg);
    NIMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(entropy512_finalize_kernel, dim3(1), dim3(KC), 0, s, (const double*)seg, 3.0 * (double)n * h * w, entropy,
                       g);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_djpeg_entropy_bwd(const float* x, const float* qtab, int n, int h, int w, int rounding, float coef, float* gx,
                           int accumulate_gx, float* dq, int accumulate_dq, void* workspace, size_t workspace_bytes,
                           void* stream) {
    if (n == 0) return NIMG_OK;
    if (!x || !qtab || !gx || !workspace || bad_shape(n, h, w)) return NIMG_ERR_ARG;
    if (rounding < NIMG_ROUND_ROUND || rounding > NIMG_ROUND_IDENTITY) return NIMG_ERR_ARG;
    if (workspace_bytes < nimg_djpeg_entropy_workspace_bytes(n, h, w)) return NIMG_ERR_WORKSPACE;
    const int grid = grid_of(task_count(n, h, w));
    hipStream_t s = (hipStream_t)stream;
    const double* g = (const double*)workspace;
    float* part = (float*)((char*)workspace + kOffPart);
    const double scale = (double)coef / (3.0 * (double)n * h * w);
    if (dq) launch_bwd<true>(rounding, grid, s, x, qtab, g, scale, gx, accumulate_gx, part, n, h, w);
    else launch_bwd<false>(rounding, grid, s, x, qtab, g, scale, gx, accumulate_gx, (float*)nullptr, n, h, w);
    NIMG_CHECK_LAUNCH();
    if (dq) {
        nimg::launch_reduce2(part, dq, 128, grid * WAVES_PER_BLOCK, nullptr, nullptr, 0, 0, accumulate_dq, s);
        NIMG_CHECK_LAUNCH();
    }
    return NIMG_OK;
}

}  // extern "C"
