// The L1 and SSIM training losses of the imaging pipelines (reference helpers/tf_helpers.py:35-40, selected by
// NIPModel.construct_loss, models/pipelines.py:53-63), each with the gradient w.r.t. the developed image.
//   mae255:    loss = mean |255 y - 255 t|;                        dy (+)= gscale * 255 sign(y - t) / count
//   ssim_loss: loss = mean_n 255 (1 - tf.image.ssim(y, t, max_val)_n)   (11x11 Gaussian window, sigma 1.5, VALID)
// SSIM backward: with the window moments m = (E y, E t, E yy, E tt, E yt) at window position q,
//   S = (2 Ey Et + c1)(2 (Eyt - Ey Et) + c2) / ((Ey^2 + Et^2 + c1)(Eyy - Ey^2 + Ett - Et^2 + c2)),
// and every moment is a Gaussian-weighted sum of the pixels, so
//   d loss / d y(p) = sum_q g(p - q) [ dS/dEy(q) + 2 y(p) dS/dEyy(q) + t(p) dS/dEyt(q) ] * (-255 / items).
// Pass 1 writes the three derivative maps (already scaled) and the per-workgroup sums of S (double, fixed order);
// pass 2 gathers them through the transposed window.  HBM/L2-bound gathers; not on the default (L2) training path.
//
// Behind them the default training loss and the metric, each described at its kernels:
//   mse255:    loss = mean (255 a - 255 b)^2 with its gradient (helpers/tf_helpers.py:31-32), and mse255_sum_s2d3, the same loss
//              fused with the sum of the manipulation gradients and the gradient of depth_to_space + clip
//   ssim:      the per-image SSIM metric, skimage's and tf.image.ssim's (helpers/metrics.py:9-25, models/compression.py:89)
#include <stdlib.h>

#include "common.h"

namespace {
using namespace nimg;

constexpr int WIN = 11;
constexpr int BPI = 64;          // workgroups per image in pass 1

__global__ __launch_bounds__(256) void mae255_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                     float* grad_a, double* __restrict__ partial, long count,
                                                     float gscale, int accumulate) {
    __shared__ double red[4];
    double s = 0.0;
    const float gk = gscale * 255.0f / (float)count;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long)gridDim.x * blockDim.x) {
        const float d = 255.0f * a[i] - 255.0f * b[i];
        s += (double)fabsf(d);
        const float g = d > 0.f ? gk : (d < 0.f ? -gk : 0.f);               // tf.abs gradient: sign(d), sign(0) = 0
        if (grad_a) grad_a[i] = accumulate ? grad_a[i] + g : g;
    }
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ void mean_final_kernel(const double* __restrict__ partial, int nblocks, double inv_count, double scale,
                                  double offset, float* loss) {
    double s = 0.0;
    for (int k = threadIdx.x; k < nblocks; k += 64) s += partial[k];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) loss[0] = (float)(offset + scale * s * inv_count);
}

__global__ __launch_bounds__(256) void ssim_loss_stats_kernel(const float* __restrict__ y, const float* __restrict__ t,
                                                              double* __restrict__ partial, float* __restrict__ maps,
                                                              long plane, int h, int w, int c, float max_val,
                                                              const float* __restrict__ gk, double coef) {
    __shared__ double red[4];
    __shared__ float gs[WIN * WIN];
    if (threadIdx.x < WIN * WIN) gs[threadIdx.x] = gk[threadIdx.x];
    __syncthreads();
    const int n = blockIdx.x / BPI, blk = blockIdx.x % BPI;
    const int ho = h - WIN + 1, wo = w - WIN + 1;
    const long items = (long)ho * wo * c;
    const double c1 = (0.01 * max_val) * (0.01 * max_val), c2 = (0.03 * max_val) * (0.03 * max_val);
    double sum = 0.0;
    for (long i = (long)blk * 256 + threadIdx.x; i < items; i += (long)BPI * 256) {
        const int ch = (int)(i % c), x0 = (int)((i / c) % wo), y0 = (int)(i / ((long)c * wo));
        double ey = 0, et = 0, eyy = 0, ett = 0, eyt = 0;
        for (int dy = 0; dy < WIN; ++dy) {
            const long row = (((long)n * h + y0 + dy) * w + x0) * c + ch;
#pragma unroll
            for (int dx = 0; dx < WIN; ++dx) {
                const double wt = (double)gs[dy * WIN + dx];
                const double vy = y[row + (long)dx * c], vt = t[row + (long)dx * c];
                ey += wt * vy; et += wt * vt; eyy += wt * vy * vy; ett += wt * vt * vt; eyt += wt * vy * vt;
            }
        }
        const double a1 = 2 * ey * et + c1, a2 = 2 * (eyt - ey * et) + c2;
        const double b1 = ey * ey + et * et + c1, b2 = (eyy - ey * ey) + (ett - et * et) + c2;
        const double inv = 1.0 / (b1 * b2), s = a1 * a2 * inv;
        sum += s;
        if (maps) {
            const long o = (long)n * items + i;
            maps[o] = (float)(coef * (2 * et * (a2 - a1) * inv - s * 2 * ey * (b2 - b1) * inv));   // dS / dEy
            maps[plane + o] = (float)(coef * (-s / b2));                                            // dS / dEyy
            maps[2 * plane + o] = (float)(coef * (2 * a1 * inv));                                   // dS / dEyt
        }
    }
    sum = wave_sum_d(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void ssim_loss_grad_kernel(const float* __restrict__ y, const float* __restrict__ t,
                                                             const float* __restrict__ maps, long plane,
                                                             float* grad, int n, int h, int w, int c,
                                                             const float* __restrict__ gk, float gscale,
                                                             int accumulate, const float* __restrict__ coef) {
    __shared__ float gs[WIN * WIN];
    if (threadIdx.x < WIN * WIN) gs[threadIdx.x] = gk[threadIdx.x];
    __syncthreads();
    const int ho = h - WIN + 1, wo = w - WIN + 1;
    const long total = (long)n * h * w * c;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int ch = (int)(i % c), px = (int)((i / c) % w), py = (int)((i / ((long)c * w)) % h);
        const long im = i / ((long)c * w * h);
        float sm = 0.f, sxx = 0.f, sxy = 0.f;
        const int dy0 = max(0, py - ho + 1), dy1 = min(WIN - 1, py);
        const int dx0 = max(0, px - wo + 1), dx1 = min(WIN - 1, px);
        for (int dy = dy0; dy <= dy1; ++dy) {
            const long row = ((im * ho + (py - dy)) * wo) * c + ch;
            for (int dx = dx0; dx <= dx1; ++dx) {
                const float wt = gs[dy * WIN + dx];
                const long o = row + (long)(px - dx) * c;
                sm = fmaf(wt, maps[o], sm);
                sxx = fmaf(wt, maps[plane + o], sxx);
                sxy = fmaf(wt, maps[2 * plane + o], sxy);
            }
        }
        const float cf = coef ? coef[im * c + ch] : 1.0f;          // MS-SSIM: the maps are unscaled, the weight is per (n, c)
        const float g = gscale * cf * (sm + 2.0f * y[i] * sxx + t[i] * sxy);
        grad[i] = accumulate ? grad[i] + g : g;
    }
}

// MS-SSIM building block (tf.image.ssim_multiscale -> _ssim_per_channel): per (image, channel) sums of the SSIM map
// (luminance x contrast-structure) and of the contrast-structure map alone, plus - optionally - the UNSCALED derivative maps of
// one of them w.r.t. the window moments (which = 1: SSIM, 2: cs).  Workgroups (n, ch, blk): every block stays in one plane.
constexpr int BPP = 8;           // workgroups per (image, channel) plane
__global__ __launch_bounds__(256) void ssim_planes_kernel(const float* __restrict__ y, const float* __restrict__ t,
                                                          double* __restrict__ partial, float* __restrict__ maps,
                                                          long plane, int h, int w, int c, float max_val,
                                                          const float* __restrict__ gk, int which) {
    __shared__ double red[8];
    __shared__ float gs[WIN * WIN];
    if (threadIdx.x < WIN * WIN) gs[threadIdx.x] = gk[threadIdx.x];
    __syncthreads();
    const int blk = blockIdx.x % BPP, ch = (blockIdx.x / BPP) % c, n = blockIdx.x / (BPP * c);
    const int ho = h - WIN + 1, wo = w - WIN + 1;
    const int items = ho * wo;
    const double c1 = (0.01 * max_val) * (0.01 * max_val), c2 = (0.03 * max_val) * (0.03 * max_val);
    double s_ssim = 0.0, s_cs = 0.0;
    for (int i = blk * 256 + threadIdx.x; i < items; i += BPP * 256) {
        const int x0 = i % wo, y0 = i / wo;
        double ey = 0, et = 0, eyy = 0, ett = 0, eyt = 0;
        for (int dy = 0; dy < WIN; ++dy) {
            const long row = (((long)n * h + y0 + dy) * w + x0) * c + ch;
#pragma unroll
            for (int dx = 0; dx < WIN; ++dx) {
                const double wt = (double)gs[dy * WIN + dx];
                const double vy = y[row + (long)dx * c], vt = t[row + (long)dx * c];
                ey += wt * vy; et += wt * vt; eyy += wt * vy * vy; ett += wt * vt * vt; eyt += wt * vy * vt;
            }
        }
        const double a1 = 2 * ey * et + c1, a2 = 2 * (eyt - ey * et) + c2;
        const double b1 = ey * ey + et * et + c1, b2 = (eyy - ey * ey) + (ett - et * et) + c2;
        const double cs = a2 / b2, ss = a1 * cs / b1;
        s_ssim += ss;
        s_cs += cs;
        if (maps && which) {
            const long o = (((long)n * ho + y0) * wo + x0) * c + ch;
            if (which == 1) {
                const double inv = 1.0 / (b1 * b2);
                maps[o] = (float)(2 * et * (a2 - a1) * inv - ss * 2 * ey * (b2 - b1) * inv);
                maps[plane + o] = (float)(-ss / b2);
                maps[2 * plane + o] = (float)(2 * a1 * inv);
            } else {
                maps[o] = (float)((-2 * et * b2 + 2 * ey * a2) / (b2 * b2));
                maps[plane + o] = (float)(-a2 / (b2 * b2));
                maps[2 * plane + o] = (float)(2.0 / b2);
            }
        }
    }
    s_ssim = wave_sum_d(s_ssim);
    s_cs = wave_sum_d(s_cs);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = s_ssim; red[4 + (threadIdx.x >> 6)] = s_cs; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = red[0] + red[1] + red[2] + red[3];
        partial[2 * blockIdx.x + 1] = red[4] + red[5] + red[6] + red[7];
    }
}

__global__ void ssim_planes_final_kernel(const double* __restrict__ partial, int planes, double inv_items,
                                         float* __restrict__ mean_ssim, float* __restrict__ mean_cs) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= planes) return;
    double a = 0.0, b = 0.0;
    for (int k = 0; k < BPP; ++k) { a += partial[2 * (p * BPP + k)]; b += partial[2 * (p * BPP + k) + 1]; }
    if (mean_ssim) mean_ssim[p] = (float)(a * inv_items);
    if (mean_cs) mean_cs[p] = (float)(b * inv_items);
}

// ms[n][c] = prod_k relu(v[k][n][c]) ^ w[k];  loss = 255 (1 - mean ms);  coef[k][n][c] = d loss / d v[k][n][c] / items[k]
__global__ __launch_bounds__(64) void msssim_combine_kernel(const float* __restrict__ v, const float* __restrict__ items,
                                                            int scales, int planes, float* __restrict__ loss,
                                                            float* __restrict__ coef) {
    const float wts[5] = {0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f};
    double acc = 0.0;
    for (int p = threadIdx.x; p < planes; p += 64) {
        double ms = 1.0;
        for (int k = 0; k < scales; ++k) ms *= pow((double)fmaxf(v[k * planes + p], 0.f), (double)wts[k]);
        acc += ms;
        if (coef)
            for (int k = 0; k < scales; ++k) {
                const float vk = v[k * planes + p];
                coef[k * planes + p] = vk > 0.f ? (float)(-255.0 / planes * wts[k] * ms / vk / items[k]) : 0.f;
            }
    }
    acc = wave_sum_d(acc);
    if (threadIdx.x == 0) loss[0] = (float)(255.0 * (1.0 - acc / planes));
}

// ---------------------------------------------------------------------------------------------------------------
// mse on 255-scaled images: loss = mean((255a-255b)^2); grad_a (+)= gscale * 2*255^2*(a-b)/count
__global__ __launch_bounds__(256) void mse255_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                     float* grad_a, double* __restrict__ partial, long count,
                                                     float gscale, int accumulate) {
    __shared__ double red[4];
    double s = 0.0;
    const float gk = gscale * 2.0f * 255.0f * 255.0f / (float)count;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long)gridDim.x * blockDim.x) {
        const float d = a[i] - b[i];
        const float e = 255.0f * d;
        s += (double)e * (double)e;
        if (grad_a) grad_a[i] = accumulate ? grad_a[i] + gk * d : gk * d;
    }
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// The head of the UNet's backward pass in the workflow, one pass instead of three (add_n -> mse255 with accumulate ->
// d2s_clip3_bwd): element (n, y, x, ch) of the result's depth_to_space image = parts[0] + parts[1] + ... + gk (a - b), the
// additions in that order with the same single rounding per step as the three kernels (the last one contracted to an fma, as
// mse255_kernel's accumulate form compiles) - written as (n, h, w, 12); the loss partials as mse255_kernel.
struct SumS2dParts { const float* p[6]; };
__global__ __launch_bounds__(256) void mse255_sum_s2d3_kernel(SumS2dParts parts, int n_parts, const float* __restrict__ a,
                                                              const float* __restrict__ b, float* __restrict__ dz,
                                                              double* __restrict__ partial, long npix, int h, int w, float gscale) {
    __shared__ double red[4];
    double s = 0.0;
    const long count = npix * 12;
    const float gk = gscale * 2.0f * 255.0f * 255.0f / (float)count;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long)gridDim.x * blockDim.x) {
        const int xx = (int)(i % w);
        const long r = i / w;
        const int yy = (int)(r % h);
        const long im = r / h;
        const long top = ((im * 2 * h + 2 * yy) * (2L * w) + 2 * xx) * 3, bot = top + 2L * w * 3;
        float v[12];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const long o = half ? bot : top;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                float2 acc = reinterpret_cast<const float2*>(parts.p[0] + o)[q];
#pragma unroll
                for (int k = 1; k < 6; ++k)
                    if (k < n_parts) {
                        const float2 t = reinterpret_cast<const float2*>(parts.p[k] + o)[q];
                        acc.x += t.x; acc.y += t.y;
                    }
                const float2 va = reinterpret_cast<const float2*>(a + o)[q], vb = reinterpret_cast<const float2*>(b + o)[q];
                const float d0 = va.x - vb.x, d1 = va.y - vb.y;
                const float e0 = 255.0f * d0, e1 = 255.0f * d1;
                s += (double)e0 * (double)e0;
                s += (double)e1 * (double)e1;
                v[half * 6 + 2 * q] = fmaf(gk, d0, acc.x);
                v[half * 6 + 2 * q + 1] = fmaf(gk, d1, acc.y);
            }
        }
        float4* dst = reinterpret_cast<float4*>(dz + i * 12);
        dst[0] = make_float4(v[0], v[1], v[2], v[3]);
        dst[1] = make_float4(v[4], v[5], v[6], v[7]);
        dst[2] = make_float4(v[8], v[9], v[10], v[11]);
    }
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// Row form of the kernel above (w even, w <= 512): a workgroup takes one OUTPUT row = two input rows of 6 w floats.  The pixel-pair
// form reads 24-byte runs at 8 bytes per lane - every 64-byte line of the seven input tensors is requested three times by
// neighbouring lanes (counters: 1.04 GB fetched per launch for 0.4 GB of operands, 150 us at B = 64); here the two rows are read
// as linear 16-byte items, summed in the same order (parts[0] + parts[1] + ..., then the fma with gk (a - b)), turned around
// through LDS and written as linear 16-byte items of the (n, h, w, 12) row.  Same values, same bits; the loss partials are per
// workgroup as before.
__global__ __launch_bounds__(256) void mse255_sum_s2d3_rows_kernel(SumS2dParts parts, int n_parts, const float* __restrict__ a,
                                                                   const float* __restrict__ b, float* __restrict__ dz,
                                                                   double* __restrict__ partial, long nrows, int h, int w,
                                                                   float gscale) {
    __shared__ double red[4];
    __shared__ __attribute__((aligned(16))) float sh[2 * 6 * 512];            // [top | bottom][6 w]
    double s = 0.0;
    const long count = nrows * w * 12;
    const float gk = gscale * 2.0f * 255.0f * 255.0f / (float)count;
    const int rq = (6 * w) >> 2;                                               // float4 items of one input row (w even)
    const int tid = threadIdx.x;
    for (long row = blockIdx.x; row < nrows; row += gridDim.x) {
        const long im = row / h;
        const int yy = (int)(row - im * h);
        const long top = ((im * 2 * h + 2 * yy) * (2L * w)) * 3;              // float offset of the upper input row (the lower one follows)
        __syncthreads();
        for (int item = tid; item < 2 * rq; item += 256) {
            const long o = top + 4L * item;
            float4 acc = *reinterpret_cast<const float4*>(parts.p[0] + o);
#pragma unroll
            for (int k = 1; k < 6; ++k)
                if (k < n_parts) {
                    const float4 t = *reinterpret_cast<const float4*>(parts.p[k] + o);
                    acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
                }
            const float4 va = *reinterpret_cast<const float4*>(a + o), vb = *reinterpret_cast<const float4*>(b + o);
            const float d0 = va.x - vb.x, d1 = va.y - vb.y, d2 = va.z - vb.z, d3 = va.w - vb.w;
            const float e0 = 255.0f * d0, e1 = 255.0f * d1, e2 = 255.0f * d2, e3 = 255.0f * d3;
            s += (double)e0 * (double)e0;
            s += (double)e1 * (double)e1;
            s += (double)e2 * (double)e2;
            s += (double)e3 * (double)e3;
            *reinterpret_cast<float4*>(sh + 4 * item) = make_float4(fmaf(gk, d0, acc.x), fmaf(gk, d1, acc.y), fmaf(gk, d2, acc.z),
                                                                     fmaf(gk, d3, acc.w));
        }
        __syncthreads();
        // output pixel px = [top 6 px .. + 5 | bottom 6 px .. + 5]: item j = (px, third t) -> t 0: top 0..3; 1: top 4, 5 + bottom 0, 1;
        // 2: bottom 2..5
        const float* st = sh;
        const float* sb = sh + 6 * w;
        float4* dst = reinterpret_cast<float4*>(dz + row * (long)w * 12);
        for (int j = tid; j < 3 * w; j += 256) {
            const int px = j / 3, third = j - 3 * px;
            float f[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 4 * third + e;                                   // channel of the (n, h, w, 12) pixel
                f[e] = k < 6 ? st[6 * px + k] : sb[6 * px + k - 6];
            }
            dst[j] = make_float4(f[0], f[1], f[2], f[3]);
        }
    }
    s = wave_sum_d(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void mse255_final_kernel(const double* __restrict__ partial, int nblocks, long count, float* loss) {
    double s = 0.0;                                      // one wave: strided partials, then a fixed-shape butterfly
    for (int k = threadIdx.x; k < nblocks; k += 64) s += partial[k];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) loss[0] = (float)(s / (double)count);
}

// ---------------------------------------------------------------------------------------------------------------
// SSIM (Wang et al. 2004), per image = mean over channels and VALID window positions.
//   mode 0: skimage.metrics.structural_similarity as helpers/metrics.py:9-25 calls it (7x7 uniform window, sample
//           covariance N/(N-1), K1 .01, K2 .03, interior crop == VALID positions);
//   mode 1: tf.image.ssim as models/compression.py:89 calls it (11x11 Gaussian sigma 1.5, population moments).
// Separable windows (uniform: 1/win x 1/win; tf's Gaussian: normalised outer product, its 1-D factor = the row sums of the
// 2-D table), moments in double.  A workgroup walks 16 x 16 tiles of window positions of one channel: the (16 + win - 1)^2 input
// patch of both images is staged in LDS, the horizontal pass writes the five moment rows (u_a, u_b, u_aa, u_bb, u_ab) to LDS
// in double, the vertical pass finishes one position per thread: 2 x 5 x win fused multiply-adds per position instead of
// 5 x win^2 products with 3 global loads each (it was one thread per position straight from global memory: 403 us for 16 images
// of 256 x 256 x 3, every training step of the codec returns the SSIM - models/compression.py:129).  Per-workgroup partial
// sums, fixed-order finish.
template <int WIN>
__global__ __launch_bounds__(256) void ssim_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           double* __restrict__ partial, int h, int w, int c, int mode,
                                                           float max_val, const float* __restrict__ gk, int blocks_per_image) {
    constexpr int T = 16, HT = T + WIN - 1;
    __shared__ float sa[HT * HT], sb[HT * HT];
    __shared__ double hm[5][HT * T];
    __shared__ double red[256];
    __shared__ double wt1[WIN];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / blocks_per_image, blk = blockIdx.x % blocks_per_image;
    const int ho = h - WIN + 1, wo = w - WIN + 1;
    const int tiles_x = (wo + T - 1) / T, tiles_y = (ho + T - 1) / T, ntiles = tiles_y * tiles_x * c;
    const double c1 = (0.01 * max_val) * (0.01 * max_val), c2 = (0.03 * max_val) * (0.03 * max_val);
    const double np_ = (double)WIN * WIN, covn = mode == 0 ? np_ / (np_ - 1.0) : 1.0;
    if (tid < WIN) {
        double s = 0.0;
        if (mode == 0) s = 1.0 / WIN;
        else
            for (int j = 0; j < WIN; ++j) s += (double)gk[tid * WIN + j];
        wt1[tid] = s;
    }
    __syncthreads();
    // The float32 table sums to 1 - 6e-9 and the outer product of its row sums to 1 - 1.2e-8: on flat regions that residue,
    // divided by c2, moved the result by 1e-6 (constant images p, q must give (2pq + c1) / (p^2 + q^2 + c1)).  The Gaussian
    // factor is therefore normalised here, in double; the uniform factor 1 / WIN is left as it is.
    double wsum = 0.0;
#pragma unroll
    for (int k = 0; k < WIN; ++k) wsum += wt1[k];
    const double wnorm = mode == 0 ? 1.0 : 1.0 / wsum;
    double wt[WIN];
#pragma unroll
    for (int k = 0; k < WIN; ++k) wt[k] = wt1[k] * wnorm;
    double sum = 0.0;
    for (int t = blk; t < ntiles; t += blocks_per_image) {
        const int ch = t % c, tile = t / c, ty0 = (tile / tiles_x) * T, tx0 = (tile % tiles_x) * T;
        __syncthreads();                                       // the previous tile's moment rows are consumed
        for (int i = tid; i < HT * HT; i += 256) {
            const int gy = ty0 + i / HT, gx = tx0 + i % HT;
            const bool ok = gy < h && gx < w;
            const long o = (((long)n * h + (ok ? gy : 0)) * w + (ok ? gx : 0)) * c + ch;
            sa[i] = ok ? a[o] : 0.f;
            sb[i] = ok ? b[o] : 0.f;
        }
        __syncthreads();
        for (int i = tid; i < HT * T; i += 256) {
            const int r = i / T, cc = i % T;
            double ux = 0, uy = 0, uxx = 0, uyy = 0, uxy = 0;
#pragma unroll
            for (int dx = 0; dx < WIN; ++dx) {
                const double va = sa[r * HT + cc + dx], vb = sb[r * HT + cc + dx], wv = wt[dx];
                const double wa = wv * va, wb = wv * vb;
                ux += wa; uy += wb; uxx += wa * va; uyy += wb * vb; uxy += wa * vb;
            }
            hm[0][i] = ux; hm[1][i] = uy; hm[2][i] = uxx; hm[3][i] = uyy; hm[4][i] = uxy;
        }
        __syncthreads();
        const int oy = tid / T, ox = tid % T;
        if (ty0 + oy < ho && tx0 + ox < wo) {
            double ux = 0, uy = 0, uxx = 0, uyy = 0, uxy = 0;
#pragma unroll
            for (int dy = 0; dy < WIN; ++dy) {
                const int i = (oy + dy) * T + ox;
                const double wv = wt[dy];
                ux += wv * hm[0][i]; uy += wv * hm[1][i]; uxx += wv * hm[2][i]; uyy += wv * hm[3][i]; uxy += wv * hm[4][i];
            }
            const double vx = covn * (uxx - ux * ux), vy = covn * (uyy - uy * uy), vxy = covn * (uxy - ux * uy);
            sum += ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
        }
    }
    red[tid] = sum;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = red[0];
}

__global__ void ssim_final_kernel(const double* __restrict__ partial, float* __restrict__ out, int blocks_per_image,
                                  double inv_items) {
    const int n = blockIdx.x;
    double s = 0.0;
    for (int k = threadIdx.x; k < blocks_per_image; k += 64) s += partial[(long)n * blocks_per_image + k];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) out[n] = (float)(s * inv_items);
}

}  // namespace

extern "C" {

size_t nimg_mae255_workspace_bytes(void) { return 2048 * sizeof(double); }

int nimg_mae255(const float* a, const float* b, float* loss, float* grad_a, long count, float grad_scale,
                int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    if (!a || !b || !loss || count <= 0 || !workspace) return NIMG_ERR_ARG;
    if (workspace_bytes < nimg_mae255_workspace_bytes()) return NIMG_ERR_WORKSPACE;
    const int grid = grid_for(count);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mae255_kernel, dim3(grid), dim3(256), 0, s, a, b, grad_a, (double*)workspace, count, grad_scale,
                       accumulate);
    NIMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(mean_final_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, grid, 1.0 / (double)count,
                       1.0, 0.0, loss);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

size_t nimg_ssim_loss_workspace_bytes(int n, int h, int w, int c, int with_grad) {
    if (n <= 0 || h < WIN || w < WIN || c <= 0) return 0;
    const size_t partials = (size_t)n * BPI * sizeof(double);
    const size_t maps = with_grad ? (size_t)3 * n * (h - WIN + 1) * (w - WIN + 1) * c * sizeof(float) : 0;
    return partials + maps;
}

int nimg_ssim_loss(const float* y, const float* t, float* loss, float* grad_y, int n, int h, int w, int c,
                   float max_val, const float* gauss_win, float grad_scale, int accumulate, void* workspace,
                   size_t workspace_bytes, void* stream) {
    if (!y || !t || !loss || !gauss_win || !workspace || n <= 0 || c <= 0 || h < WIN || w < WIN || !(max_val > 0.f))
        return NIMG_ERR_ARG;
    if (workspace_bytes < nimg_ssim_loss_workspace_bytes(n, h, w, c, grad_y != nullptr)) return NIMG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long items = (long)(h - WIN + 1) * (w - WIN + 1) * c, plane = (long)n * items;
    double* partial = (double*)workspace;
    float* maps = grad_y ? (float*)(partial + (size_t)n * BPI) : nullptr;
    const double coef = -255.0 / ((double)n * (double)items);
    hipLaunchKernelGGL(ssim_loss_stats_kernel, dim3(n * BPI), dim3(256), 0, s, y, t, partial, maps, plane, h, w, c,
                       max_val, gauss_win, coef);
    NIMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(mean_final_kernel, dim3(1), dim3(64), 0, s, (const double*)partial, n * BPI,
                       1.0 / ((double)n * (double)items), -255.0, 255.0, loss);
    NIMG_CHECK_LAUNCH();
    if (grad_y) {
        hipLaunchKernelGGL(ssim_loss_grad_kernel, dim3(grid_for((long)n * h * w * c)), dim3(256), 0, s, y, t, maps, plane,
                           grad_y, n, h, w, c, gauss_win, grad_scale, accumulate, (const float*)nullptr);
        NIMG_CHECK_LAUNCH();
    }
    return NIMG_OK;
}

size_t nimg_ssim_planes_workspace_bytes(int n, int c) { return (size_t)2 * n * c * BPP * sizeof(double); }

int nimg_ssim_planes(const float* y, const float* t, int n, int h, int w, int c, float max_val, const float* gauss_win,
                     float* mean_ssim, float* mean_cs, float* maps, int which_maps, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (!y || !t || !gauss_win || !workspace || n <= 0 || c <= 0 || h < WIN || w < WIN || !(max_val > 0.f) ||
        which_maps < 0 || which_maps > 2 || (which_maps && !maps) || (long)n * c * BPP > 0x7fffffffL)
        return NIMG_ERR_ARG;
    if (workspace_bytes < nimg_ssim_planes_workspace_bytes(n, c)) return NIMG_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long plane = (long)n * (h - WIN + 1) * (w - WIN + 1) * c;
    hipLaunchKernelGGL(ssim_planes_kernel, dim3(n * c * BPP), dim3(256), 0, s, y, t, (double*)workspace, maps, plane, h, w,
                       c, max_val, gauss_win, which_maps);
    NIMG_CHECK_LAUNCH();
    const int planes = n * c;
    hipLaunchKernelGGL(ssim_planes_final_kernel, dim3((planes + 63) / 64), dim3(64), 0, s, (const double*)workspace, planes,
                       1.0 / ((double)(h - WIN + 1) * (w - WIN + 1)), mean_ssim, mean_cs);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_msssim_combine(const float* values, const float* items, int scales, int planes, float* loss, float* coef,
                        void* stream) {
    if (!values || !items || !loss || scales < 1 || scales > 5 || planes <= 0) return NIMG_ERR_ARG;
    hipLaunchKernelGGL(msssim_combine_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, values, items, scales, planes,
                       loss, coef);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_ssim_maps_grad(const float* y, const float* t, const float* maps, const float* coef, float* grad_y, int n,
                        int h, int w, int c, const float* gauss_win, float grad_scale, int accumulate, void* stream) {
    if (!y || !t || !maps || !grad_y || !gauss_win || n <= 0 || c <= 0 || h < WIN || w < WIN) return NIMG_ERR_ARG;
    const long plane = (long)n * (h - WIN + 1) * (w - WIN + 1) * c;
    hipLaunchKernelGGL(ssim_loss_grad_kernel, dim3(grid_for((long)n * h * w * c)), dim3(256), 0, (hipStream_t)stream, y,
                       t, maps, plane, grad_y, n, h, w, c, gauss_win, grad_scale, accumulate, coef);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

size_t nimg_mse255_workspace_bytes(void) { return 2048 * sizeof(double); }

int nimg_mse255(const float* a, const float* b, float* loss, float* grad_a, long count, float grad_scale,
                int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    if (!a || !b || !loss || count <= 0 || !workspace) return NIMG_ERR_ARG;
    if (workspace_bytes < nimg_mse255_workspace_bytes()) return NIMG_ERR_WORKSPACE;
    const int grid = grid_for(count);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mse255_kernel, dim3(grid), dim3(256), 0, s, a, b, grad_a, (double*)workspace, count,
                       grad_scale, accumulate);
    NIMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(mse255_final_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, grid, count, loss);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_mse255_sum_s2d3(const float* const* parts, int n_parts, const float* y, const float* target, float* loss, float* dz,
                         int n, int h, int w, float grad_scale, void* workspace, size_t workspace_bytes, void* stream) {
    if (n == 0) return NIMG_OK;
    if (!parts || n_parts < 1 || n_parts > 6 || !y || !target || !loss || !dz || !workspace || n < 0 || h <= 0 || w <= 0)
        return NIMG_ERR_ARG;
    if (workspace_bytes < nimg_mse255_workspace_bytes()) return NIMG_ERR_WORKSPACE;
    SumS2dParts sp;
    for (int i = 0; i < 6; ++i) {
        sp.p[i] = i < n_parts ? parts[i] : nullptr;
        if (i < n_parts && (!parts[i] || ((size_t)parts[i] & 7))) return NIMG_ERR_ARG;
    }
    if (((size_t)y & 7) || ((size_t)target & 7) || ((size_t)dz & 15)) return NIMG_ERR_ARG;
    const long npix = (long)n * h * w;
    int grid = grid_for(npix);
    hipStream_t s = (hipStream_t)stream;
    bool a16 = (((size_t)y | (size_t)target) & 15) == 0;
    for (int i = 0; i < n_parts; ++i) a16 = a16 && ((size_t)parts[i] & 15) == 0;
    static const bool no_rows = getenv("NIMG_NO_S2D3_ROWS") != nullptr;
    if (!no_rows && a16 && (w & 1) == 0 && w <= 512) {          // row form: linear 16-byte items on both sides
        const long nrows = (long)n * h;
        grid = (int)(nrows < 2048 ? nrows : 2048);
        hipLaunchKernelGGL(mse255_sum_s2d3_rows_kernel, dim3(grid), dim3(256), 0, s, sp, n_parts, y, target, dz, (double*)workspace,
                           nrows, h, w, grad_scale);
    } else {
        hipLaunchKernelGGL(mse255_sum_s2d3_kernel, dim3(grid), dim3(256), 0, s, sp, n_parts, y, target, dz, (double*)workspace, npix,
                           h, w, grad_scale);
    }
    NIMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(mse255_final_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, grid, npix * 12, loss);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

size_t nimg_ssim_workspace_bytes(int n) { return (size_t)n * 64 * sizeof(double); }

int nimg_ssim(const float* a, const float* b, float* out, int n, int h, int w, int c, int mode, float max_val,
              const float* gauss_win, void* workspace, size_t workspace_bytes, void* stream) {
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    const int win = mode == 0 ? 7 : 11;
    if (!a || !b || !out || !workspace || n < 0 || c <= 0 || h < win || w < win || mode < 0 || mode > 1) return NIMG_ERR_ARG;
    if (mode == 1 && !gauss_win) return NIMG_ERR_ARG;
    if (workspace_bytes < nimg_ssim_workspace_bytes(n)) return NIMG_ERR_WORKSPACE;
    if (n == 0) return NIMG_OK;
    hipStream_t s = (hipStream_t)stream;
    const int bpi = 64;
    if (mode == 0)
        hipLaunchKernelGGL(ssim_partial_kernel<7>, dim3(n * bpi), dim3(256), 0, s, a, b, (double*)workspace, h, w, c, mode, max_val,
                           gauss_win, bpi);
    else
        hipLaunchKernelGGL(ssim_partial_kernel<11>, dim3(n * bpi), dim3(256), 0, s, a, b, (double*)workspace, h, w, c, mode, max_val,
                           gauss_win, bpi);
    NIMG_CHECK_LAUNCH();
    const double items = (double)(h - win + 1) * (w - win + 1) * c;
    hipLaunchKernelGGL(ssim_final_kernel, dim3(n), dim3(64), 0, s, (const double*)workspace, out, bpi, 1.0 / items);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

}  // extern "C"
