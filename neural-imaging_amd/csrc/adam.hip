// The optimiser step of the imaging channel (gfx950): Keras Adam over a flat parameter buffer (tf.keras.optimizers.Adam,
// models/pipelines.py:51 etc.), the form that also keeps the bf16 weight images and the ConstrainedConv2D filter current, and the
// NaN flag the step is skipped by.
#include "common.h"
#include "constrained.h"

namespace {

using namespace nimg;

// ---------------------------------------------------------------------------------------------------------------
// Keras Adam: theta -= lr_t * m / (sqrt(v) + eps), lr_t = lr * sqrt(1-b2^t)/(1-b1^t); optional grad pre-scale
// One element: m, v in / out, returns the new parameter.  Every product is rounded on its own before it is added: that is what
// adam_kernel has always computed (hipcc pairs its products into v_pk_mul_f32 before it looks for a*b+c), but the same
// expressions unrolled sixteen times in adam_images_kernel came out as v_fmac_f32 - another rounding.  The empty asm hides a
// product from the contraction pass and costs no instruction; both kernels go through this one function.
__device__ __forceinline__ float rounded(float x) {
    asm("" : "+v"(x));
    return x;
}

__device__ __forceinline__ float adam_value(float pi, float g, float& m, float& v, float lr_t, float b1, float b2, float eps,
                                            float gscale) {
    const float gi = gscale * g;
    const float mi = rounded(b1 * m) + rounded((1.0f - b1) * gi);
    const float vi = rounded(b2 * v) + rounded((1.0f - b2) * gi * gi);
    m = mi;
    v = vi;
    return pi - lr_t * mi / (sqrtf(vi) + eps);
}

__device__ __forceinline__ float adam_at(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                         float* __restrict__ v, long i, float lr_t, float b1, float b2, float eps, float gscale) {
    float mi = m[i], vi = v[i];
    const float pn = adam_value(p[i], g[i], mi, vi, lr_t, b1, b2, eps, gscale);
    m[i] = mi;
    v[i] = vi;
    p[i] = pn;
    return pn;
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long count, float lr_t, float b1, float b2, float eps,
                            float gscale, const int* __restrict__ skip_flag, const float* __restrict__ lr_t_dev) {
    if (skip_flag && skip_flag[0]) return;      // NaN gradients: leave the model untouched (reference raises first)
    if (lr_t_dev) lr_t = lr_t_dev[0];           // captured step: the bias-corrected rate of THIS replay lives on the device
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long)gridDim.x * blockDim.x)
        adam_at(p, g, m, v, i, lr_t, b1, b2, eps, gscale);
}

// The update AND both bf16 images of every registered 4-D weight (the table of nimg_conv_weights_bf16_batch: entries 2j / 2j + 1 =
// mode 0 / mode 1 of weight j; the weights lie inside [p, p + count), ascending, apart) in one launch: the images are functions
// of the master weights alone, and those change only here - built at the head of each forward they were 29 + 10 us of launches
// with the chip idle, re-reading what this kernel has in registers.
//   blockIdx.y = j < n_weights: the workgroups walk the (tap, 64 cin, 64 cout) blocks of weight j.  A block is updated once,
//       kept in LDS as [cin][cout], and emitted as the four 16-cin chunks of the mode-0 image (rows = cout) and the four 16-cout
//       chunks of the mode-1 image (rows = cin, taps reversed) - the pieces weights_bf16_batch_kernel writes, 8 bytes per
//       thread; channels beyond cin / cout are the images' zero padding.
//   blockIdx.y = n_weights: everything between the weights (biases, 2-D kernels, alignment gaps), the plain loop.
//   cc.kernel = one of the weights, a ConstrainedConv2D kernel (optional): see below.
constexpr int ADAM_IMG_GRID = 192;
struct AdamConstrained { const float* kernel; float* nf; float* nft; float strength; int ks, c; };
__global__ __launch_bounds__(256) void adam_images_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v, long count,
                                                          float lr_t, float b1, float b2, float eps, float gscale,
                                                          const int* __restrict__ skip_flag,
                                                          const float* __restrict__ lr_t_dev,
                                                          const long long* __restrict__ table, int n_weights,
                                                          const AdamConstrained cc) {
    if (skip_flag && skip_flag[0]) return;      // nothing is written: the images stay those of the unchanged weights
    if (lr_t_dev) lr_t = lr_t_dev[0];
    const int tid = threadIdx.x;
    if ((int)blockIdx.y == n_weights) {
        for (int gap = 0; gap <= n_weights; ++gap) {
            long lo = 0, hi = count;
            if (gap > 0) {
                const long long* e = table + 8 * (gap - 1);
                lo = (reinterpret_cast<const float*>(e[0]) - p) + (e[2] >> 32) * (e[3] >> 32) * (e[3] & 0xffffffffll);
            }
            if (gap < n_weights) hi = reinterpret_cast<const float*>(table[8 * gap]) - p;
            for (long i = lo + (long)blockIdx.x * 256 + tid; i < hi; i += (long)gridDim.x * 256)
                adam_at(p, g, m, v, i, lr_t, b1, b2, eps, gscale);
        }
        return;
    }
    const long long* e = table + 8 * blockIdx.y;
    const long base = reinterpret_cast<const float*>(e[0]) - p;
    __bf16* wb0 = reinterpret_cast<__bf16*>(e[1]);
    __bf16* wb1 = reinterpret_cast<__bf16*>(e[5]);
    const int taps = (int)(e[2] >> 32), cin = (int)(e[3] >> 32), cout = (int)(e[3] & 0xffffffffll);
    const int cib = (cin + 63) / 64, cob = (cout + 63) / 64, nblocks = taps * cib * cob;
    const int chunks0 = (cin + 15) / 16, chunks1 = (cout + 15) / 16;
    __shared__ float tile[64][65];
    if (reinterpret_cast<const float*>(e[0]) == cc.kernel && taps == cc.ks * cc.ks && cin == cc.c && cout == cc.c) {
        // The ConstrainedConv2D kernel (225 values): ONE workgroup updates it whole, keeps it in LDS, and makes from there its two
        // images (element by element, as weights_bf16_kernel) and what the forward pass and the input gradient read of it - the
        // normalised filter and its flipped form (constrained_fwd_kernel was 18 us of three threads summing 75 L2 reads each).
        if (blockIdx.x != 0) return;
        __shared__ float df[16];
        float* kl = &tile[0][0];
        const int total = taps * cin * cout;               // <= 4096 (entry point)
        for (int i = tid; i < total; i += 256) kl[i] = adam_at(p, g, m, v, base + i, lr_t, b1, b2, eps, gscale);
        __syncthreads();
        const int cpad = (cin + 15) / 16 * 16;             // cin == cout: the same padding in both modes
        for (int i = tid; i < taps * cin * cpad; i += 256) {
            const int c = i % 16 + 16 * (i / (16 * cin * taps)), r = (i / 16) % cin, t = (i / (16 * cin)) % taps;
            wb0[i] = (__bf16)(c < cin ? kl[(t * cin + c) * cout + r] : 0.f);
            wb1[i] = (__bf16)(c < cout ? kl[((taps - 1 - t) * cin + r) * cout + c] : 0.f);
        }
        constrained_normalise(kl, cc.nf, cc.nft, df, cc.ks, cc.c, cc.strength);
        return;
    }
    const int col = tid & 63, row4 = tid >> 6;             // update: a wave = 64 consecutive couts of one cin row
    const int rl = tid >> 2, kq = (tid & 3) * 4;           // emit: a thread = 4 consecutive k of one image row
    for (int bl = blockIdx.x; bl < nblocks; bl += gridDim.x) {
        const int co0 = (bl % cob) * 64, ci0 = (bl / cob % cib) * 64, t = bl / (cob * cib);
        const long at = base + ((long)t * cin + ci0 + row4) * cout + co0 + col;
        __syncthreads();
        if (ci0 + 64 <= cin && co0 + 64 <= cout) {         // whole block: no predicate, every load of the block in flight at once
            float pv[16], gv[16], mv[16], vv[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const long i = at + (long)4 * k * cout;
                pv[k] = p[i]; gv[k] = g[i]; mv[k] = m[i]; vv[k] = v[i];
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const long i = at + (long)4 * k * cout;
                pv[k] = adam_value(pv[k], gv[k], mv[k], vv[k], lr_t, b1, b2, eps, gscale);
                m[i] = mv[k]; v[i] = vv[k]; p[i] = pv[k];
                tile[row4 + 4 * k][col] = pv[k];
            }
        } else {
            for (int k = 0; k < 16; ++k) {
                const bool in = ci0 + row4 + 4 * k < cin && co0 + col < cout;
                tile[row4 + 4 * k][col] = in ? adam_at(p, g, m, v, at + (long)4 * k * cout, lr_t, b1, b2, eps, gscale) : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int chunk = ci0 / 16 + c;
            if (chunk < chunks0 && co0 + rl < cout) {
                nimg_bf16x4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = (__bf16)tile[16 * c + kq + k][rl];
                *reinterpret_cast<nimg_bf16x4*>(wb0 + (((long)chunk * taps + t) * cout + co0 + rl) * 16 + kq) = o;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int chunk = co0 / 16 + c;
            if (chunk < chunks1 && ci0 + rl < cin) {
                nimg_bf16x4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = (__bf16)tile[rl][16 * c + kq + k];
                *reinterpret_cast<nimg_bf16x4*>(wb1 + (((long)chunk * taps + (taps - 1 - t)) * cin + ci0 + rl) * 16 + kq) = o;
            }
        }
    }
}

// flag[0] = 1 if any element is NaN (workflows/manipulation_classification.py:281-282, kept on device)
__global__ void nan_flag_kernel(const float* __restrict__ g, long count, int* flag) {
    bool bad = false;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long)gridDim.x * blockDim.x)
        bad |= (g[i] != g[i]);
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

}  // namespace

extern "C" {

int nimg_adam_step(float* params, const float* grads, float* m, float* v, long count, float lr, float beta1,
                   float beta2, float eps, int step, float grad_scale, const int* skip_flag, void* stream) {
    if (!params || !grads || !m || !v || count < 0 || step < 1) return NIMG_ERR_ARG;
    if (count == 0) return NIMG_OK;
    const double lr_t = (double)lr * __builtin_sqrt(1.0 - __builtin_pow((double)beta2, (double)step)) /
                        (1.0 - __builtin_pow((double)beta1, (double)step));
    hipLaunchKernelGGL(adam_kernel, dim3(grid_for(count)), dim3(256), 0, (hipStream_t)stream, params, grads, m, v,
                       count, (float)lr_t, beta1, beta2, eps, grad_scale, skip_flag, (const float*)nullptr);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_adam_step_dev(float* params, const float* grads, float* m, float* v, long count, const float* lr_t, float beta1,
                       float beta2, float eps, float grad_scale, const int* skip_flag, void* stream) {
    if (!params || !grads || !m || !v || !lr_t || count < 0) return NIMG_ERR_ARG;
    if (count == 0) return NIMG_OK;
    hipLaunchKernelGGL(adam_kernel, dim3(grid_for(count)), dim3(256), 0, (hipStream_t)stream, params, grads, m, v,
                       count, 0.f, beta1, beta2, eps, grad_scale, skip_flag, lr_t);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_adam_step_images(float* params, const float* grads, float* m, float* v, long count, float lr, const float* lr_t,
                          float beta1, float beta2, float eps, int step, float grad_scale, const int* skip_flag,
                          const void* image_table, int n_entries, const float* cc_kernel, float* cc_nf, float* cc_nft,
                          int cc_ks, int cc_channels, float cc_strength, void* stream) {
    if (!params || !grads || !m || !v || count < 0 || (!lr_t && step < 1)) return NIMG_ERR_ARG;
    if (n_entries < 0 || (n_entries & 1) || n_entries / 2 >= 65535 || (n_entries && !image_table)) return NIMG_ERR_ARG;
    if (cc_kernel && (!cc_nf || cc_ks <= 0 || cc_channels <= 0 || cc_channels > 16 ||
                      (long)cc_ks * cc_ks * cc_channels * cc_channels > 4096 || cc_kernel < params ||
                      cc_kernel + cc_ks * cc_ks * cc_channels * cc_channels > params + count))
        return NIMG_ERR_ARG;
    if (count == 0) return NIMG_OK;
    const AdamConstrained cc{cc_kernel, cc_nf, cc_nft, cc_strength, cc_ks, cc_channels};
    float rate = 0.f;
    if (!lr_t)
        rate = (float)((double)lr * __builtin_sqrt(1.0 - __builtin_pow((double)beta2, (double)step)) /
                       (1.0 - __builtin_pow((double)beta1, (double)step)));
    hipLaunchKernelGGL(adam_images_kernel, dim3(ADAM_IMG_GRID, (unsigned)(n_entries / 2 + 1)), dim3(256), 0, (hipStream_t)stream,
                       params, grads, m, v, count, rate, beta1, beta2, eps, grad_scale, skip_flag, lr_t,
                       (const long long*)image_table, n_entries / 2, cc);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_nan_flag(const float* g, long count, int* flag, void* stream) {
    if (!g || !flag || count < 0) return NIMG_ERR_ARG;
    if (count == 0) return NIMG_OK;
    hipLaunchKernelGGL(nan_flag_kernel, dim3(grid_for(count)), dim3(256), 0, (hipStream_t)stream, g, count, flag);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

}  // extern "C"
