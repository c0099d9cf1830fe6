// 2x2 max-pooling of the imaging channel (gfx950), float32 and bf16, HBM-bound: float4 / 16-byte accesses along the NHWC channel
// axis, grid-stride loops capped at 2048 workgroups (common.h grid_for).
//
//   max-pool 2x2 fwd / bwd(+skip add, +LeakyReLU')        models/pipelines.py:197, models/forensics.py:70
//   un-pool: the backward of the fused conv -> LeakyReLU -> max-pool epilogue, from the pooled tensor and its arg-max bytes
#include "common.h"

namespace {

using namespace nimg;

// ---------------------------------------------------------------------------------------------------------------
template <int V>
__global__ void maxpool2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int h, int w, int c) {
    const int ho = h / 2, wo = w / 2, cv = c / V;
    const long total = (long)n * ho * wo * cv;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cv) * V;
        long r = i / cv;
        const int ox = (int)(r % wo);
        r /= wo;
        const int oy = (int)(r % ho), im = (int)(r / ho);
        const float* p00 = x + (((long)im * h + 2 * oy) * w + 2 * ox) * c + cc;
        const float* p10 = p00 + (long)w * c;
        float* q = y + (((long)im * ho + oy) * wo + ox) * c + cc;
        if (V == 4) {
            const float4 a = *reinterpret_cast<const float4*>(p00), b = *reinterpret_cast<const float4*>(p00 + c);
            const float4 d = *reinterpret_cast<const float4*>(p10), e = *reinterpret_cast<const float4*>(p10 + c);
            *reinterpret_cast<float4*>(q) = make_float4(fmaxf(fmaxf(a.x, b.x), fmaxf(d.x, e.x)), fmaxf(fmaxf(a.y, b.y), fmaxf(d.y, e.y)),
                                                        fmaxf(fmaxf(a.z, b.z), fmaxf(d.z, e.z)), fmaxf(fmaxf(a.w, b.w), fmaxf(d.w, e.w)));
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) q[k] = fmaxf(fmaxf(p00[k], p00[c + k]), fmaxf(p10[k], p10[c + k]));
        }
    }
}

// dz[n,y,x,c] = (first arg-max of the window ? dp : 0) [+ add] ) * [lrelu'(y)]
// Backward of the fused conv -> LeakyReLU -> MaxPool2D epilogue (nimg_conv2d_pool_fwd): the full-resolution activation
// was never stored, so the pre-activation gradient is rebuilt from the pooled tensor, its argmax byte and the
// upstream gradient: dz[window position] = (position == argmax) ? dp * lrelu'(pooled) : 0.  (The sign of the window
// maximum is the sign of the pooled value, which is all lrelu' needs.)

// bf16 in, bf16 out, no activation mask (what the FAN's backward runs in throughput mode): 8 channels per thread - one
// 16-byte load of the pooled gradient, 8 arg-max bytes, four 16-byte stores - and the routing is done on the packed bf16
// pairs with byte-wise equality masks (no float conversions).
__device__ __forceinline__ unsigned unpool_eq_bytes(unsigned k, unsigned pos) {      // 0xFF in every byte of k equal to pos (0..3)
    const unsigned x = k ^ (pos * 0x01010101u);
    return (((x | (x >> 1)) & 0x01010101u) ^ 0x01010101u) * 0xFFu;
}

__global__ void maxpool2_unpool_bf16x8_kernel(const uint4* __restrict__ dp, const uint2* __restrict__ idx, uint4* __restrict__ dz,
                                              int n, int ho, int wo, int c8) {
    const long total = (long)n * ho * wo * c8;
    const long row = (long)2 * wo * c8;                    // uint4 entries per full-resolution row
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % c8);
        long r = i / c8;
        const int ox = (int)(r % wo);
        r /= wo;                                            // r = im * ho + oy
        const uint4 g = dp[i];
        const uint2 k = idx[i];
        const long base = (2 * r * (long)(2 * wo) + 2 * ox) * c8 + cc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned m0 = unpool_eq_bytes(k.x, q), m1 = unpool_eq_bytes(k.y, q);
            uint4 o;
            o.x = g.x & __builtin_amdgcn_perm(m0, m0, 0x01010000u);
            o.y = g.y & __builtin_amdgcn_perm(m0, m0, 0x03030202u);
            o.z = g.z & __builtin_amdgcn_perm(m1, m1, 0x01010000u);
            o.w = g.w & __builtin_amdgcn_perm(m1, m1, 0x03030202u);
            dz[base + (q >> 1) * row + (q & 1) * c8] = o;
        }
    }
}

template <bool IN_BF16, bool OUT_BF16>
__global__ void maxpool2_unpool_kernel(const float* __restrict__ dp, const unsigned char* __restrict__ idx,
                                       const float* __restrict__ pooled, float* __restrict__ dz, int n, int ho, int wo,
                                       int c, int apply_mask, float alpha) {
    const int cv = c / 4, w = 2 * wo;
    const long total = (long)n * ho * wo * cv;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cv) * 4;
        long r = i / cv;
        const int ox = (int)(r % wo);
        r /= wo;
        const int oy = (int)(r % ho), im = (int)(r / ho);
        const long po = (((long)im * ho + oy) * wo + ox) * c + cc;
        float4 g;
        if (IN_BF16) {
            const nimg_bf16x4 gb = *reinterpret_cast<const nimg_bf16x4*>(reinterpret_cast<const __bf16*>(dp) + po);
            g = make_float4((float)gb[0], (float)gb[1], (float)gb[2], (float)gb[3]);
        } else {
            g = *reinterpret_cast<const float4*>(dp + po);
        }
        const uchar4 k = *reinterpret_cast<const uchar4*>(idx + po);
        if (apply_mask) {
            const float4 pv = *reinterpret_cast<const float4*>(pooled + po);
            g.x *= pv.x > 0.f ? 1.0f : alpha; g.y *= pv.y > 0.f ? 1.0f : alpha;
            g.z *= pv.z > 0.f ? 1.0f : alpha; g.w *= pv.w > 0.f ? 1.0f : alpha;
        }
        const long base = (((long)im * 2 * ho + 2 * oy) * w + 2 * ox) * c + cc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 o = make_float4(k.x == q ? g.x : 0.f, k.y == q ? g.y : 0.f, k.z == q ? g.z : 0.f,
                                         k.w == q ? g.w : 0.f);
            const long off = base + (long)(q >> 1) * w * c + (long)(q & 1) * c;
            if (OUT_BF16) {
                nimg_bf16x4 ob;
                ob[0] = (__bf16)o.x; ob[1] = (__bf16)o.y; ob[2] = (__bf16)o.z; ob[3] = (__bf16)o.w;
                *reinterpret_cast<nimg_bf16x4*>(reinterpret_cast<__bf16*>(dz) + off) = ob;
            } else {
                *reinterpret_cast<float4*>(dz + off) = o;
            }
        }
    }
}

// bf16-stored activations (UNet in throughput mode): 8 channels = 16 bytes per lane.  Rounding to bf16 is monotonic, so
// the maximum of the rounded values is the rounded maximum - pooling bf16 tensors changes nothing for their bf16 consumers.
typedef __bf16 nimg_bf16x8 __attribute__((ext_vector_type(8)));
__global__ void maxpool2_fwd_bf16_kernel(const __bf16* __restrict__ x, __bf16* __restrict__ y, int n, int h, int w, int c) {
    const int ho = h / 2, wo = w / 2, cv = c / 8;
    const long total = (long)n * ho * wo * cv;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cv) * 8;
        long r = i / cv;
        const int ox = (int)(r % wo);
        r /= wo;
        const int oy = (int)(r % ho), im = (int)(r / ho);
        const __bf16* p00 = x + (((long)im * h + 2 * oy) * w + 2 * ox) * c + cc;
        const __bf16* p10 = p00 + (long)w * c;
        const nimg_bf16x8 a = *reinterpret_cast<const nimg_bf16x8*>(p00), b = *reinterpret_cast<const nimg_bf16x8*>(p00 + c);
        const nimg_bf16x8 d = *reinterpret_cast<const nimg_bf16x8*>(p10), e = *reinterpret_cast<const nimg_bf16x8*>(p10 + c);
        nimg_bf16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            o[k] = (__bf16)fmaxf(fmaxf((float)a[k], (float)b[k]), fmaxf((float)d[k], (float)e[k]));
        *reinterpret_cast<nimg_bf16x8*>(y + (((long)im * ho + oy) * wo + ox) * c + cc) = o;
    }
}

// maxpool2_bwd_kernel on bf16-stored tensors (dp, yact, add, dz all bf16): same first-maximum routing, skip-gradient add
// and LeakyReLU' factor, float32 arithmetic per element, one rounding at the store.
__global__ void maxpool2_bwd_bf16_kernel(const __bf16* __restrict__ dp, const __bf16* __restrict__ yact, const __bf16* add,
                                         __bf16* dz, int n, int h, int w, int c, int apply_mask, float alpha) {
    const int ho = h / 2, wo = w / 2, cv = c / 8;
    const long total = (long)n * ho * wo * cv;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cv) * 8;
        long r = i / cv;
        const int ox = (int)(r % wo);
        r /= wo;
        const int oy = (int)(r % ho), im = (int)(r / ho);
        const long base = (((long)im * h + 2 * oy) * w + 2 * ox) * c + cc;
        const long offs[4] = {0, (long)c, (long)w * c, (long)w * c + c};
        nimg_bf16x8 v[4], a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[q] = *reinterpret_cast<const nimg_bf16x8*>(yact + base + offs[q]);
            if (add) a[q] = *reinterpret_cast<const nimg_bf16x8*>(add + base + offs[q]);
        }
        const nimg_bf16x8 g = *reinterpret_cast<const nimg_bf16x8*>(dp + (((long)im * ho + oy) * wo + ox) * c + cc);
        nimg_bf16x8 o[4];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float v0 = (float)v[0][k], v1 = (float)v[1][k], v2 = (float)v[2][k], v3 = (float)v[3][k];
            const float m = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
            const int sel = v0 == m ? 0 : (v1 == m ? 1 : (v2 == m ? 2 : 3));
            const float vv[4] = {v0, v1, v2, v3};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float t = (q == sel) ? (float)g[k] : 0.f;
                if (add) t += (float)a[q][k];
                if (apply_mask) t *= (vv[q] > 0.f ? 1.0f : alpha);
                o[q][k] = (__bf16)t;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<nimg_bf16x8*>(dz + base + offs[q]) = o[q];
    }
}

// V channels per thread; V == 4 moves float4s (16 B per lane, coalesced along the NHWC channel axis)
template <int V>
__global__ void maxpool2_bwd_kernel(const float* __restrict__ dp, const float* __restrict__ yact,
                                    const float* add, float* dz, int n, int h, int w, int c, int apply_mask,
                                    float alpha) {
    const int ho = h / 2, wo = w / 2, cv = c / V;
    const long total = (long)n * ho * wo * cv;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cc = (int)(i % cv) * V;
        long r = i / cv;
        const int ox = (int)(r % wo);
        r /= wo;
        const int oy = (int)(r % ho), im = (int)(r / ho);
        const long base = (((long)im * h + 2 * oy) * w + 2 * ox) * c + cc;
        const long offs[4] = {0, (long)c, (long)w * c, (long)w * c + c};
        float v[4][V], a[4][V], g[V], o[4][V];
        if (V == 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 t = *reinterpret_cast<const float4*>(yact + base + offs[q]);
                v[q][0] = t.x; v[q][1] = t.y; v[q][2] = t.z; v[q][3] = t.w;
                if (add) {
                    const float4 u = *reinterpret_cast<const float4*>(add + base + offs[q]);
                    a[q][0] = u.x; a[q][1] = u.y; a[q][2] = u.z; a[q][3] = u.w;
                }
            }
            const float4 t = *reinterpret_cast<const float4*>(dp + (((long)im * ho + oy) * wo + ox) * c + cc);
            g[0] = t.x; g[1] = t.y; g[2] = t.z; g[3] = t.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    v[q][k] = yact[base + offs[q] + k];
                    if (add) a[q][k] = add[base + offs[q] + k];
                }
#pragma unroll
            for (int k = 0; k < V; ++k) g[k] = dp[(((long)im * ho + oy) * wo + ox) * c + cc + k];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float m = fmaxf(fmaxf(v[0][k], v[1][k]), fmaxf(v[2][k], v[3][k]));
            int sel = 3;
            if (v[0][k] == m) sel = 0; else if (v[1][k] == m) sel = 1; else if (v[2][k] == m) sel = 2;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float t = (q == sel) ? g[k] : 0.f;
                if (add) t += a[q][k];
                if (apply_mask) t *= (v[q][k] > 0.f ? 1.0f : alpha);
                o[q][k] = t;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (V == 4) *reinterpret_cast<float4*>(dz + base + offs[q]) = make_float4(o[q][0], o[q][1], o[q][2], o[q][3]);
            else
#pragma unroll
                for (int k = 0; k < V; ++k) dz[base + offs[q] + k] = o[q][k];
        }
    }
}

// VALID pooling of an odd size with the skip gradient added in place (add == dz) under the LeakyReLU' mask: the last row
// and / or column lies in no window, so the kernel above never visits it - its gradient is add * lrelu'(yact).
__global__ void maxpool2_bwd_border_kernel(const float* __restrict__ yact, float* __restrict__ dz, int n, int h, int w, int c,
                                           float alpha) {
    const long rowpart = (h & 1) ? (long)w * c : 0;                 // the last row, every column
    const long colpart = (w & 1) ? (long)(h & ~1) * c : 0;          // the last column of the rows that are in a window
    const long per = rowpart + colpart, total = (long)n * per;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long im = i / per, r = i % per;
        long o;
        if (r < rowpart) {
            o = ((im * h + (h - 1)) * w) * c + r;
        } else {
            const long q = r - rowpart;
            o = ((im * h + q / c) * w + (w - 1)) * c + q % c;
        }
        dz[o] *= yact[o] > 0.f ? 1.0f : alpha;
    }
}

}  // namespace

extern "C" {

int nimg_maxpool2_fwd(const float* x, float* y, int n, int h, int w, int c, void* stream) {
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    if (!x || !y || n < 0 || h < 2 || w < 2 || c <= 0) return NIMG_ERR_ARG;      /* odd sizes: VALID (the last row / column is dropped) */
    if (n == 0) return NIMG_OK;
    hipStream_t s = (hipStream_t)stream;
    if (c % 4 == 0)
        hipLaunchKernelGGL(maxpool2_fwd_kernel<4>, dim3(grid_for((long)n * (h / 2) * (w / 2) * (c / 4))), dim3(256),
                           0, s, x, y, n, h, w, c);
    else
        hipLaunchKernelGGL(maxpool2_fwd_kernel<1>, dim3(grid_for((long)n * (h / 2) * (w / 2) * c)), dim3(256), 0, s,
                           x, y, n, h, w, c);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_maxpool2_bwd(const float* dp, const float* yact, const float* add, float* dz, int n, int h, int w, int c,
                      int apply_lrelu_mask, float alpha, void* stream) {
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    if (!dp || !yact || !dz || n < 0 || h < 2 || w < 2 || c <= 0) return NIMG_ERR_ARG;
    if (n == 0) return NIMG_OK;
    hipStream_t s = (hipStream_t)stream;
    if ((h & 1) || (w & 1)) {            /* VALID pooling of an odd size: the dropped last row / column gets no gradient */
        if (add && add != dz) return NIMG_ERR_ARG;
        if (!add && hipMemsetAsync(dz, 0, (size_t)n * h * w * c * sizeof(float), s) != hipSuccess) return NIMG_ERR_LAUNCH;
        if (add && apply_lrelu_mask) {   /* in place: the dropped elements hold add and still owe the LeakyReLU' factor */
            const long border = (long)n * (((h & 1) ? (long)w * c : 0) + ((w & 1) ? (long)(h & ~1) * c : 0));
            hipLaunchKernelGGL(maxpool2_bwd_border_kernel, dim3(grid_for(border)), dim3(256), 0, s, yact, dz, n, h, w, c, alpha);
            NIMG_CHECK_LAUNCH();
        }
    }
    if (c % 4 == 0)
        hipLaunchKernelGGL(maxpool2_bwd_kernel<4>, dim3(grid_for((long)n * (h / 2) * (w / 2) * (c / 4))), dim3(256),
                           0, s, dp, yact, add, dz, n, h, w, c, apply_lrelu_mask, alpha);
    else
        hipLaunchKernelGGL(maxpool2_bwd_kernel<1>, dim3(grid_for((long)n * (h / 2) * (w / 2) * c)), dim3(256), 0, s,
                           dp, yact, add, dz, n, h, w, c, apply_lrelu_mask, alpha);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

/* MaxPool2D(2) forward / backward on bf16-stored NHWC tensors (even h, w; c % 8 == 0): see nimg_maxpool2_fwd / _bwd */
int nimg_maxpool2_fwd_bf16(const void* x, void* y, int n, int h, int w, int c, void* stream) {
    if (n == 0) return NIMG_OK;
    if (!x || !y || n < 0 || h < 2 || w < 2 || c <= 0 || (h & 1) || (w & 1) || (c & 7)) return NIMG_ERR_ARG;
    hipLaunchKernelGGL(maxpool2_fwd_bf16_kernel, dim3(grid_for((long)n * (h / 2) * (w / 2) * (c / 8))), dim3(256), 0,
                       (hipStream_t)stream, (const __bf16*)x, (__bf16*)y, n, h, w, c);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_maxpool2_bwd_bf16(const void* dp, const void* yact, const void* add, void* dz, int n, int h, int w, int c,
                           int apply_lrelu_mask, float alpha, void* stream) {
    if (n == 0) return NIMG_OK;
    if (!dp || !yact || !dz || n < 0 || h < 2 || w < 2 || c <= 0 || (h & 1) || (w & 1) || (c & 7)) return NIMG_ERR_ARG;
    hipLaunchKernelGGL(maxpool2_bwd_bf16_kernel, dim3(grid_for((long)n * (h / 2) * (w / 2) * (c / 8))), dim3(256), 0,
                       (hipStream_t)stream, (const __bf16*)dp, (const __bf16*)yact, (const __bf16*)add, (__bf16*)dz, n, h, w, c,
                       apply_lrelu_mask, alpha);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_maxpool2_unpool(const float* dp, const unsigned char* idx, const float* pooled, float* dz, int n, int ho, int wo,
                         int c, int apply_lrelu_mask, float alpha, void* stream) {
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    if (!dp || !idx || !dz || n < 0 || ho <= 0 || wo <= 0 || c <= 0 || (c & 3)) return NIMG_ERR_ARG;
    if (apply_lrelu_mask && !pooled) return NIMG_ERR_ARG;
    if (n == 0) return NIMG_OK;
    return nimg_maxpool2_unpool_ex(dp, idx, pooled, dz, n, ho, wo, c, apply_lrelu_mask, alpha, 0, stream);
}

int nimg_maxpool2_unpool_ex(const float* dp, const unsigned char* idx, const float* pooled, float* dz, int n, int ho,
                            int wo, int c, int apply_lrelu_mask, float alpha, int flags, void* stream) {
    if (n == 0) return NIMG_OK;
    if (!dp || !idx || !dz || n < 0 || ho <= 0 || wo <= 0 || c <= 0 || (c & 3)) return NIMG_ERR_ARG;
    if (apply_lrelu_mask && !pooled) return NIMG_ERR_ARG;
    const dim3 grid(grid_for((long)n * ho * wo * (c / 4)));
    hipStream_t s = (hipStream_t)stream;
    if ((flags & NIMG_BF16_IN) && (flags & NIMG_BF16_OUT) && !apply_lrelu_mask && (c & 7) == 0) {
        hipLaunchKernelGGL(maxpool2_unpool_bf16x8_kernel, dim3(grid_for((long)n * ho * wo * (c / 8))), dim3(256), 0, s,
                           (const uint4*)dp, (const uint2*)idx, (uint4*)dz, n, ho, wo, c / 8);
        NIMG_CHECK_LAUNCH();
        return NIMG_OK;
    }
#define NIMG_UNPOOL(A_, B_) hipLaunchKernelGGL((maxpool2_unpool_kernel<A_, B_>), grid, dim3(256), 0, s, dp, idx, pooled, dz, \
                                               n, ho, wo, c, apply_lrelu_mask, alpha)
    if (flags & NIMG_BF16_IN) { if (flags & NIMG_BF16_OUT) NIMG_UNPOOL(true, true); else NIMG_UNPOOL(true, false); }
    else { if (flags & NIMG_BF16_OUT) NIMG_UNPOOL(false, true); else NIMG_UNPOOL(false, false); }
#undef NIMG_UNPOOL
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

}  // extern "C"
