// HBM-bound element-wise kernels of the imaging channel (gfx950): one output element (or float4) per thread and step.
// float4 along the NHWC channel axis wherever C % 4 == 0, grid-stride loops capped at 2048 workgroups (common.h grid_for).
//
//   Conv2DTranspose 2x2 s2 fwd                            models/pipelines.py:205
//   depth_to_space (DCR) + straight-through clip fwd/bwd  models/pipelines.py:218-223, models/compression.py:248-271
//   LeakyReLU backward, add, add_n, integer and float fills
// Pooling is in pool.hip, the losses in losses.hip, the FAN head in head.hip, Adam in adam.hip.
#include "common.h"

namespace {

using namespace nimg;

// ---------------------------------------------------------------------------------------------------------------
// Conv2DTranspose(k=2,s=2): out[n,2y+i,2x+j,co] = sum_ci in[n,y,x,ci] * w[i,j,co,ci] + b[co]
// One workgroup: 16 input pixels x 64 output channels x the 4 taps, Cin streamed through LDS in chunks of 32.
__global__ __launch_bounds__(256) void convt2x2_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ y,
                                                           long npix, int h, int wd, int cin, int cout) {
    __shared__ float sx[16][33];
    __shared__ float sw[4][64][33];
    const int tid = threadIdx.x;
    const int cot = (cout + 63) / 64;
    const int co0 = (blockIdx.x % cot) * 64;
    const long p0 = (long)(blockIdx.x / cot) * 16;
    const int co = tid & 63, pg = tid >> 6;          // thread: channel co, pixels pg*4..pg*4+3, all 4 taps
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    for (int c0 = 0; c0 < cin; c0 += 32) {
        __syncthreads();
        for (int it = tid; it < 16 * 32; it += 256) {
            const int pp = it / 32, k = it % 32;
            sx[pp][k] = (p0 + pp < npix && c0 + k < cin) ? x[(p0 + pp) * cin + c0 + k] : 0.f;
        }
        for (int it = tid; it < 4 * 64 * 32; it += 256) {
            const int k = it % 32, oc = (it / 32) % 64, t = it / (32 * 64);
            sw[t][oc][k] = (co0 + oc < cout && c0 + k < cin) ? w[((long)t * cout + co0 + oc) * cin + c0 + k] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < 32; ++k) {
            float xv[4], wv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) xv[a] = sx[pg * 4 + a][k];
#pragma unroll
            for (int t = 0; t < 4; ++t) wv[t] = sw[t][co][k];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[a][t] = fmaf(xv[a], wv[t], acc[a][t]);
        }
    }
    if (co0 + co >= cout) return;
    const float bv = bias ? bias[co0 + co] : 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long pp = p0 + pg * 4 + a;
        if (pp >= npix) continue;
        const int xx = (int)(pp % wd);
        const long rest = pp / wd;
        const int yy = (int)(rest % h);
        const long im = rest / h;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            y[(((im * 2 * h) + 2 * yy + (t >> 1)) * (2L * wd) + 2 * xx + (t & 1)) * cout + co0 + co] = acc[a][t] + bv;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// depth_to_space(DCR, block 2) with optional affine + straight-through clip: y = clip(scale*d2s(x)+shift, 0, 1)
__global__ void d2s_clip_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int h, int w, int co,
                                    float scale, float shift, int clip) {
    const long total = (long)n * h * w * 4 * co;        // output elements
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % co);
        long r = i / co;
        const int X = (int)(r % (2 * w));
        r /= 2 * w;
        const int Y = (int)(r % (2 * h)), im = (int)(r / (2 * h));
        const float v = x[(((long)im * h + (Y >> 1)) * w + (X >> 1)) * (4 * co) + ((Y & 1) * 2 + (X & 1)) * co + c];
        float o = scale * v + shift;
        if (clip) o = fminf(fmaxf(o, 0.f), 1.f);
        y[i] = o;
    }
}
// co == 3 (every NIP of the reference ends in depth_to_space of 12 channels): one thread per INPUT pixel - its 12 floats are
// three 16-byte loads, and they land as two runs of 6 contiguous floats (output rows 2y and 2y + 1, pixels 2x and 2x + 1):
// 8-byte stores.  The per-element form above spends its time on 64-bit divisions and 4-byte accesses (2.5 TB/s).
__global__ void d2s_clip3_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long npix, int h, int w, float scale,
                                     float shift, int clip) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long)gridDim.x * blockDim.x) {
        const int xx = (int)(i % w);
        const long r = i / w;
        const int yy = (int)(r % h);
        const long im = r / h;
        const float4* src = reinterpret_cast<const float4*>(x + i * 12);
        const float4 a = src[0], b = src[1], c = src[2];
        float v[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            float o = scale * v[k] + shift;
            if (clip) o = fminf(fmaxf(o, 0.f), 1.f);
            v[k] = o;
        }
        float2* top = reinterpret_cast<float2*>(y + ((im * 2 * h + 2 * yy) * (2L * w) + 2 * xx) * 3);
        float2* bot = reinterpret_cast<float2*>(y + ((im * 2 * h + 2 * yy + 1) * (2L * w) + 2 * xx) * 3);
        top[0] = make_float2(v[0], v[1]); top[1] = make_float2(v[2], v[3]); top[2] = make_float2(v[4], v[5]);
        bot[0] = make_float2(v[6], v[7]); bot[1] = make_float2(v[8], v[9]); bot[2] = make_float2(v[10], v[11]);
    }
}
__global__ void d2s_clip3_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, long npix, int h, int w, float scale) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long)gridDim.x * blockDim.x) {
        const int xx = (int)(i % w);
        const long r = i / w;
        const int yy = (int)(r % h);
        const long im = r / h;
        const float2* top = reinterpret_cast<const float2*>(dy + ((im * 2 * h + 2 * yy) * (2L * w) + 2 * xx) * 3);
        const float2* bot = reinterpret_cast<const float2*>(dy + ((im * 2 * h + 2 * yy + 1) * (2L * w) + 2 * xx) * 3);
        const float2 t0 = top[0], t1 = top[1], t2 = top[2], b0 = bot[0], b1 = bot[1], b2 = bot[2];
        float4* dst = reinterpret_cast<float4*>(dx + i * 12);
        dst[0] = make_float4(scale * t0.x, scale * t0.y, scale * t1.x, scale * t1.y);
        dst[1] = make_float4(scale * t2.x, scale * t2.y, scale * b0.x, scale * b0.y);
        dst[2] = make_float4(scale * b1.x, scale * b1.y, scale * b2.x, scale * b2.y);
    }
}
// The 32-bit loops below advance an unsigned index by up to 2048 * 256 per trip: a float4 count within one grid stride of 2^32
// would wrap to a value below total4 and never end, so the dispatch keeps them a whole stride away from 2^32.
constexpr long D2S_CLIP4_STRIDE = 2048L * 256;
// co % 4 == 0 (the codec's 128- and 64-channel layers, models/compression.py:233,245): 16-byte granules never straddle a
// channel block, 32-bit index arithmetic - the per-element forms run at 1.5 TB/s on their 64-bit divisions.
// Forward: one thread per OUTPUT granule (stores coalesced; loads are runs of co floats).  Backward: per INPUT-gradient granule.
__global__ void d2s_clip4_fwd_kernel(const float4* __restrict__ x, float4* __restrict__ y, unsigned total4, unsigned h, unsigned w,
                                     unsigned c4, float scale, float shift, int clip) {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += gridDim.x * blockDim.x) {
        const unsigned c = i % c4;
        unsigned r = i / c4;
        const unsigned X = r % (2 * w);
        r /= 2 * w;
        const unsigned Y = r % (2 * h), im = r / (2 * h);
        const float4 v = x[((im * h + (Y >> 1)) * w + (X >> 1)) * (4 * c4) + ((Y & 1) * 2 + (X & 1)) * c4 + c];
        float4 o = make_float4(scale * v.x + shift, scale * v.y + shift, scale * v.z + shift, scale * v.w + shift);
        if (clip) {
            o.x = fminf(fmaxf(o.x, 0.f), 1.f); o.y = fminf(fmaxf(o.y, 0.f), 1.f);
            o.z = fminf(fmaxf(o.z, 0.f), 1.f); o.w = fminf(fmaxf(o.w, 0.f), 1.f);
        }
        y[i] = o;
    }
}
__global__ void d2s_clip4_bwd_kernel(const float4* __restrict__ dy, float4* __restrict__ dx, unsigned total4, unsigned h,
                                     unsigned w, unsigned c4, float scale) {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += gridDim.x * blockDim.x) {
        const unsigned ch = i % (4 * c4);
        unsigned r = i / (4 * c4);
        const unsigned xx = r % w;
        r /= w;
        const unsigned yy = r % h, im = r / h;
        const unsigned blk = ch / c4, c = ch - blk * c4;
        const float4 v = dy[((im * 2 * h + 2 * yy + (blk >> 1)) * (2 * w) + 2 * xx + (blk & 1)) * c4 + c];
        dx[i] = make_float4(scale * v.x, scale * v.y, scale * v.z, scale * v.w);
    }
}
// gradient: straight-through (identity through the clip), dx = scale * space_to_depth(dy)
__global__ void d2s_clip_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int n, int h, int w,
                                    int co, float scale) {
    const long total = (long)n * h * w * 4 * co;        // input elements
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int ch = (int)(i % (4 * co));
        long r = i / (4 * co);
        const int xx = (int)(r % w);
        r /= w;
        const int yy = (int)(r % h), im = (int)(r / h);
        const int blk = ch / co, c = ch % co;
        dx[i] = scale * dy[(((long)im * 2 * h + 2 * yy + (blk >> 1)) * (2L * w) + 2 * xx + (blk & 1)) * co + c];
    }
}

// dz = dy * lrelu'(y)
__global__ void lrelu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ yact, float* dz, long count,
                                 float alpha) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long)gridDim.x * blockDim.x)
        dz[i] = dy[i] * (yact[i] > 0.f ? 1.0f : alpha);
}

// out = a + b (residual adds; out may alias a)
__global__ void add_kernel(const float* a, const float* __restrict__ b, float* out, long count) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long)gridDim.x * blockDim.x)
        out[i] = a[i] + b[i];
}

// out = a0 + a1 + ... (2..6 float32 tensors, 16-byte accesses; out may alias any input): the manipulation gradients of the
// channel are summed onto the native branch in ONE pass instead of one add launch each
__global__ void add_n_kernel(const float4* a0, const float4* a1, const float4* a2, const float4* a3, const float4* a4,
                             const float4* a5, float4* out, long count4) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < count4; i += (long)gridDim.x * blockDim.x) {
        float4 s = a0[i];
        const float4 b = a1[i];
        s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
        if (a2) { const float4 c = a2[i]; s.x += c.x; s.y += c.y; s.z += c.z; s.w += c.w; }
        if (a3) { const float4 c = a3[i]; s.x += c.x; s.y += c.y; s.z += c.z; s.w += c.w; }
        if (a4) { const float4 c = a4[i]; s.x += c.x; s.y += c.y; s.z += c.z; s.w += c.w; }
        if (a5) { const float4 c = a5[i]; s.x += c.x; s.y += c.y; s.z += c.z; s.w += c.w; }
        out[i] = s;
    }
}

__global__ void int_words_kernel(int* __restrict__ dst, const int* __restrict__ src, long n, int value, int mode) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        dst[i] = mode == 0 ? value : max(dst[i], src[i]);
}
__global__ void float_fill_kernel(float* __restrict__ dst, long n, float value) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dst[i] = value;
}

}  // namespace

extern "C" {

int nimg_convt2x2_fwd(const float* x, const float* w, const float* bias, float* y, int n, int h, int wd, int cin,
                      int cout, void* stream) {
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    if (!x || !w || !y || n < 0 || h <= 0 || wd <= 0 || cin <= 0 || cout <= 0) return NIMG_ERR_ARG;
    if (n == 0) return NIMG_OK;
    const long npix = (long)n * h * wd;
    const long blocks = ((npix + 15) / 16) * ((cout + 63) / 64);
    hipLaunchKernelGGL(convt2x2_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, w, bias, y,
                       npix, h, wd, cin, cout);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_d2s_clip_fwd(const float* x, float* y, int n, int h, int w, int cout, float scale, float shift, int clip,
                      void* stream) {
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    if (!x || !y || n < 0 || h <= 0 || w <= 0 || cout <= 0) return NIMG_ERR_ARG;
    if (n == 0) return NIMG_OK;
    if (cout == 3) {
        hipLaunchKernelGGL(d2s_clip3_fwd_kernel, dim3(grid_for((long)n * h * w)), dim3(256), 0, (hipStream_t)stream, x, y,
                           (long)n * h * w, h, w, scale, shift, clip);
        NIMG_CHECK_LAUNCH();
        return NIMG_OK;
    }
    if ((cout & 3) == 0 && (long)n * h * w * cout < (1L << 32) - D2S_CLIP4_STRIDE) {
        hipLaunchKernelGGL(d2s_clip4_fwd_kernel, dim3(grid_for((long)n * h * w * cout)), dim3(256), 0, (hipStream_t)stream,
                           (const float4*)x, (float4*)y, (unsigned)((long)n * h * w * cout), (unsigned)h, (unsigned)w,
                           (unsigned)(cout >> 2), scale, shift, clip);
        NIMG_CHECK_LAUNCH();
        return NIMG_OK;
    }
    hipLaunchKernelGGL(d2s_clip_fwd_kernel, dim3(grid_for((long)n * h * w * 4 * cout)), dim3(256), 0,
                       (hipStream_t)stream, x, y, n, h, w, cout, scale, shift, clip);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_d2s_clip_bwd(const float* dy, float* dx, int n, int h, int w, int cout, float scale, void* stream) {
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    if (!dy || !dx || n < 0 || h <= 0 || w <= 0 || cout <= 0) return NIMG_ERR_ARG;
    if (n == 0) return NIMG_OK;
    if (cout == 3) {
        hipLaunchKernelGGL(d2s_clip3_bwd_kernel, dim3(grid_for((long)n * h * w)), dim3(256), 0, (hipStream_t)stream, dy, dx,
                           (long)n * h * w, h, w, scale);
        NIMG_CHECK_LAUNCH();
        return NIMG_OK;
    }
    if ((cout & 3) == 0 && (long)n * h * w * cout < (1L << 32) - D2S_CLIP4_STRIDE) {
        hipLaunchKernelGGL(d2s_clip4_bwd_kernel, dim3(grid_for((long)n * h * w * cout)), dim3(256), 0, (hipStream_t)stream,
                           (const float4*)dy, (float4*)dx, (unsigned)((long)n * h * w * cout), (unsigned)h, (unsigned)w,
                           (unsigned)(cout >> 2), scale);
        NIMG_CHECK_LAUNCH();
        return NIMG_OK;
    }
    hipLaunchKernelGGL(d2s_clip_bwd_kernel, dim3(grid_for((long)n * h * w * 4 * cout)), dim3(256), 0,
                       (hipStream_t)stream, dy, dx, n, h, w, cout, scale);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_lrelu_bwd(const float* dy, const float* yact, float* dz, long count, float alpha, void* stream) {
    if (count == 0) return NIMG_OK;        /* empty stream: nothing to do (its buffers may be null) */
    if (!dy || !yact || !dz || count < 0) return NIMG_ERR_ARG;
    hipLaunchKernelGGL(lrelu_bwd_kernel, dim3(grid_for(count)), dim3(256), 0, (hipStream_t)stream, dy, yact, dz,
                       count, alpha);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_add(const float* a, const float* b, float* out, long count, void* stream) {
    if (count == 0) return NIMG_OK;        /* empty stream: nothing to do (its buffers may be null) */
    if (!a || !b || !out || count < 0) return NIMG_ERR_ARG;
    hipLaunchKernelGGL(add_kernel, dim3(grid_for(count)), dim3(256), 0, (hipStream_t)stream, a, b, out, count);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_add_n(const float* const* inputs, int n_inputs, float* out, long count, void* stream) {
    if (count == 0) return NIMG_OK;        /* empty stream: nothing to do (its buffers may be null) */
    if (!inputs || !out || n_inputs < 2 || n_inputs > 6 || count < 0 || (count & 3)) return NIMG_ERR_ARG;
    const float4* a[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < n_inputs; ++i) {
        if (!inputs[i]) return NIMG_ERR_ARG;
        a[i] = reinterpret_cast<const float4*>(inputs[i]);
    }
    hipLaunchKernelGGL(add_n_kernel, dim3(grid_for(count / 4)), dim3(256), 0, (hipStream_t)stream, a[0], a[1], a[2], a[3], a[4],
                       a[5], reinterpret_cast<float4*>(out), count / 4);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

/* The step's flag / scalar bookkeeping as kernels of this library (no framework-native launch inside a training step):
 * mode 0: dst[0 .. n) = value;  mode 1: dst[i] = max(dst[i], src[i]) (the workflow's "NaN seen since the last check" word) */
int nimg_int_words(int* dst, const int* src, long n, int value, int mode, void* stream) {
    if (n == 0) return NIMG_OK;        /* empty stream: nothing to do (its buffers may be null) */
    if (!dst || n < 0 || mode < 0 || mode > 1 || (mode == 1 && !src)) return NIMG_ERR_ARG;
    hipLaunchKernelGGL(int_words_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, dst, src, n, value, mode);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_float_fill(float* dst, long n, float value, void* stream) {
    if (n == 0) return NIMG_OK;        /* empty stream: nothing to do (its buffers may be null) */
    if (!dst || n < 0) return NIMG_ERR_ARG;
    hipLaunchKernelGGL(float_fill_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, dst, n, value);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

}  // extern "C"
