// Throughput mode of the convolutions: bf16 operands on the CDNA4 matrix cores (v_mfma_f32_32x32x16_bf16, 16x the f32
// MFMA rate), float32 accumulation, float32 master weights and float32 activations in HBM (converted to bf16 while the
// tiles are staged into LDS).  Same im2col-free implicit GEMM as conv_mfma.hip / conv_wgrad.hip; judged on PSNR /
// accuracy parity, not on the 1e-4 contract (that is the f32 mode).
//
//   forward / input gradient: A tile [pixel][16 ci] bf16 (32 B per pixel, one ds_read_b128 per fragment, 1-bit XOR
//       swizzle of the two 16-byte halves => conflict-free), B tile [tap][co][16 ci] bf16 read the same way from weights
//       that nimg_conv_weights_bf16 lays out once per step as [ci chunk][tap][co][16].
//
// The kernels are compiled apart from this file, which took five minutes as one unit: the forward / input-gradient templates
// in conv_bf16_tile.h / _ring.h / _dma.h (shared pieces: conv_bf16.h), one conv_bf16_k*.hip per kernel size and input storage;
// the weight gradient in conv_bf16_wgrad.hip; the few-channel kernels of the FAN front end in conv_bf16_packed.hip.
// Here: the weight-image converters and the forward entry points.
#include "conv_bf16.h"

namespace {

// wb[chunk][tap'][co][16] (mode 0, forward) = w[tap][ci = 16*chunk + k][co];  mode 1 (input gradient): roles of ci/co
// swap and the taps are flipped.  Chunk-major, so the weight tile a workgroup stages per 16-channel K chunk is one
// contiguous 2 KiB run per tap (fully coalesced 16-byte loads).  Padding channels are zero.
__global__ void weights_bf16_kernel(const float* __restrict__ w, __bf16* __restrict__ wb, int taps, int cin, int cout,
                                    int mode) {
    const int rows = mode == 0 ? cout : cin, cols = mode == 0 ? cin : cout;
    const int cpad = (cols + 15) / 16 * 16;
    const long total = (long)taps * rows * cpad;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % 16) + 16 * (int)(i / (16L * rows * taps)), r = (int)((i / 16) % rows);
        const int t = (int)((i / (16L * rows)) % taps);
        float v = 0.f;
        if (c < cols) v = mode == 0 ? w[((long)t * cin + c) * cout + r] : w[((long)(taps - 1 - t) * cin + r) * cout + c];
        wb[i] = (__bf16)v;
    }
}

// All bf16 weight images of a model in ONE launch (blockIdx.y = table entry): the per-layer launches were 54 kernels of
// ~5 us per training step.  Table entry = 4 x int64: {w pointer, wb pointer, (taps << 32) | mode, (cin << 32) | cout}.
__global__ __launch_bounds__(256) void weights_bf16_batch_kernel(const long long* __restrict__ table) {
    const long long* e = table + 4 * blockIdx.y;
    const float* w = reinterpret_cast<const float*>(e[0]);
    __bf16* wb = reinterpret_cast<__bf16*>(e[1]);
    const int taps = (int)(e[2] >> 32), mode = (int)(e[2] & 0xffffffffll);
    const int cin = (int)(e[3] >> 32), cout = (int)(e[3] & 0xffffffffll);
    const int rows = mode == 0 ? cout : cin, cols = mode == 0 ? cin : cout;
    const int chunks = (cols + 15) / 16, rblocks = (rows + 63) / 64;
    const int ntiles = chunks * taps * rblocks;            // tile = one (chunk, tap) x 64 rows x 16 columns
    __shared__ float tile[16][65];
    const int tid = threadIdx.x;
    for (int tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int rb = tl % rblocks, ct = tl / rblocks, t = ct % taps, chunk = ct / taps;
        const int r0 = rb * 64, c0 = chunk * 16;
        __syncthreads();
        if (mode == 0) {       // w[(t*cin + c)*cout + r]: r is the contiguous axis -> 16 rows of 64 floats, transposed via LDS
            const int cl = tid >> 4, rq = (tid & 15) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c0 + cl, r = r0 + rq + k;
                tile[cl][rq + k] = (c < cols && r < rows) ? w[((long)t * cin + c) * cout + r] : 0.f;
            }
        } else {               // w[((taps-1-t)*cin + r)*cout + c]: c is contiguous
            const int rl = tid >> 2, cq = (tid & 3) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c0 + cq + k, r = r0 + rl;
                tile[cq + k][rl] = (c < cols && r < rows) ? w[((long)(taps - 1 - t) * cin + r) * cout + c] : 0.f;
            }
        }
        __syncthreads();
        const int rl = tid >> 2, kq = (tid & 3) * 4;
        if (r0 + rl < rows) {
            bf16x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (__bf16)tile[kq + k][rl];
            *reinterpret_cast<bf16x4*>(wb + ((long)ct * rows + r0 + rl) * 16 + kq) = o;
        }
    }
}

template <int KS, int STRIDE>
int dispatch_b(const ConvParamsB& p, hipStream_t s) {
    if constexpr (STRIDE == 1) {          // bf16-stored inputs: the stride-1 layers (FAN, UNet) ...
        if (p.flags & NIMG_BF16_IN) return conv_bf16_dispatch<KS, STRIDE, true>(p, s);
    } else if constexpr (KS == 2) {       // ... and for the 2x2 / stride-2 form (input gradient of the UNet's Conv2DTranspose)
        if (p.flags & NIMG_BF16_IN) return conv_bf16_dispatch<KS, STRIDE, true>(p, s);
    } else {
        if (p.flags & NIMG_BF16_IN) return NIMG_ERR_ARG;
    }
    return conv_bf16_dispatch<KS, STRIDE, false>(p, s);
}

}  // namespace

extern "C" {

size_t nimg_conv_weights_bf16_bytes(int ks_h, int ks_w, int cin, int cout, int mode) {
    const long rows = mode == 0 ? cout : cin, cols = mode == 0 ? cin : cout;
    return (size_t)ks_h * ks_w * rows * ((cols + 15) / 16 * 16) * 2;
}

int nimg_conv_weights_bf16(const float* w, void* wb, int ks_h, int ks_w, int cin, int cout, int mode, void* stream) {
    if (!w || !wb || ks_h <= 0 || ks_w <= 0 || cin <= 0 || cout <= 0 || mode < 0 || mode > 1) return NIMG_ERR_ARG;
    const long total = (long)nimg_conv_weights_bf16_bytes(ks_h, ks_w, cin, cout, mode) / 2;
    const int grid = (int)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
    hipLaunchKernelGGL(weights_bf16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, (__bf16*)wb,
                       ks_h * ks_w, cin, cout, mode);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_conv_weights_bf16_batch(const void* table, int n_entries, void* stream) {
    if (n_entries == 0) return NIMG_OK;
    if (!table || n_entries < 0) return NIMG_ERR_ARG;
    // 384 workgroups per entry: the launch lasts as long as its largest entry (512 x 512 x 9: 2304 tiles -> 6 per workgroup;
    // with 96 it was 24 serial tiles = 36 of the launch's 40 us at the head of every step)
    hipLaunchKernelGGL(weights_bf16_batch_kernel, dim3(384, (unsigned)n_entries), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)table);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

static int conv2d_fwd_bf16_impl(const float* in1, int c1, const float* in2, int c2, const void* wb, const float* bias,
                         float* out1, int o1, float* out2, int o2, const float* act_mask, int n, int h, int wd,
                         int ks, int stride, int pad_t, int pad_l, int pad_mode, int hout, int wout, int act,
                         float alpha, int flags, void* stream, const unsigned char* in_idx = nullptr,
                         const float* res = nullptr, void* out1b = nullptr, float* pool_out = nullptr,
                         unsigned char* pool_idx = nullptr, const unsigned char* act_sign = nullptr) {
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    if (!in1 || !wb || !out1 || c1 <= 0 || c2 < 0 || o1 <= 0 || o2 < 0 || n < 0 || h <= 0 || wd <= 0) return NIMG_ERR_ARG;
    if ((c2 > 0 && !in2) || (o2 > 0 && !out2) || hout <= 0 || wout <= 0 || pad_t < 0 || pad_l < 0) return NIMG_ERR_ARG;
    if (act < 0 || act > 1 || pad_mode < 0 || pad_mode > 2) return NIMG_ERR_ARG;
    if (c2 == 0 ? ((c1 % 4) || ((flags & NIMG_BF16_IN) && (c1 % 8))) : ((c1 % 8) || (c2 % 8)))
        return NIMG_ERR_ARG;                           // 8-channel staging granules (a single float32 input may end on 4)
    if (n == 0) return NIMG_OK;
    ConvParamsB p;
    p.in1 = in1; p.in2 = in2; p.wb = (const __bf16*)wb; p.bias = bias; p.out1 = out1; p.out2 = out2; p.act1 = act_mask;
    p.pool_out = pool_out; p.pool_idx = pool_idx; p.convt = 0; p.flags = flags; p.in_idx = in_idx; p.res = res;
    p.out1b = (float*)out1b;
    if (((flags & NIMG_POOL_ALSO) != 0) != (pool_out != nullptr)) return NIMG_ERR_ARG;
    if (res && (ks != 3 || stride != 1)) return NIMG_ERR_ARG;
    if ((res || out1b) && (o2 != 0 || (o1 & 3))) return NIMG_ERR_ARG;
    if (out1b && (flags & NIMG_BF16_OUT)) return NIMG_ERR_ARG;
    if ((flags & NIMG_COPY_LRELU) && (!out1b || act != 0)) return NIMG_ERR_ARG;
    if (in_idx && (!(flags & NIMG_BF16_IN) || stride != 1 || ks != 5 || (h & 1) || (wd & 1) || pad_mode != 0)) return NIMG_ERR_ARG;
    if ((flags & (NIMG_BF16_OUT | NIMG_BF16_MASK)) && ((o1 & 3) || (o2 & 3))) return NIMG_ERR_ARG;   // vector epilogue only
    if ((flags & NIMG_BF16_MASK) && o2 != 0) return NIMG_ERR_ARG;
    // the sign plane stands for a bf16 mask of a bf16 output in 8-channel groups; the mask itself stays required
    if (act_sign && (!act_mask || !(flags & NIMG_BF16_MASK) || !(flags & NIMG_BF16_OUT) || (o1 & 7) || o2 != 0)) return NIMG_ERR_ARG;
    p.act_sign = act_sign;
    if ((flags & NIMG_D2S_OUT) && (ks != 3 || stride != 1 || o2 != 0 || (o1 & 15) || in_idx)) return NIMG_ERR_ARG;
    if ((flags & NIMG_S2D_OUT) && (ks != 3 || stride != 1 || o2 != 0 || (o1 & 3) || in_idx || (hout & 1) || (wout & 1) ||
                                   (flags & NIMG_D2S_OUT)))
        return NIMG_ERR_ARG;
    p.C1 = c1; p.C2 = c2; p.O1 = o1; p.O2 = o2; p.CinP = (c1 + c2 + 15) / 16 * 16;
    p.N = n; p.H = h; p.W = wd; p.Hout = hout; p.Wout = wout; p.pad_t = pad_t; p.pad_l = pad_l;
    p.tiles_y = p.tiles_x = 0; p.act = act; p.pad_mode = pad_mode; p.alpha = alpha;
    hipStream_t s = (hipStream_t)stream;
    if (stride == 1 && ks == 1) return dispatch_b<1, 1>(p, s);
    if (stride == 1 && ks == 3) return dispatch_b<3, 1>(p, s);
    if (stride == 1 && ks == 5) return dispatch_b<5, 1>(p, s);
    if (stride == 2 && ks == 2) return dispatch_b<2, 2>(p, s);
    if (stride == 2 && ks == 5) return dispatch_b<5, 2>(p, s);
    return NIMG_ERR_ARG;
}

int nimg_conv2d_fwd_bf16(const float* in1, int c1, const float* in2, int c2, const void* wb, const float* bias,
                         float* out1, int o1, float* out2, int o2, const float* act_mask, int n, int h, int wd,
                         int ks, int stride, int pad_t, int pad_l, int pad_mode, int hout, int wout, int act,
                         float alpha, void* stream) {
    return conv2d_fwd_bf16_impl(in1, c1, in2, c2, wb, bias, out1, o1, out2, o2, act_mask, n, h, wd, ks, stride, pad_t, pad_l,
                                pad_mode, hout, wout, act, alpha, 0, stream);
}

int nimg_conv2d_fwd_bf16_ex(const float* in1, int c1, const float* in2, int c2, const void* wb, const float* bias,
                            float* out1, int o1, float* out2, int o2, const float* act_mask, int n, int h, int wd,
                            int ks, int stride, int pad_t, int pad_l, int pad_mode, int hout, int wout, int act,
                            float alpha, int flags, void* stream) {
    return conv2d_fwd_bf16_impl(in1, c1, in2, c2, wb, bias, out1, o1, out2, o2, act_mask, n, h, wd, ks, stride, pad_t, pad_l,
                                pad_mode, hout, wout, act, alpha, flags, stream);
}

/* A SAME stride-1 3x3 convolution (+ bias + activation) that stores BOTH its output and the 2x2 max-pooled output, bf16 in
 * and out: the UNet's second encoder convolutions (models/pipelines.py:160-173 - the full tensor is the skip connection, the
 * pooled one the next level's input).  cin % 8 == 0, cout % 8 == 0, even h / wd > 8 (the 16x16-pixel tiles); pool_idx optional. */
int nimg_conv2d_fwd_pool_also_bf16(const float* in, int cin, const void* wb, const float* bias, float* out, float* pool_out,
                                   unsigned char* pool_idx, int cout, int n, int h, int wd, int act, float alpha, void* stream) {
#ifdef NIMG_NO_EPI8
    return NIMG_ERR_ARG;           /* A/B build without the 8-wide epilogue: the NIMG_POOL_ALSO branch lives there (ops probes with n = 0) */
#endif
    if (n == 0) return NIMG_OK;
    if (!pool_out || (h & 1) || (wd & 1) || h <= 8 || wd <= 8 || (cout & 7) || (cin & 7)) return NIMG_ERR_ARG;
    return conv2d_fwd_bf16_impl(in, cin, nullptr, 0, wb, bias, out, cout, nullptr, 0, nullptr, n, h, wd, 3, 1, 1, 1, 0, h, wd, act,
                                alpha, NIMG_BF16_IN | NIMG_BF16_OUT | NIMG_POOL_ALSO, stream, nullptr, nullptr, nullptr, pool_out,
                                pool_idx);
}

/* The input gradient of the first convolution of a UNet encoder level, written THROUGH the 2x2 max-pool in front of it
 * (models/pipelines.py:160-173 backward): dz (bf16, n x cin... see include/nimg.h). */
int nimg_conv2d_dgrad_unpool_out_bf16(const float* dz, int c1, const void* wb, const float* act, const float* skip, float* out,
                                      int cout, int n, int h, int wd, int apply_mask, float alpha, void* stream) {
#ifdef NIMG_NO_EPI8
    return NIMG_ERR_ARG;           /* A/B build without the 8-wide epilogue: the NIMG_UNPOOL_OUT branch lives there (ops probes with n = 0) */
#endif
    if (n == 0) return NIMG_OK;
    if (!dz || !wb || !act || !out || (c1 & 7) || (cout & 7) || h <= 0 || wd <= 0) return NIMG_ERR_ARG;
    if ((long)n * 4 * h * wd * cout * 2 >= (1l << 40)) return NIMG_ERR_ARG;
    ConvParamsB p;
    p.in1 = dz; p.in2 = nullptr; p.wb = (const __bf16*)wb; p.bias = nullptr; p.out1 = out; p.out2 = nullptr; p.act1 = act;
    p.pool_out = nullptr; p.pool_idx = nullptr; p.convt = 0; p.flags = NIMG_BF16_IN | NIMG_BF16_OUT | NIMG_BF16_MASK | NIMG_UNPOOL_OUT;
    p.in_idx = nullptr; p.res = skip; p.out1b = nullptr;
    p.C1 = c1; p.C2 = 0; p.O1 = cout; p.O2 = 0; p.CinP = (c1 + 15) / 16 * 16;
    p.N = n; p.H = h; p.W = wd; p.Hout = h; p.Wout = wd; p.pad_t = p.pad_l = 1;
    p.tiles_y = p.tiles_x = 0; p.act = apply_mask ? 1 : 0; p.pad_mode = 0; p.alpha = alpha;
    return dispatch_b<3, 1>(p, (hipStream_t)stream);
}

/* nimg_conv2d_fwd_bf16_ex for the layers of a residual block (models/compression.py:224-227, 240-243): `residual` (float32, the
 * shape of out1, optional) is added to the result after bias, activation and mask - net + conv(a) forward, d_net + mask * dgrad
 * backward, one pass - and `out_bf16_copy` (optional) receives the same result rounded to bf16 next to the float32 out1: the
 * residual stream keeps its exact float32 sum, its consumers read the bf16 copy (flag NIMG_COPY_LRELU: the copy holds
 * LeakyReLU(alpha) of the result - the codec feeds its first block the activation of the tensor it skips around,
 * models/compression.py:224).  At least one of the two; one float32 output with o1 % 4 == 0, the residual with 3x3 / stride 1
 * layers only (else NIMG_ERR_ARG). */
int nimg_conv2d_fwd_bf16_res(const float* in1, int c1, const void* wb, const float* bias, float* out1, int o1,
                             const float* act_mask, const float* residual, void* out_bf16_copy, int n, int h, int wd, int ks,
                             int stride, int pad_t, int pad_l, int pad_mode, int hout, int wout, int act, float alpha, int flags,
                             void* stream) {
    if (!residual && !out_bf16_copy) return NIMG_ERR_ARG;
    return conv2d_fwd_bf16_impl(in1, c1, nullptr, 0, wb, bias, out1, o1, nullptr, 0, act_mask, n, h, wd, ks, stride, pad_t, pad_l,
                                pad_mode, hout, wout, act, alpha, flags, stream, nullptr, residual, out_bf16_copy);
}

/* The same convolution on the 2x2 UN-POOLING of a pooled bf16 tensor: in_pooled (n, h/2, wd/2, c1) bf16 + in_idx arg-max bytes
 * stand for the (n, h, wd, c1) tensor that holds in_pooled[y/2][x/2][c] where in_idx[y/2][x/2][c] == 2 (y & 1) + (x & 1) and zero
 * elsewhere (the gradient MaxPool2D hands back).  Used as the input-gradient pass of the FAN's fused conv + pool layers: the
 * full-resolution gradient never exists in HBM.  5x5, stride 1, zero padding, c1 % 16 == 0, cout % 32 == 0 (else NIMG_ERR_ARG:
 * un-pool explicitly with nimg_maxpool2_unpool_ex and call nimg_conv2d_fwd_bf16_ex). */
int nimg_conv2d_fwd_bf16_unpool(const void* in_pooled, const unsigned char* in_idx, int c1, const void* wb, const float* bias,
                                float* out1, int o1, const float* act_mask, int n, int h, int wd, int ks, int pad_t, int pad_l,
                                int hout, int wout, int act, float alpha, int flags, void* stream) {
    return nimg_conv2d_fwd_bf16_unpool_sign(in_pooled, in_idx, c1, wb, bias, out1, o1, act_mask, nullptr, n, h, wd, ks, pad_t, pad_l,
                                            hout, wout, act, alpha, flags, stream);
}

/* ... with the sign plane of act_mask next to it (see include/nimg.h): the ring kernels read the plane, every other route the mask */
int nimg_conv2d_fwd_bf16_unpool_sign(const void* in_pooled, const unsigned char* in_idx, int c1, const void* wb, const float* bias,
                                     float* out1, int o1, const float* act_mask, const unsigned char* act_sign, int n, int h, int wd,
                                     int ks, int pad_t, int pad_l, int hout, int wout, int act, float alpha, int flags,
                                     void* stream) {
    if (!in_idx) return NIMG_ERR_ARG;
    return conv2d_fwd_bf16_impl((const float*)in_pooled, c1, nullptr, 0, wb, bias, out1, o1, nullptr, 0, act_mask, n, h, wd, ks, 1,
                                pad_t, pad_l, 0, hout, wout, act, alpha, flags | NIMG_BF16_IN, stream, in_idx, nullptr, nullptr,
                                nullptr, nullptr, act_sign);
}

/* Conv2DTranspose(cout, 2x2, stride 2) forward (pipelines.py:205) on the matrix core: four 1x1 products, one per output
 * phase (dy, dx), in a single launch.  wb = nimg_conv_weights_bf16(w, 2, 2, cin'=cout, cout'=cin, mode 1) of the Keras
 * kernel (2,2,Cout,Cin).  x (n,h,wd,cin) -> y (n,2h,2wd,cout). */
int nimg_convt2x2_fwd_bf16(const float* x, const void* wb, const float* bias, float* y, int n, int h, int wd, int cin,
                           int cout, void* stream) {
    return nimg_convt2x2_fwd_bf16_ex(x, wb, bias, y, n, h, wd, cin, cout, 0, stream);
}

/* flags: NIMG_BF16_IN = x is stored as bf16, NIMG_BF16_OUT = y is stored as bf16 (cout % 4 == 0) */
int nimg_convt2x2_fwd_bf16_ex(const float* x, const void* wb, const float* bias, float* y, int n, int h, int wd, int cin,
                              int cout, int flags, void* stream) {
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    if (!x || !wb || !y || n < 0 || h <= 0 || wd <= 0 || cin <= 0 || cout <= 0 || (cin % 8)) return NIMG_ERR_ARG;
    if ((flags & ~(NIMG_BF16_IN | NIMG_BF16_OUT)) || ((flags & NIMG_BF16_OUT) && (cout & 3))) return NIMG_ERR_ARG;
    ConvParamsB p;
    p.in1 = x; p.in2 = nullptr; p.wb = (const __bf16*)wb; p.bias = bias; p.out1 = y; p.out2 = nullptr; p.act1 = nullptr;
    p.pool_out = nullptr; p.pool_idx = nullptr; p.convt = 1; p.flags = flags; p.in_idx = nullptr; p.res = nullptr; p.out1b = nullptr;
    p.C1 = cin; p.C2 = 0; p.O1 = cout; p.O2 = 0; p.CinP = (cin + 15) / 16 * 16;
    p.N = n; p.H = h; p.W = wd; p.Hout = h; p.Wout = wd; p.pad_t = 0; p.pad_l = 0;
    p.tiles_y = p.tiles_x = 0; p.act = 0; p.pad_mode = 0; p.alpha = 0.f;
#ifndef NIMG_NO_EPI8
    // bf16-stored output, cout % 8 == 0 (the UNet's four layers): ONE 1x1 product with N = 4 cout columns - the input tile is
    // staged once for the four output phases instead of once per phase, a quarter of the workgroups pay prologue and epilogue -
    // and the phase is a pixel offset of the 16-byte store (NIMG_D2S_CONVT).  Same products in the same order: bit-identical.
    static const bool no_fat = getenv("NIMG_NO_CONVT_FAT") != nullptr;
    if (!no_fat && (flags & NIMG_BF16_OUT) && (cout & 7) == 0) {
        p.convt = 0; p.O1 = 4 * cout; p.flags = flags | NIMG_D2S_CONVT;
    }
#endif
    return dispatch_b<1, 1>(p, (hipStream_t)stream);
}

}  // extern "C"
