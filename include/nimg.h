/*
 * nimg.h - C ABI of libnimg.so: MI355X (gfx950) HIP kernels for the neural-imaging channel hot path
 *          RAW -> UNet ISP -> manipulations -> differentiable JPEG -> FAN classifier, forward + backward.
 *
 * The reference (pkorus/neural-imaging, TF 2.1, pure Python) has NO FFI: its seam is the Python duck type
 * TFModel (models/tfmodel.py:86-294).  This header is the native boundary underneath the build's Python mirror of
 * that surface (neural-imaging_amd/models/ *.py): every entry point replaces one TensorFlow op call site of the
 * reference, cited per function.  INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions (all entry points):
 *   - plain C types only; every buffer is a CALLER-ALLOCATED DEVICE pointer (no hidden hipMalloc)
 *   - tensors are NHWC float32 unless stated; weights in the Keras layouts the reference's checkpoints use:
 *     Conv2D (kh,kw,Cin,Cout), Conv2DTranspose (kh,kw,Cout,Cin), Dense (in,out)
 *   - asynchronous on `stream` (a hipStream_t passed as void*), no internal synchronisation, capturable in a hipGraph
 *   - returns NIMG_OK (0) or a negative NIMG_ERR_* code; never throws, never exits
 *   - re-entrant: no mutable global state (Q tables etc. are passed per call)
 */
#ifndef NIMG_H
#define NIMG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NIMG_OK 0
#define NIMG_ERR_ARG (-1)     /* invalid shape / null pointer / unsupported configuration */
#define NIMG_ERR_LAUNCH (-2)  /* HIP launch failure (hipGetLastError) */
#define NIMG_ERR_WORKSPACE (-3) /* workspace too small */

/* tensor-storage flags of the *_ex throughput-mode entry points: the named tensor holds bf16 instead of float32 */
#define NIMG_BF16_IN 1    /* in1 AND in2 (convolutions: c1 % 8 == 0, c2 % 8 == 0) / dp (un-pool) */
#define NIMG_BF16_OUT 2   /* out1 AND out2 (o1 % 4 == 0, o2 % 4 == 0) / pool_out / dz of the un-pool */
#define NIMG_BF16_MASK 4  /* act_mask */
#define NIMG_BF16_DZ 8    /* dz of a weight gradient (cout % 8 == 0) */
#define NIMG_D2S_OUT 16   /* 3x3 stride-1 convolutions (o1 % 16 == 0, no out2): out1 - and the act_mask / residual / bf16 copy that
                           * share its indexing - is the depth_to_space(2) image (n, 2 hout, 2 wout, o1 / 4) of the result, the
                           * tf.nn.depth_to_space layout (block 2 dy + dx of pixel (y, x) -> pixel (2y + dy, 2x + dx)):
                           * models/compression.py:233,245,249 forward, and the input gradient of a stride-2 layer computed
                           * over its space-to-depth image (nimg_s2d_conv_weights) */
#define NIMG_MASK_CONV 128 /* with NIMG_D2S_OUT: act_mask keeps the convolution's own (n, hout, wout, o1) layout (the activation it masks
                            * by was itself stored as a space-to-depth image) instead of the depth-to-space layout of out1 */
#define NIMG_COPY_LRELU 64 /* nimg_conv2d_fwd_bf16_res: the bf16 copy holds LeakyReLU(alpha) of the (activation-free) result */
#define NIMG_S2D_OUT 32   /* 3x3 stride-1 convolutions (o1 % 4 == 0, even hout / wout, no out2): out1 (and the bf16 copy) is the
                           * space_to_depth(2) image (n, hout / 2, wout / 2, 4 o1) of the result - the gradient of a depth_to_space
                           * layer, written by the input-gradient pass that produces it (models/compression.py:233,245 backward);
                           * act_mask and residual keep the convolution's own (n, hout, wout, o1) layout */
#define NIMG_UNPOOL_OUT 512 /* internal to nimg_conv2d_dgrad_unpool_out_bf16: the result is routed through a 2x2 max-pool's backward */
#define NIMG_D2S_CONVT 1024 /* internal to nimg_convt2x2_fwd_bf16_ex: the transposed convolution as ONE 1x1 product with 4 cout columns, phase
                              3 - b = channel block b written to pixel (2 y + dy, 2 x + dx); the bias repeats per block */
#define NIMG_POOL_ALSO 256 /* internal to nimg_conv2d_fwd_pool_also_bf16: the pooled tensor is written next to out1, not instead of it */

/* library / ABI version, bumped on any change of an existing entry point's signature or data layout (3: nimg_conv2d_fwd_bf16_res
 * gained out_bf16_copy and stride; 5: the arg-max of nimg_conv1_pool_fwd_c4 / nimg_conv1_wgrad_c4 / nimg_conv1_dgrad_pooled is 2 bits
 * per value; 6: the nimg_l3ic_* bitstream entry points; 7: the nimg_jpeg_* baseline codec entry points; 8: the per-item
 * nimg_jpeg_*_items forms and nimg_msssim; version 8 also carries the later, purely added nimg_jpeg_decode* and
 * nimg_jpeg_reconstruct_tables entry points, the nimg_jpeg_histogram / _optimal_tables / _encode_tables ones and
 * nimg_jpeg_transform_tables / nimg_jpeg_tables_from_float, and the nimg_jpeg_*_restart ones).  A binding compares nimg_abi_version()
 * with the NIMG_ABI_VERSION it was written against. */
#define NIMG_ABI_VERSION 8
int nimg_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------------
 * Differentiable JPEG - replaces DifferentiableJPEG.call, models/jpeg.py:91-159, and the Quantization layer it uses,
 * models/layers.py:118-134.  One fused kernel per direction (the reference runs ~25 TF ops).
 * rounding modes = Quantization.rounding (models/layers.py:97): */
#define NIMG_ROUND_ROUND 0    /* tf.round, no gradient            (layers.py:122-123) */
#define NIMG_ROUND_SOFT 1     /* fwd round, bwd 1-cos(2 pi x)     (layers.py:126-128)  <- dJPEG default 'soft' */
#define NIMG_ROUND_SIN 2      /* x - sin(2 pi x)/(2 pi)           (layers.py:125)     */
#define NIMG_ROUND_HARMONIC 3 /* x - sin(2 pi x)/pi (taylor_terms=1; layers.py:130-134) */
#define NIMG_ROUND_IDENTITY 4 /* layers.py:136-137 */

/* x,y: (n,h,w,3) in [0,1]; h,w multiples of 8.   qtab: (3,8,8) float32 tables for Y,Cb,Cr (device).
 * mask (optional, may be NULL): (n,h,w) uint8, bit c set <=> channel c was NOT clipped (needed by the backward).
 * idx  (optional): (n,3,h/8,w/8,8,8) int16  rint(X/Q) quantisation indices - the bit-exact sub-contract.
 * xdq  (optional): same shape float32, dequantised coefficients = 2nd output of the reference model (jpeg.py:159). */
int nimg_djpeg_fwd(const float* x, float* y, const float* qtab, uint8_t* mask, int16_t* idx, float* xdq,
                   int n, int h, int w, int rounding, void* stream);
/* gx = d loss / d x given gy = d loss / d y.  Recomputes the forward DCT from x (no saved coefficients). */
int nimg_djpeg_bwd(const float* x, const float* gy, const uint8_t* mask, const float* qtab, float* gx,
                   int n, int h, int w, int rounding, void* stream);
/* The same backward pass plus the gradient of TRAINABLE quantisation tables (DifferentiableJPEG(trainable=True),
 * models/jpeg.py:57-62 add_weight('Q_mtx_luma' / 'Q_mtx_chroma'); gradient through X / Q ... * Q at :129-131):
 * dq (2,8,8) float32 = [d loss / d Q_luma, d loss / d Q_chroma (Cb + Cr)], (+)= when accumulate.  Deterministic: per-wave
 * partial sums in `workspace` (nimg_djpeg_dq_workspace_bytes), fixed-order reduction. */
size_t nimg_djpeg_dq_workspace_bytes(int n, int h, int w);
int nimg_djpeg_bwd_dq(const float* x, const float* gy, const uint8_t* mask, const float* qtab, float* gx, float* dq,
                      int n, int h, int w, int rounding, int accumulate, void* workspace, size_t workspace_bytes,
                      void* stream);
/* Differentiable JPEG with chroma sub-sampling (csrc/djpeg_sub.hip): (hs, vs) = (2, 1) is 4:2:2, (2, 2) is 4:2:0;
 * h % (8 vs) == 0 and w % (8 hs) == 0 (whole MCUs).  Any other factors - (1, 1) included: 4:4:4 stays with the entry points above -
 * or a ragged image are NIMG_ERR_ARG.  The operator: colour as above; Cb / Cr = the mean of each hs x vs group (libjpeg's h2v1 /
 * h2v2 without the bias); the 8x8 block path of nimg_djpeg_fwd on Y at (h, w) and on Cb / Cr at (h / vs, w / hs); chroma up-sampled
 * by libjpeg's triangle filter in float (out[2i] = 3/4 in[i] + 1/4 in[i-1], out[2i+1] = 3/4 in[i] + 1/4 in[i+1], the edge sample
 * beyond the component, down the columns then along the rows at 4:2:0); + 127, inverse colour, / 255, clip.
 * x, y, qtab, mask (optional): as nimg_djpeg_fwd.  idx (optional, int16) / xdq (optional, float32): ONE buffer each, per image
 * [Y blocks (h/8, w/8) | Cb blocks | Cr blocks (h/(8 vs), w/(8 hs))], every block [8][8] in natural order.
 * workspace: nimg_djpeg_sub_workspace_bytes(n, h, w, hs, vs, with_dq) device bytes, 16-byte aligned (0 for an empty or refused
 * shape) - the reduced chroma planes (forward: reconstructed, backward: gradients) and, with_dq, the per-wave table-gradient sums;
 * with_dq = 0 serves the forward and a backward with dq == NULL.  A shorter one is NIMG_ERR_WORKSPACE.  Two launches per direction
 * on `stream` (plus the reduction with dq), asynchronous, capturable, no allocation.  n == 0 is a no-op. */
size_t nimg_djpeg_sub_workspace_bytes(int n, int h, int w, int hs, int vs, int with_dq);
int nimg_djpeg_sub_fwd(const float* x, float* y, const float* qtab, uint8_t* mask, int16_t* idx, float* xdq,
                       int n, int h, int w, int hs, int vs, int rounding, void* workspace, size_t workspace_bytes,
                       void* stream);
/* gx = d loss / d x of nimg_djpeg_sub_fwd given gy and the forward's mask; recomputes the forward DCTs from x.  dq (may be NULL):
 * (2,8,8) float32 = [d loss / d Q_luma, d loss / d Q_chroma (Cb + Cr)], (+)= when accumulate - deterministic, the contract of
 * nimg_djpeg_bwd_dq (per-wave partial sums in the workspace, fixed-order reduction; always the IEEE division). */
int nimg_djpeg_sub_bwd(const float* x, const float* gy, const uint8_t* mask, const float* qtab, float* gx,
                       float* dq /* may be NULL */, int n, int h, int w, int hs, int vs, int rounding, int accumulate,
                       void* workspace, size_t workspace_bytes, void* stream);
/* Rate term of the 4:4:4 differentiable JPEG (csrc/djpeg_entropy.hip): the soft entropy the DCN trains against
 * (helpers/tf_helpers.py:290-333), of the quantiser's OUTPUT e = quantise<rounding>(z), z = X / Q exactly as nimg_djpeg_fwd forms it
 * (same float32 order, same division: with the modes that round, its idx output is e).  Code book: the 512 integers -255 .. 256
 * (Quantization(latent_bpf=9), models/jpeg.py:89), v = 50, gamma = 25, eps = 1e-72; one pooled histogram of the N = 3 n h w values;
 * weights, histogram, 1e-9 clip, re-normalisation and / 0.6931 in float64.  entropy: ONE float32 on the device (bits per value).
 * The transform is recomputed from x; nothing of size N x 512 exists.  Values inside [-255.5, 256.5] see the five centres around
 * the nearest one (every other centre weighs < 2e-33 of it), values outside all 512.
 * workspace: nimg_djpeg_entropy_workspace_bytes(n, h, w) device bytes, 16-byte aligned (0 for an empty or refused shape); a shorter
 * one is NIMG_ERR_WORKSPACE.  _fwd leaves dH / d mean_k there for _bwd - the first 512 float64 of the workspace, centre -255 first,
 * exactly 0 where the 1e-9 clip is active: the workspace must stay untouched between the two (several _bwd calls may follow one
 * _fwd).  h % 8, w % 8, a null pointer, a rounding mode out of range: NIMG_ERR_ARG.  The workgroups'
 * partial histograms are summed in a fixed order; inside a workgroup the float64 LDS atomics arrive in any order, so two runs agree
 * to the last bits of float64, not bit for bit.  Asynchronous on `stream`, capturable, no allocation, no synchronisation; n == 0 is
 * a no-op. */
size_t nimg_djpeg_entropy_workspace_bytes(int n, int h, int w);
int nimg_djpeg_entropy_fwd(const float* x, const float* qtab, int n, int h, int w, int rounding, float* entropy,
                           void* workspace, size_t workspace_bytes, void* stream);
/* gx (+)= coef * d entropy / d x, plain autograd of the expression above: d H / d e from the estimator in float64, d e / d z the
 * mode's backward surrogate as nimg_djpeg_bwd applies it (1 - cos(2 pi z) for SOFT and SIN, none for ROUND), d z / d X = 1 / Q, back
 * through the DCT, the colour matrix and the 255.  dq (may be NULL): (2,8,8) float32 (+)= coef * [d H / d Q_luma, d H / d Q_chroma
 * (Cb + Cr)] through d z / d Q = -z / Q - the layout and the fixed-order reduction of nimg_djpeg_bwd_dq; with dq the IEEE division.
 * With SOFT the estimator is evaluated at integers, where its derivative vanishes: gx is ~1e-29. */
int nimg_djpeg_entropy_bwd(const float* x, const float* qtab, int n, int h, int w, int rounding, float coef, float* gx,
                           int accumulate_gx, float* dq /* 128 floats or NULL */, int accumulate_dq, void* workspace,
                           size_t workspace_bytes, void* stream);
/* IJG quality scaling - replaces jpeg_qtable, compression/jpeg_helpers.py:264-305.  HOST function: out64 is a host
 * pointer to 64 floats (row-major 8x8).  channel 0 = luma, >0 = chroma. */
int nimg_jpeg_qtable(int quality, int channel, float* out64);

/* ------------------------------------------------------------------------------------------------------------------
 * Convolutions on the matrix cores (float32 MFMA, exact f32).  Replace tf.keras.layers.Conv2D / tf.nn.conv2d call sites:
 *   UNet  models/pipelines.py:191-192,207-208,216 ; FAN models/forensics.py:69,76 ; ConstrainedConv2D models/layers.py:56-57
 *   TwitterDCN models/compression.py:221-237,247-265.
 * in1/in2: the input may be split over two NHWC tensors with c1 + c2 channels (concat-free skip connections,
 *          pipelines.py:206,211); in2 = NULL, c2 = 0 otherwise.   w: (ks,ks,c1+c2,o1+o2) HWIO.   bias: (o1+o2) or NULL.
 * out1/out2: the output may be split the same way (o2 = 0 normally; used by the dgrad of a concat input).
 * act_mask (optional): tensor shaped like out1; out1 is multiplied by LeakyReLU'(act_mask) - fuses the previous
 *          layer's activation derivative into an input-gradient pass.
 * pad_mode: 0 zeros, 1 SYMMETRIC, 2 REFLECT (tf.pad modes folded into the tile load).  act: 0 none, 1 LeakyReLU(alpha).
 * Supported (ks,stride): (1,1) (3,1) (5,1) (2,2) (5,2).  hout/wout/pad_t/pad_l are explicit so TF's asymmetric SAME
 * padding is the caller's choice.  Input gradients = this same entry point on nimg_conv_flip_weights output. */
int nimg_conv2d_fwd(const float* in1, int c1, const float* in2, int c2, const float* w, const float* bias,
                    float* out1, int o1, float* out2, int o2, const float* act_mask, int n, int h, int wd, int ks,
                    int stride, int pad_t, int pad_l, int pad_mode, int hout, int wout, int act, float alpha,
                    void* stream);
/* wt[ks*ks-1-t][co][ci] = w[t][ci][co]: spatially flipped, channel-transposed weights for the input-gradient pass */
int nimg_conv_flip_weights(const float* w, float* wt, int ks_h, int ks_w, int cin, int cout, void* stream);
/* dw (ks,ks,c1+c2,cout) (+)= sum over pixels of in (x) dz - the weight half of tape.gradient (pipelines.py:84-88,
 * forensics.py:118-124, workflows/manipulation_classification.py:280).  Deterministic split-K through `workspace`.
 * db (optional, may be NULL): (cout) bias gradient = column sums of dz, fused into the same pass. */
size_t nimg_conv2d_wgrad_workspace_bytes(int cin, int cout, int ks_h, int ks_w, int n, int hout, int wout);
int nimg_conv2d_wgrad(const float* in1, int c1, const float* in2, int c2, const float* dz, int cout, float* dw,
                      float* db, int n, int h, int wd, int ks, int stride, int pad_t, int pad_l, int pad_mode, int hout,
                      int wout, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* db (cout) (+)= sum over npix pixels of dz (npix, cout) */
size_t nimg_bias_grad_workspace_bytes(long npix, int cout);
int nimg_bias_grad(const float* dz, float* db, long npix, int cout, int accumulate, void* workspace,
                   size_t workspace_bytes, void* stream);
/* flags: NIMG_BF16_DZ = dz is stored as bf16 (cout % 4 == 0, cout / 4 divides 256); sums in float32 */
int nimg_bias_grad_ex(const float* dz, float* db, long npix, int cout, int accumulate, void* workspace,
                      size_t workspace_bytes, int flags, void* stream);
/* Conv2DTranspose(k=2,s=2,SAME), kernel (2,2,cout,cin) - models/pipelines.py:205.  Its input gradient is
 * nimg_conv2d_fwd(ks=2,stride=2) on the same kernel, its weight gradient nimg_conv2d_wgrad(ks=2,stride=2) with the
 * roles of input and output gradient swapped (see neural-imaging_amd/models/pipelines.py). */
int nimg_convt2x2_fwd(const float* x, const float* w, const float* bias, float* y, int n, int h, int wd, int cin,
                      int cout, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Pooling / layout / element-wise */
/* MaxPool2D 2x2 (pipelines.py:197 SAME, forensics.py:70 VALID; identical on even sizes).  Odd sizes follow VALID: y is
 * (n, h/2, w/2, c) with the last row / column dropped, and the backward pass leaves it a zero gradient. */
int nimg_maxpool2_fwd(const float* x, float* y, int n, int h, int w, int c, void* stream);
/* dz = (route dp to the FIRST arg-max of each window) [+ add] [* LeakyReLU'(yact)]; add may alias dz.  At an odd h or w add must
 * be null or dz itself (NIMG_ERR_ARG otherwise): the dropped row / column then holds 0, or add [* LeakyReLU'(yact)]. */
int nimg_maxpool2_bwd(const float* dp, const float* yact, const float* add, float* dz, int n, int h, int w, int c,
                      int apply_lrelu_mask, float alpha, void* stream);
/* The same two passes on bf16-stored tensors (UNet activations / gradients in throughput mode: pipelines.py:197 and its
 * gradient); h, w even, c % 8 == 0; every tensor argument is bf16.  Rounding is monotonic, so pooling the rounded tensor
 * equals rounding the pooled one. */
int nimg_maxpool2_fwd_bf16(const void* x, void* y, int n, int h, int w, int c, void* stream);
int nimg_maxpool2_bwd_bf16(const void* dp, const void* yact, const void* add, void* dz, int n, int h, int w, int c,
                           int apply_lrelu_mask, float alpha, void* stream);
/* Fused Conv2D(SAME, stride 1) -> [LeakyReLU] -> MaxPool2D(2) of the FAN feature extractor (models/forensics.py:69-77:
 * every conv{i} is followed by its pool; the full-resolution activation is consumed by nothing else), float32 MFMA.
 * pool_out (n,h/2,w/2,cout) receives the pooled activation, pool_idx (same shape, bytes; may be NULL for inference)
 * the position 0..3 of the first maximum inside each window (row-major).  h, w even; cout % 4 == 0; ks 3|5. */
int nimg_conv2d_pool_fwd(const float* in, int cin, const float* w, const float* bias, float* pool_out,
                         unsigned char* pool_idx, int cout, int n, int h, int wd, int ks, int act, float alpha,
                         void* stream);
/* The same pass with bf16 MFMA operands (throughput mode): w = the f32 kernel (read when cin <= 4), wb = its
 * nimg_conv_weights_bf16(mode 0) image (read otherwise; cin % 8 == 0). */
int nimg_conv2d_pool_fwd_bf16(const float* in, int cin, const float* w, const void* wb, const float* bias,
                              float* pool_out, unsigned char* pool_idx, int cout, int n, int h, int wd, int ks, int act,
                              float alpha, void* stream);
/* Backward of that epilogue: dz (n,2ho,2wo,c) = dp routed to the stored arg-max [* LeakyReLU'(pooled)], zero elsewhere
 * (sign(window max) == sign(pooled), so the un-stored activation is not needed).  c % 4 == 0. */
int nimg_maxpool2_unpool(const float* dp, const unsigned char* idx, const float* pooled, float* dz, int n, int ho, int wo,
                         int c, int apply_lrelu_mask, float alpha, void* stream);
/* y = [clip01](scale * depth_to_space_DCR(x, 2) + shift); x (n,h,w,4*cout) -> y (n,2h,2w,cout).
 * pipelines.py:218-223 (scale 1, shift 0, clip 1), compression.py:248,263,266-271.  The clip is straight-through:
 * the backward is dx = scale * space_to_depth(dy). */
int nimg_d2s_clip_fwd(const float* x, float* y, int n, int h, int w, int cout, float scale, float shift, int clip,
                      void* stream);
int nimg_d2s_clip_bwd(const float* dy, float* dx, int n, int h, int w, int cout, float scale, void* stream);
int nimg_lrelu_bwd(const float* dy, const float* yact, float* dz, long count, float alpha, void* stream);
int nimg_add(const float* a, const float* b, float* out, long count, void* stream);
/* out = sum of 2..6 float32 tensors of `count` elements (count % 4 == 0; `inputs` is a HOST array of device pointers; out may
 * alias an input): the per-manipulation gradients of workflows/manipulation_classification.py:199-208 summed in one pass. */
int nimg_add_n(const float* const* inputs, int n_inputs, float* out, long count, void* stream);
/* avg_pool downsampling of the channel, workflows/manipulation_classification.py:235 */
int nimg_avgpool_fwd(const float* x, float* y, int n, int h, int w, int c, int factor, void* stream);
int nimg_avgpool_bwd(const float* dy, float* dx, int n, int h, int w, int c, int factor, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Losses, classifier head, optimiser */
/* helpers/tf_helpers.py:31-32  loss = mean((255a - 255b)^2); grad_a (+)= grad_scale * dloss/da (grad_a may be NULL) */
size_t nimg_mse255_workspace_bytes(void);
int nimg_mse255(const float* a, const float* b, float* loss, float* grad_a, long count, float grad_scale,
                int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* helpers/tf_helpers.py:35-36  loss = mean |255a - 255b|; grad_a (+)= grad_scale * 255 sign(a - b) / count (NIP --loss L1) */
size_t nimg_mae255_workspace_bytes(void);
int nimg_mae255(const float* a, const float* b, float* loss, float* grad_a, long count, float grad_scale,
                int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* helpers/tf_helpers.py:39-40  loss = mean_n 255 (1 - tf.image.ssim(y, t, max_val)_n)  (NIP --loss SSIM); y, t (n,h,w,c),
 * h, w >= 11; gauss_win = the 121 window weights (device); grad_y (may be NULL) (+)= grad_scale * dloss/dy. */
size_t nimg_ssim_loss_workspace_bytes(int n, int h, int w, int c, int with_grad);
int nimg_ssim_loss(const float* y, const float* t, float* loss, float* grad_y, int n, int h, int w, int c,
                   float max_val, const float* gauss_win, float grad_scale, int accumulate, void* workspace,
                   size_t workspace_bytes, void* stream);
/* SSIM per image (mean over channels and VALID window positions), a/b (n,h,w,c) in [0,max_val], out (n).
 *   mode 0 = skimage.metrics.structural_similarity(multichannel=True, data_range=max_val) as helpers/metrics.py:9-25 uses
 *            it (7x7 uniform window, sample covariance);   mode 1 = tf.image.ssim(max_val) as models/compression.py:89
 *            uses it (11x11 Gaussian window sigma 1.5 passed by the caller in gauss_win[121], population moments). */
/* The workflow's hand-over to the UNet backward in one pass (workflows/manipulation_classification.py:265-283 under the tape:
 * d loss / d Y = the manipulations' input gradients + lambda_nip * d mse255(Y, target) / d Y, then the gradient of
 * depth_to_space + clip, models/pipelines.py:203-205): dz (n,h,w,12) = space_to_depth of [parts[0] + ... + parts[n_parts-1] +
 * grad_scale * d mse255(y, target) / d y] with parts / y / target (n,2h,2w,3), 1 <= n_parts <= 6; loss (1) = mse255(y, target).
 * Same additions in the same order as nimg_add_n -> nimg_mse255(accumulate) -> nimg_d2s_clip_bwd(scale 1): same bits.
 * workspace: nimg_mse255_workspace_bytes(). */
int nimg_mse255_sum_s2d3(const float* const* parts, int n_parts, const float* y, const float* target, float* loss, float* dz,
                         int n, int h, int w, float grad_scale, void* workspace, size_t workspace_bytes, void* stream);
size_t nimg_ssim_workspace_bytes(int n);
int nimg_ssim(const float* a, const float* b, float* out, int n, int h, int w, int c, int mode, float max_val,
              const float* gauss_win, void* workspace, size_t workspace_bytes, void* stream);
/* FAN head, models/forensics.py:80-94: GAP -> Dense(k, softmax) -> SparseCategoricalCrossentropy on probabilities
 * (Keras eager semantics: clip to [1e-7, 1-1e-7], renormalise).  act (n,hw,c) is the 1x1-conv output AFTER LeakyReLU.
 * labels may be NULL (inference: only gap/probs are written).  loss_scale = 1/batch (mean reduction).  k <= 256 classes (the
 * reference's own bound, models/forensics.py:37): one lane sums up to 16 classes, from 17 on the wave's lanes own the classes. */
int nimg_fan_head_fwd(const float* act, const float* w, const float* b, const int* labels, float* gap, float* probs,
                      float* loss_per, float* dlogits, int n, int hw, int c, int k, float loss_scale, void* stream);
/* dact = gradient wrt the 1x1 conv PRE-activation (LeakyReLU' fused), dw (c,k), db (k), loss (1) */
int nimg_fan_head_bwd(const float* act, const float* gap, const float* w, const float* dlogits,
                      const float* loss_per, float* dact, float* dw, float* db, float* loss, int n, int hw, int c,
                      int k, float loss_scale, float alpha, void* stream);
/* tf.keras.optimizers.Adam over a flat buffer: theta -= lr*sqrt(1-b2^t)/(1-b1^t) * m/(sqrt(v)+eps); g is pre-scaled
 * by grad_scale (e.g. 1/world_size after a sum all-reduce).  step is the 1-based iteration count.  skip_flag (optional
 * device int): when non-zero the update is skipped - the device-side form of the NaN guard at workflows/...:281-283. */
int nimg_adam_step(float* params, const float* grads, float* m, float* v, long count, float lr, float beta1,
                   float beta2, float eps, int step, float grad_scale, const int* skip_flag, void* stream);
/* The same update with the bias-corrected rate lr*sqrt(1-b2^t)/(1-b1^t) read from DEVICE memory (one float): the form a
 * captured hipGraph replays - the host refreshes *lr_t before every replay, the launch itself never changes. */
int nimg_adam_step_dev(float* params, const float* grads, float* m, float* v, long count, const float* lr_t, float beta1,
                       float beta2, float eps, float grad_scale, const int* skip_flag, void* stream);
/* The same update (lr_t != NULL: the rate from device memory, lr and step unused; else from lr and step on the host) which, in
 * the same launch, writes both bf16 images of every 4-D weight from the updated values: image_table is the table of
 * nimg_conv_weights_bf16_batch with its entries in pairs - 2j = the mode-0, 2j + 1 = the mode-1 image of weight j - and the
 * weights inside [params, params + count), ascending and apart (the caller's duty: the table is device memory).  params, m, v and
 * the images get the bytes that nimg_adam_step[_dev] followed by nimg_conv_weights_bf16_batch give; a set skip_flag writes
 * nothing at all.
 * cc_kernel (optional): one of the table's weights, a ConstrainedConv2D kernel (cc_ks, cc_ks, cc_channels, cc_channels) of at
 * most 4096 values.  The workgroup that updates it also writes cc_nf = nimg_constrained_kernel_fwd(updated kernel, cc_strength)
 * and, where cc_nft is given, cc_nft = nimg_conv_flip_weights(cc_nf), both byte for byte.  A kernel that is not in the table
 * with these dimensions is updated like any other value and neither is written.
 * Purely added: NIMG_ABI_VERSION stays. */
int nimg_adam_step_images(float* params, const float* grads, float* m, float* v, long count, float lr, const float* lr_t,
                          float beta1, float beta2, float eps, int step, float grad_scale, const int* skip_flag,
                          const void* image_table, int n_entries, const float* cc_kernel, float* cc_nf, float* cc_nft,
                          int cc_ks, int cc_channels, float cc_strength, void* stream);
/* flag[0] |= 1 if any gradient is NaN (device-side version of workflows/manipulation_classification.py:281-282) */
int nimg_nan_flag(const float* g, long count, int* flag, void* stream);
/* flag / scalar bookkeeping of a training step on the library's own kernels: mode 0 dst[0 .. n) = value, mode 1 dst[i] =
 * max(dst[i], src[i]) (the "NaN seen since the last check" word);  nimg_float_fill: dst[0 .. n) = value (a captured step's
 * device-resident learning rate) */
int nimg_int_words(int* dst, const int* src, long n, int value, int mode, void* stream);
int nimg_float_fill(float* dst, long n, float value, void* stream);

/* In-kernel finish of the split-K weight-gradient sums (throughput-mode kernels: nimg_conv2d_wgrad_bf16*, nimg_conv1_wgrad_*,
 * nimg_conv_wgrad_c3k5 ...; replaces the separate fixed-order reduction launch behind tape.gradient(loss, weights),
 * workflows/manipulation_classification.py:280).  The workgroups that contribute to one tile of dw share arrival counters and
 * the last to arrive sums the tile's slabs in a fixed order (deterministic).  The counters are the CALLER's memory: bind `bytes`
 * (a multiple of 4, >= NIMG_TICKET_BYTES recommended) of device memory that is ZERO to a stream; every launch on that stream
 * may use them and leaves them zero.  One buffer per stream that launches weight gradients concurrently; a stream without a
 * binding (or buf = NULL: unbind) keeps the separate reduction launch - results differ from the ticketed ones only in the order
 * of the additions.  The binding table holds NIMG_TICKET_STREAMS streams.  Host-side call, no device work. */
#define NIMG_TICKET_BYTES (64 * 1024)
#define NIMG_TICKET_STREAMS 16
int nimg_bind_tickets(void* stream, void* buf, size_t bytes);

/* A HIP stream whose kernels run on `n_cus` compute units only (hipExtStreamCreateWithCUMask, mask = the low n_cus bits: the
 * driver deals mask bits round-robin over the 8 XCDs, so any n is balanced to within one CU per XCD).  For partitioning the chip
 * between kernel classes that only evict each other when interleaved workgroup by workgroup - the matrix-core-bound weight
 * gradients of the FAN beside the byte-bound backward pass of the image chain (workflows/manipulation_classification.py:260-285
 * under the tape).  *stream is a hipStream_t the caller owns (nimg_stream_destroy). */
int nimg_stream_create_cu_mask(int n_cus, void** stream);
int nimg_stream_destroy(void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The FAN's head in throughput mode - Conv2D(nf, 1x1, leaky_relu) -> GlobalAveragePooling2D -> Dense(softmax),
 * models/forensics.py:76-94 - with the pooling fused into the 1x1 layer (csrc/head.hip).  hw = pixels per image (64 | 128 | 256),
 * c = channels in = channels out (64 | 128 | 256): nimg_head_fused_ok.  x (n * hw, c) bf16; wimg / wimg_t the 1x1 kernel's bf16
 * images (nimg_conv_weights_bf16 mode 0 / mode 1).
 *   nimg_head_fwd:   gap (n, c) = mean over the image of LeakyReLU(x W + b); mask (n * hw, c / 32) words, bit j of word f = the
 *                    activation of channel 32 f + j is > 0 (NULL at inference) - the activation tensor itself is not written.
 *   nimg_fan_dense_fwd / _bwd: the Dense softmax / sparse-CE classifier on a pooled feature (the two halves of nimg_fan_head_fwd /
 *                    _bwd that do not touch the activation tensor).
 *   nimg_head_dgrad: dx (n * hw, c) bf16 = ((g (x) (bit ? 1 : alpha)) W^T) * LeakyReLU'(in_mask) with g[n] = wdense dlogits[n] / hw:
 *                    the gradient at the INPUT of the 1x1 layer straight from the classifier's dlogits (n, k); in_mask bf16 or NULL.
 *   nimg_head_dact:  the gradient at the 1x1 layer's pre-activation as bf16 (n * hw, c), for its weight gradient. */
int nimg_head_fused_ok(int hw, int c);
int nimg_head_fwd(const void* x, const void* wimg, const float* bias, unsigned* mask, unsigned* mask_p, float* gap, int n, int hw,
                  int c, float alpha, void* stream);
/*   nimg_head_wgrad: weight + bias gradient of the 1x1 layer from its bf16 input x and the PIXEL-MAJOR sign words mask_p
 *                    (n, hw / 32, c): bit j of word [n][b][co] = the activation of channel co at pixel 32 b + j is > 0 (written by
 *                    nimg_head_fwd next to mask) - the gradient at the pre-activation is built inside the kernel.  dw (c, c) in the
 *                    Keras (1, 1, cin, cout) layout, db (c) or NULL; split over the images, fixed-order reduction through
 *                    `workspace` (nimg_head_wgrad_workspace_bytes). */
size_t nimg_head_wgrad_workspace_bytes(int n, int c);
int nimg_head_wgrad(const void* x, const unsigned* mask_p, const float* dlogits, const float* wdense, int k, float* dw, float* db,
                    int n, int hw, int c, float alpha, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
int nimg_head_dgrad(const unsigned* mask, const float* dlogits, const float* wdense, int k, const void* wimg_t,
                    const void* in_mask, void* dx, int n, int hw, int c, float alpha, void* stream);
int nimg_head_dact(const unsigned* mask, const float* dlogits, const float* wdense, int k, void* dact, int n, int hw, int c,
                   float alpha, void* stream);
int nimg_fan_dense_fwd(const float* gap, const float* w, const float* b, const int* labels, float* probs, float* loss_per,
                       float* dlogits, int n, int c, int k, float loss_scale, void* stream);
int nimg_fan_dense_bwd(const float* gap, const float* dlogits, const float* loss_per, float* dw, float* db, float* loss, int n,
                       int c, int k, float loss_scale, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * ConstrainedConv2D kernel re-normalisation, models/layers.py:45-53 (ks=5, channels=3, strength=100) */
int nimg_constrained_kernel_fwd(const float* kernel, float* nf, int ks, int channels, float strength, void* stream);
int nimg_constrained_kernel_bwd(const float* kernel, const float* dnf, float* dkernel, int ks, int channels,
                                float strength, void* stream);
/* backward of tf.pad(SYMMETRIC|REFLECT): fold a gradient on the padded domain (n,h+2p,w+2p,c) onto (n,h,w,c) */
int nimg_fold_pad(const float* dpad, float* dx, int n, int h, int w, int c, int pad, int pad_mode, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Photo manipulations, helpers/tf_helpers.py.  Images (n,h,w,3).  mask: (n,h,w) uint8 clip mask written by the forward
 * (bit c set <=> channel c not clipped), consumed by the backward. */
/* manipulation_gaussian :113-125 - gk25 = 5x5 normalised kernel (device), REFLECT pad */
int nimg_gaussian_fwd(const float* x, float* y, uint8_t* mask, const float* gk25, int n, int h, int w, int clip,
                      void* stream);
int nimg_gaussian_bwd(const float* dy, const uint8_t* mask, float* dx, const float* gk25, int n, int h, int w,
                      void* stream);
/* any odd k x k (k <= 31) per-channel filter with a mirrored border (pad_mode 1 SYMMETRIC, 2 REFLECT) and an optional hard
 * clip: manipulation_gaussian with kernel != 5 (:113-125, REFLECT), manipulation_sharpen(hsv=False) (:156-184, SYMMETRIC),
 * residual(hsv=False) (:127-154, REFLECT, clip 0).  taps = k*k floats (device), mask as nimg_gaussian_fwd (may be NULL). */
int nimg_dwfilter_fwd(const float* x, float* y, uint8_t* mask, const float* taps, int k, int pad_mode, int n, int h, int w,
                      int clip, void* stream);
int nimg_dwfilter_bwd(const float* dy, const uint8_t* mask, float* dx, const float* taps, int k, int pad_mode, int n, int h,
                      int w, void* stream);
/* manipulation_sharpen(hsv=True) :156-184 - gk9 = 3x3 H/V filter (device); aux_hsv (n,h,w,3) scratch kept between
 * forward and backward (filtered HSV; overwritten by the backward) */
int nimg_sharpen_fwd(const float* x, float* y, float* aux_hsv, uint8_t* mask, const float* gk9, int n, int h, int w,
                     void* stream);
int nimg_sharpen_bwd(const float* x, const float* dy, float* aux_hsv, const uint8_t* mask, float* dx,
                     const float* gk9, int n, int h, int w, void* stream);
/* banded linear operator along one spatial axis (CSR rows = output index): manipulation_resample :68-76 and
 * tf.image.resize bilinear down-sampling are two such passes; their backward uses the transposed CSR. */
int nimg_sparse_axis_apply(const float* in, float* out, const int* rowptr, const int* col, const float* val, int n,
                           int hin, int win, int c, int axis, int out_size, void* stream);

/* Building blocks of the MS-SSIM loss (helpers/tf_helpers.py:43-44 -> tf.image.ssim_multiscale, 5 scales, weights 0.0448,
 * 0.2856, 0.3001, 0.2363, 0.1333; the 2x2 average pooling between the scales is nimg_avgpool_fwd / _bwd):
 *  ssim_planes: per (image, channel) means of the SSIM map and of its contrast-structure factor (either may be NULL) over
 *               the VALID positions of the 11x11 Gaussian window, and - which_maps 1 (SSIM) | 2 (cs) - the unscaled
 *               derivative maps w.r.t. the window moments, 3 x n x (h-10) x (w-10) x c floats;
 *  msssim_combine: values (scales, n*c) = cs means of scales 0..S-2 and the SSIM mean of the last one; items (scales) = window
 *               positions per plane; loss = 255 (1 - mean prod relu(v)^w); coef (scales, n*c) = d loss / d v / items;
 *  ssim_maps_grad: grad_y (+)= grad_scale * coef[n, c] * (transposed-window gather of the maps). */
size_t nimg_ssim_planes_workspace_bytes(int n, int c);
int nimg_ssim_planes(const float* y, const float* t, int n, int h, int w, int c, float max_val, const float* gauss_win,
                     float* mean_ssim, float* mean_cs, float* maps, int which_maps, void* workspace,
                     size_t workspace_bytes, void* stream);
int nimg_msssim_combine(const float* values, const float* items, int scales, int planes, float* loss, float* coef,
                        void* stream);
int nimg_ssim_maps_grad(const float* y, const float* t, const float* maps, const float* coef, float* grad_y, int n,
                        int h, int w, int c, const float* gauss_win, float grad_scale, int accumulate, void* stream);
/* The metric itself: out[i] = tf.image.ssim_multiscale(a, b, max_val)[i] of two (n,h,w,c) batches, a float64 (its users take
 * 1 - out[i]) - the five scales of nimg_ssim_planes with nimg_avgpool_fwd (2x2) between them, then
 * out[i] = mean_c prod_k relu(v[k][i][c]) ^ w[k].  The value of an image does not depend on the rest of the batch: every sum has one
 * fixed order and is taken over that image alone.  h and w must be multiples of 16 with h / 16, w / 16 >= 11 (TF pads odd scales
 * symmetrically instead; not built) - workspace_bytes is 0 and the call NIMG_ERR_ARG otherwise.  The workspace holds the pooled
 * pyramids of both batches, the per-scale values and nimg_ssim_planes' own. */
size_t nimg_msssim_workspace_bytes(int n, int h, int w, int c);
int nimg_msssim(const float* a, const float* b, int n, int h, int w, int c, float max_val, const float* gauss_win, double* out,
                void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * GPU-resident training-data feed (helpers/dataset.py:89-131 `Dataset.next_training_batch`, helpers/loading.py:132-211
 * `sample_patch`).  rgb: (n_images, h, w, 3) uint8, raw: (n_images, h/2, w/2, 4) uint16, both resident in HBM.
 * image_idx (b) picks the image of every batch entry; cand_xy (b, attempts, 2) are candidate (xx, yy) patch corners (even
 * numbers, the Bayer alignment of loading.py:160-161); patch = RGB patch size (even).
 *  stats:  var / mean (b, attempts) of every candidate patch / 255 (np.var, np.mean over all three channels; :166-168).
 *  select: the discard policy over each image's candidates -> chosen_xy (b, 2); mode 0 none, 1 'flat' (uniforms (b,
 *          attempts) feed its coin flip, :177-178), 2 'flat-aggressive', 3 'dark-n-textured'; max_attempts = the panic
 *          counter (:156); attempts_used (b, may be NULL) = candidates consumed.  Two deviations from the reference: if the
 *          candidates run out before the policy settles the last one is taken; and since stats gives an exactly flat patch
 *          the variance 0.0 (exact integer moments), 'dark-n-textured' rejects it by `0 < variance` - the reference's np.var of
 *          a constant patch / 255 is a rounding residue of ~1e-34 at most byte levels, which it accepts when the mean is in
 *          (0.35, 0.99).
 *  stats and gather need even h and w (2-byte row loads), NIMG_ERR_ARG otherwise.
 *  gather: x_out (b, patch/2, patch/2, 4) = raw crop / 65535, y_out (b, patch, patch, 3) = rgb crop / 255 (either may be
 *          NULL), float32 of the float64 quotient like dataset.py:124-126. */
int nimg_patch_stats(const uint8_t* rgb, int n_images, int h, int w, const int* image_idx, const int* cand_xy, int b,
                     int attempts, int patch, double* var_out, double* mean_out, void* stream);
int nimg_patch_select(const int* cand_xy, const float* uniforms, const double* var, const double* mean, int b,
                      int attempts, int max_attempts, int mode, int* chosen_xy, int* attempts_used, void* stream);
int nimg_patch_gather(const uint16_t* raw, const uint8_t* rgb, int n_images, int h, int w, const int* image_idx,
                      const int* xy, int b, int patch, float* x_out, float* y_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Learned codec (TwitterDCN, models/compression.py:197-279) specific pieces */
int nimg_affine(const float* x, float* y, long count, float a, float b, void* stream);     /* y = a*x + b (:219,:268) */
int nimg_lrelu_fwd(const float* x, float* y, long count, float alpha, void* stream);       /* tf.nn.leaky_relu (:224) */
/* Element-wise pieces of the INet / DNet pipelines (models/pipelines.py:238-345): tanh of the gamma MLP (:283) and its
 * derivative through the stored output, the straight-through clip (:287, :341; gradient = identity), and
 * tf.pad(x, [[0,0],[P,P],[P,P],[0,0]], CONSTANT | SYMMETRIC | REFLECT) (:272, :320, :338; backward = nimg_fold_pad). */
int nimg_tanh_fwd(const float* x, float* y, long count, void* stream);
int nimg_tanh_bwd(const float* dy, const float* y, float* dx, long count, void* stream);
int nimg_clip01(const float* x, float* y, long count, void* stream);
int nimg_pad2d(const float* x, float* y, int n, int h, int w, int c, int pad, int pad_mode, void* stream);
/* Element-wise pieces of ClassicISP (models/pipelines.py:416-453 `_ClassicISP.call`, models/layers.py:206-258
 * `DemosaicingLayer`).
 *  residual: y = [clip01](x - alpha[0] * f)  (layers.py:252-255; f NULL = the c_filters=() case, y = [clip01](x)); the clip
 *            is straight-through, so the backward pass is df = -alpha dy, dalpha (+)= -sum(dy f) (fixed-order sum;
 *            workspace = nimg_isp_residual_workspace_bytes() bytes of device scratch), dx = dy.
 *  sigmoid:  activation of the non-residual head (layers.py:235), backward through the stored output.
 *  gamma_ste: y = pow(clip(x, lo, hi), exponent) with a straight-through clip (pipelines.py:449-451: lo 1/255, hi 1,
 *            exponent 1/2.2): dx = dy * exponent * pow(clip(x), exponent - 1). */
int nimg_isp_residual_fwd(const float* x, const float* f, const float* alpha, float* y, long count, int clip,
                          void* stream);
long nimg_isp_residual_workspace_bytes(void);
int nimg_isp_residual_bwd(const float* dy, const float* f, const float* alpha, float* df, float* dalpha,
                          float* workspace, long count, int accumulate, void* stream);
/* Dropout of the FAN's hidden Dense layers at training time (models/forensics.py:88), forward and backward alike:
 * y = keep[i] ? x[i] * scale : 0, keep = the Bernoulli(1 - rate) mask bytes, scale = 1 / (1 - rate). */
int nimg_mask_scale(const float* x, const uint8_t* keep, float* y, long count, float scale, void* stream);
/* Input gradient of a fused 5x5 conv + pool layer (stride 1, SAME) from the POOLED gradient g (n, h/2, wd/2, cout) bf16 + arg-max
 * bytes on the 2:4 structured-sparsity matrix instruction (csrc/dgrad5s.hip): the same result as nimg_conv2d_fwd_bf16_unpool to
 * summation order.  `image` = nimg_conv5_dgrad_sparse_weights(w (5,5,cin,cout) float32) of nimg_conv5_dgrad_sparse_image_bytes
 * bytes, rebuilt whenever w changes.  out (n, h, wd, cin) float32 | bf16 (NIMG_BF16_OUT), act_mask optional (float32 | bf16 with
 * NIMG_BF16_MASK): out *= act_mask > 0 ? 1 : alpha.  cin % 32 == 0, cout % 8 == 0, even h / wd (else NIMG_ERR_ARG). */
size_t nimg_conv5_dgrad_sparse_image_bytes(int cin, int cout);
int nimg_conv5_dgrad_sparse_weights(const float* w, void* image, int cin, int cout, void* stream);
int nimg_conv5_dgrad_sparse(const void* g, const unsigned char* idx, int cout, const void* image, void* out, int cin,
                            const void* act_mask, int n, int h, int wd, float alpha, int flags, void* stream);
/* nimg_conv2d_fwd_bf16_ex for the layers of a residual block (models/compression.py:224-227, 240-243): `residual` (float32, the
 * shape of out1, optional) is added after bias, activation and mask (net + conv(a) forward, d_net + mask * dgrad backward), and
 * `out_bf16_copy` (optional) receives the same result rounded to bf16 next to the float32 out1 (the exact float32 stream for the
 * skip sum, the bf16 copy for the convolutions / weight gradients that read it; with NIMG_COPY_LRELU the copy holds
 * LeakyReLU(alpha) of the result, models/compression.py:224).  At least one of the two; float32 output with o1 % 4 == 0; the
 * residual with 3x3 / stride 1 layers only. */
int nimg_conv2d_fwd_bf16_res(const float* in1, int c1, const void* wb, const float* bias, float* out1, int o1,
                             const float* act_mask, const float* residual, void* out_bf16_copy, int n, int h, int wd, int ks,
                             int stride, int pad_t, int pad_l, int pad_mode, int hout, int wout, int act, float alpha, int flags,
                             void* stream);
/* Backward of the FAN's fused conv + LeakyReLU + MaxPool2D layers conv2..4 (models/forensics.py:73-77) straight from the POOLED
 * gradient g (bf16, already x LeakyReLU') and the arg-max bytes: the MaxPool2D routing is applied while the kernels stage their
 * tiles, so the full-resolution gradient (4x the bytes, 3/4 zeros) is never written nor re-read.  5x5, stride 1, SAME.
 *   _fwd_bf16_unpool:   input gradient = convolution of the un-pooled g with wb = nimg_conv_weights_bf16(w, mode 1); arguments as
 *                       nimg_conv2d_fwd_bf16_ex with (h, wd) the FULL resolution; flags may add NIMG_BF16_OUT / NIMG_BF16_MASK
 *   _wgrad_bf16_unpool: dw (5,5,cin,cout) / db (cout) from the layer input `in` (n,h,wd,cin) bf16 and (g, idx) */
int nimg_conv2d_fwd_bf16_unpool(const void* in_pooled, const unsigned char* in_idx, int c1, const void* wb, const float* bias,
                                float* out1, int o1, const float* act_mask, int n, int h, int w_, int ks, int pad_t, int pad_l,
                                int hout, int wout, int act, float alpha, int flags, void* stream);
int nimg_conv2d_wgrad_bf16_unpool(const void* in, int cin, const void* g, const unsigned char* idx, int cout, float* dw, float* db,
                                  int n, int h, int w_, int ks, int accumulate, void* workspace, size_t workspace_bytes,
                                  void* stream);
/* DEFERRED slab reduction (round 5): nimg_conv2d_wgrad_bf16_deferred = nimg_conv2d_wgrad_bf16_ex (idx == null) or
 * nimg_conv2d_wgrad_bf16_unpool (idx != null) with accumulate = 0, except that the reduction of the split-K partial sums is not
 * launched but described in *entry (nimg_reduce_entry_bytes() bytes of HOST memory); the workspace must stay untouched until
 * nimg_reduce_slabs_batch(entries, n, stream) has been issued on the same stream.  One batch launch runs the reductions of up to
 * nimg_reduce_batch_max() weight gradients (the entries travel as kernel arguments: nothing is copied to the device, the launch
 * can be captured); every sum is bit-identical to the per-layer reduction of the non-deferred entry points. */
int nimg_conv2d_wgrad_bf16_deferred(const void* in1, int c1, const void* in2, int c2, const void* dz, const unsigned char* idx,
                                    int cout, float* dw, float* db, int n, int h, int wd, int ks, int stride, int pad_t, int pad_l,
                                    int pad_mode, int hout, int wout, void* workspace, size_t workspace_bytes, int flags,
                                    void* entry, void* stream);
/* Chained form: the same call, which ALSO runs the reduction owed by a previous deferred / chained call on this stream (pre_entry:
 * the entry that call filled, or NULL) - in the prologue of this call's own kernel where that kernel can (the 3x3 all-taps and the
 * generic bf16 weight-gradient kernels), as a separate launch in front of it otherwise.  The previous call's workspace must stay
 * untouched until this call has been issued; the last entry of a chain goes to nimg_reduce_slabs_batch.  Sums bit-identical to the
 * per-layer reduction.  entry may alias pre_entry. */
int nimg_conv2d_wgrad_bf16_chained(const void* in1, int c1, const void* in2, int c2, const void* dz, const unsigned char* idx,
                                   int cout, float* dw, float* db, int n, int h, int wd, int ks, int stride, int pad_t, int pad_l,
                                   int pad_mode, int hout, int wout, void* workspace, size_t workspace_bytes, int flags,
                                   const void* pre_entry, void* entry, void* stream);
size_t nimg_reduce_entry_bytes(void);
int nimg_reduce_batch_max(void);
int nimg_reduce_slabs_batch(const void* entries, int n, void* stream);

/* The same 5x5, 3 -> 3 convolution with ZERO padding and bf16 matrix-core operands (float32 accumulation, float32 output): the
 * main term of the ConstrainedConv2D input gradient in throughput mode (models/layers.py:56-57 backward; w = the flipped /
 * transposed filter, nimg_conv_flip_weights).  wd % 64 == 0 (else NIMG_ERR_ARG: use nimg_cconv3). */
int nimg_conv5c3_bf16(const float* in, const float* w, float* out, int n, int h, int wd, void* stream);
/* ------------------------------------------------------------------------------------------------------------------
 * FAN front end (csrc/frontend.hip): ConstrainedConv2D, models/layers.py:56-57 (tf.pad SYMMETRIC + VALID conv2d) and the
 * first FAN convolution, models/forensics.py:69-70, as row-band kernels (float32 VALU stencil / bf16 MFMA).
 *
 * nimg_cconv3: 5x5 convolution 3 -> 3, same-size output, no bias: out[y][x][o] = sum in_pad[y+ky-2][x+kx-2][i] w[ky][kx][i][o]
 * with pad_mode 0 (zeros) | 1 (SYMMETRIC).  w = the 225 floats of a (5,5,3,3) HWIO kernel in device memory.
 *   forward:        w = the normalised filter (nimg_constrained_kernel_fwd), pad_mode 1
 *   input gradient: w = nimg_conv_flip_weights(normalised filter), pad_mode 0, then nimg_cconv3_dgrad_border adds what the
 *                   SYMMETRIC pad folds back onto the two outermost rows / columns (needs h, w >= 4).
 * out_f32 (n,h,w,3) float32 and / or out_c4 (n,h,w,4) bf16 = {o0, o1, o2, 1.0} (the 8-byte pixel of the throughput-mode
 * conv1 kernels; the constant channel carries the bias gradient through their weight-gradient GEMM); at least one. */
int nimg_cconv3(const float* in, const float* w, float* out_f32, void* out_c4, int n, int h, int w_, int pad_mode,
                void* stream);
int nimg_cconv3_dgrad_border(const float* dc, const float* nf, float* dx, int n, int h, int w_, void* stream);
/* The same terms added to dx in the same order, so bit for bit the same result, with the strips of dc that a stretch of the
 * border needs staged in LDS (one workgroup per 64 border positions) instead of one dependent L2 read per tap. */
int nimg_cconv3_dgrad_border_strips(const float* dc, const float* nf, float* dx, int n, int h, int w_, void* stream);
/* First FAN convolution in throughput mode, models/forensics.py:69-70: Conv2D(32, 5x5, SAME) + bias + LeakyReLU(alpha) +
 * MaxPool2D(2) in one pass over the bf16 {c0,c1,c2,1} pixels of nimg_cconv3 (bf16 MFMA operands, float32 accumulation).
 * c4 (n,h,w,4) bf16; w (5,5,3,32) float32 HWIO; bias (32) or NULL; pooled (n,h/2,w/2,32) bf16 (out_bf16 = 1) or float32;
 * pool_idx (n,h/2,w/2,8) uint8 or NULL: the arg-max position inside the window (row-major, first maximum wins) as 2 bits per
 * channel - channel c in byte c >> 2, bits 2 (c & 3) .. 2 (c & 3) + 1 (the layout nimg_conv1_wgrad_c4 / nimg_conv1_dgrad_pooled read).
 * h, w even; 0 < alpha <= 1 (1 = no activation). */
int nimg_conv1_pool_fwd_c4(const void* c4, const float* w, const float* bias, void* pooled, unsigned char* pool_idx, int n,
                           int h, int w_, float alpha, int out_bf16, void* stream);
/* Weight and bias gradient of that convolution from the POOLED gradient (backward of nimg_conv1_pool_fwd_c4; the tape of
 * forensics.py:118-124 for this layer): dw (5,5,3,32) (+)= sum c (x) dz, db (32) (+)= sum dz with dz = the MaxPool2D routing of g
 * by the arg-max bytes.  c4 as above; g (n,h/2,w/2,32) bf16 (g_bf16 = 1) or float32, already multiplied by LeakyReLU';
 * db may be NULL.  workspace: nimg_conv1_wgrad_c4_workspace_bytes() bytes (one slab per workgroup, reduced in a fixed order). */
size_t nimg_conv1_wgrad_c4_workspace_bytes(void);
int nimg_conv1_wgrad_c4(const void* c4, const void* g, const unsigned char* pool_idx, float* dw, float* db, int n, int h, int w_,
                        int g_bf16, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* Input gradient of that convolution from the pooled gradient: dc (n,h,w,3) float32 = sum_{ky,kx,o} dz[y+2-ky][x+2-kx][o]
 * w[ky][kx][i][o] (bf16 MFMA operands, float32 accumulation); w = the (5,5,3,32) float32 forward kernel as stored. */
int nimg_conv1_dgrad_pooled(const void* g, const unsigned char* pool_idx, const float* w, float* dc, int n, int h, int w_,
                            int g_bf16, void* stream);
/* Classifier decisions + confusion matrix on the device - replaces the host loop of validate_fan,
 * training/validation.py:163-202 (np.argmax per batch, conf[c, c_] += sum((y == c) * (pred == c_)), one D2H per batch).
 * probs (n,k) float32; labels (n) int32 or NULL; pred (n) int32 or NULL: first arg-max of each row (numpy.argmax);
 * conf (k,k) uint64 or NULL (needs labels): conf[label][pred] += 1, accumulated over calls - the caller zeroes it once per
 * validation pass and reads it back once. */
int nimg_confusion_accumulate(const float* probs, const int* labels, int* pred, unsigned long long* conf, int n, int k,
                              void* stream);
int nimg_sigmoid_fwd(const float* x, float* y, long count, void* stream);
int nimg_sigmoid_bwd(const float* dy, const float* y, float* dx, long count, void* stream);
/* The activations a UNet / FAN / TwitterDCN may be built with besides LeakyReLU(0.2) - helpers/tf_helpers.py:22-28
 * `activation_mapping`, selected by the models' `activation=` hyper-parameter (models/pipelines.py:179, forensics.py:55,
 * compression.py:202): kind 0 leaky_relu(alpha), 1 relu, 2 tanh, 3 sigmoid, 4 softsign x / (1 + |x|).  Element-wise on float32,
 * y may alias x; the backward pass takes the derivative from the stored OUTPUT y (y > 0 ? 1 : alpha | y > 0 | 1 - y^2 |
 * y (1 - y) | (1 - |y|)^2), dx may alias dy.  NIMG_ERR_ARG for another kind. */
int nimg_activation_fwd(const float* x, float* y, long count, int kind, float alpha, void* stream);
int nimg_activation_bwd(const float* dy, const float* y, float* dx, long count, int kind, float alpha, void* stream);
int nimg_gamma_ste_fwd(const float* x, float* y, long count, float lo, float hi, float exponent, void* stream);
int nimg_gamma_ste_bwd(const float* x, const float* dy, float* dx, long count, float lo, float hi, float exponent,
                       void* stream);
/* out (n,2h,2w,c) = in with zeros inserted (stride-2 transposed convolution = zero insertion + stride-1 conv) */
/* 5x5 stride-2 TF-SAME convolution (Conv2D(.., 5, strides=2) of TwitterDCN, models/compression.py:217-229) as a 3x3 stride-1
 * convolution over the space-to-depth image (even h, w; cp >= 4 c block channels, the rest zero):
 *   s2d2_affine_bf16       y (n,h/2,w/2,cp) bf16: y[by][bx][(2 pr + pc) c + ci] = a x[2by + pr][2bx + pc][ci] + b
 *   s2d_conv_weights       w5 (5,5,cin,cout) -> w3 (3,3,cp,cout), tap ky = 2 dy + pr - 1;  _bwd gathers dw3 back into dw5
 *   d2s2_scale             x (n,h,w,c) = scale * depth-to-space of xs (n,h/2,w/2,cp): the input gradient of the layer */
int nimg_s2d2_affine_bf16(const float* x, void* y, int n, int h, int w, int c, int cp, float a, float b, void* stream);
int nimg_s2d_conv_weights(const float* w5, float* w3, int cin, int cp, int cout, void* stream);
int nimg_s2d_conv_weights_bwd(const float* dw3, float* dw5, int cin, int cp, int cout, int accumulate, void* stream);
int nimg_d2s2_scale(const float* xs, float* x, int n, int h, int w, int c, int cp, float scale, void* stream);
int nimg_zero_insert2(const float* in, float* out, int n, int h, int w, int c, void* stream);
/* DiscreteLatent (models/layers.py:183-203): latent = Quantization('soft-codebook' | identity)(scale * z) evaluated in
 * float64 like the reference (layers.py:141), plus the batch-global differentiable entropy of the latent
 * (helpers/tf_helpers.py:290-333).  scale: device scalar (may be NULL = 1).  count_global: number of latent values over
 * ALL ranks (0 = count).  finalize = 0 leaves the K float64 histogram sums at workspace + 1024*K doubles for an
 * all-reduce; call nimg_latent_entropy_finalize afterwards. The workspace must stay untouched until nimg_latent_bwd.
 * soft_codebook: bit 0 = Quantization('soft-codebook') (else identity); bit 1 = the caller's promise that the codebook is
 * unit-spaced (codebook[k] = codebook[0] + k, the reference's consecutive integers, models/layers.py:160-170): with gamma >= 25
 * and v = 50 the kernels then evaluate, for a value inside the codebook's range, only the five centres around the nearest one -
 * the weight of any other centre is below 2e-33 of the nearest one's, under the last bit of every float64 sum it would enter. */
size_t nimg_latent_workspace_bytes(int codebook_size);
int nimg_latent_fwd(const float* z, const float* scale, const float* codebook, int codebook_size, float v,
                    float gamma, int soft_codebook, float* latent, float* entropy, long count, long count_global,
                    void* workspace, size_t workspace_bytes, int finalize, void* stream);
int nimg_latent_entropy_finalize(int codebook_size, long count_global, float* entropy, void* workspace, void* stream);
/* dz = d loss / d z given dlatent (may be NULL) and the entropy term's coefficient d loss / d H; dscale (optional) */
int nimg_latent_bwd(const float* z, const float* scale, const float* latent, const float* dlatent,
                    float entropy_coef, const float* codebook, int codebook_size, float v, float gamma,
                    int soft_codebook, float* dz, float* dscale, int accumulate_dscale, long count, void* workspace,
                    size_t workspace_bytes, void* stream);
/* tf.nn.l2_loss(target - y) = sum((target-y)^2)/2 and grad_y (+)= grad_scale * (y - target)  (compression.py:92-93) */
size_t nimg_l2_loss_workspace_bytes(void);
int nimg_l2_loss(const float* target, const float* y, float* loss, float* grad_y, long count, float grad_scale,
                 int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Throughput mode of the convolutions: bf16 operands on the matrix cores (v_mfma_f32_32x32x16_bf16), float32
 * accumulation, float32 tensors in HBM.  Same semantics / arguments as nimg_conv2d_fwd / nimg_conv2d_wgrad; channel
 * counts must be multiples of 8 (forward) / 4 (weight gradient).  Judged on PSNR / accuracy parity (BASELINE.json),
 * not on the 1e-4 contract.  Weights are laid out once per step by nimg_conv_weights_bf16:
 *   mode 0 (forward)        wb[ci/16][tap][co][ci%16]        = w[tap][ci][co]   (16-channel chunk major, zero padded)
 *   mode 1 (input gradient) wb[co/16][taps-1-tap][ci][co%16] = w[tap][ci][co]   (then call with cin/cout swapped) */
size_t nimg_conv_weights_bf16_bytes(int ks_h, int ks_w, int cin, int cout, int mode);
int nimg_conv_weights_bf16(const float* w, void* wb, int ks_h, int ks_w, int cin, int cout, int mode, void* stream);
/* Backward of a fused conv+pool layer with few input channels (FAN conv1, forensics.py:69-70) without materialising
 * the sparse full-resolution gradient: g (n,h/2,wd/2,cout) = upstream gradient x LeakyReLU'(pooled), idx = arg-max
 * bytes of nimg_conv2d_pool_fwd[_bf16]; the 2x2 un-pooling happens while the tiles are staged.
 *   wgrad: cin 3|4, ks 3|5, SAME, stride 1;  dgrad: ci 3, cz 32, ks 5 (w = the forward kernel as stored). */
int nimg_conv2d_wgrad_pooled_bf16(const float* in, int cin, const float* g, const unsigned char* idx, int cout,
                                  float* dw, float* db, int n, int h, int wd, int ks, int accumulate, void* workspace,
                                  size_t workspace_bytes, void* stream);
int nimg_conv2d_dgrad_fewin_pooled_bf16(const float* g, const unsigned char* idx, const float* w, float* out, int ci,
                                        int cz, int n, int h, int wd, int ks, void* stream);
/* bf16 STORAGE of the FAN-internal tensors in throughput mode.  Every consumer of the pooled activations, of the
 * un-pooled gradients and of the pooled gradients converts them to bf16 MFMA operands anyway, so keeping them in bf16
 * in HBM changes no result bit - it only halves the bytes the kernels stage.  Same arguments as the entry points
 * without _ex, plus `flags` (NIMG_BF16_*) saying which tensors hold bf16. */
int nimg_conv2d_fwd_bf16_ex(const float* in1, int c1, const float* in2, int c2, const void* wb, const float* bias,
                            float* out1, int o1, float* out2, int o2, const float* act_mask, int n, int h, int wd,
                            int ks, int stride, int pad_t, int pad_l, int pad_mode, int hout, int wout, int act,
                            float alpha, int flags, void* stream);
int nimg_conv2d_wgrad_bf16_ex(const float* in1, int c1, const float* in2, int c2, const float* dz, int cout, float* dw,
                              float* db, int n, int h, int wd, int ks, int stride, int pad_t, int pad_l, int pad_mode,
                              int hout, int wout, int accumulate, void* workspace, size_t workspace_bytes, int flags,
                              void* stream);
int nimg_conv2d_pool_fwd_bf16_ex(const float* in, int cin, const float* w, const void* wb, const float* bias,
                                 float* pool_out, unsigned char* pool_idx, int cout, int n, int h, int wd, int ks,
                                 int act, float alpha, int flags, void* stream);
/* 3x3 SAME stride-1 convolution + bias + activation storing BOTH the full output and its 2x2 max-pooled tensor (bf16 in and out;
 * cin % 8 == 0, cout % 8 == 0, even h / wd > 8; pool_idx - the arg-max bytes - optional).  The second convolution of a UNet
 * encoder level + its max_pool2d (models/pipelines.py:160-173): the full tensor is the skip connection. */
int nimg_conv2d_fwd_pool_also_bf16(const float* in, int cin, const void* wb, const float* bias, float* out, float* pool_out,
                                   unsigned char* pool_idx, int cout, int n, int h, int wd, int act, float alpha, void* stream);
/* Row-band STREAMING form of the 3x3 / stride 1 / SAME convolution over bf16-stored activations with 32 output channels
 * (csrc/conv3_rows.hip; the UNet's level-1 layers, models/pipelines.py:190-216, throughput mode): in1 (n, h, wd, c1) [+ in2
 * (n, h, wd, c2)], wb = nimg_conv_weights_bf16 image (mode 0 forward, mode 1 input gradient), bias (32) or null, mask = optional
 * (n, h, wd, 32) bf16 activation whose LeakyReLU' multiplies the result, out (n, h, wd, 32) bf16, pool_out = optional
 * (n, h / 2, wd / 2, 32) bf16 2x2 max-pool of out.  Results are bit-identical to nimg_conv2d_fwd_bf16_ex (+ nimg_maxpool2_fwd_bf16).
 * Shapes: wd == 128, h % 4 == 0, cout == 32, (c1, c2) in {(32, 0), (64, 0), (32, 32)}; or cout == 64 from c1 == 32 as TWO 32-channel
 * tensors out / out2 (a decoder layer's input gradient, no bias / mask / pool).  flags: NIMG_ROWS_F32_OUT = out holds float32.
 * Second level of the UNet: wd == 64, (c1, c2, cout) in {(32, 0, 64), (64, 0, 64)}, out (n, h, wd, 64) bf16 (mask likewise), no pool.
 * Anything else NIMG_ERR_ARG (use the tile kernels). */
#define NIMG_ROWS_F32_OUT 1
int nimg_conv3_rows_bf16(const void* in1, int c1, const void* in2, int c2, const void* wb, const float* bias, const void* mask,
                         void* out, void* out2, void* pool_out, int n, int h, int wd, int cout, int act, float alpha, int flags,
                         void* stream);
/* The UNet's last layer in the same form: 3x3 convolution 32 -> 12 channels + bias, written as clip(depth_to_space(., 2), 0, 1)
 * (models/pipelines.py:216-223; the clip is straight-through, this is its forward value): in (n, h, wd, 32) bf16, wb the mode-0
 * weight image of the (3, 3, 32, 12) kernel, bias (12) or null, y (n, 2 h, 2 wd, 3) float32.  Bit-identical to
 * nimg_conv2d_fwd_bf16_ex + nimg_d2s_clip_fwd(scale 1, shift 0, clip).  wd == 128, h % 4 == 0. */
int nimg_conv3_rows_d2s_bf16(const void* in, int c1, const void* wb, const float* bias, float* y, int n, int h, int wd, void* stream);
/* The UNet's first layer in the same form: Conv2D(32, 3x3, SAME) + bias [+ LeakyReLU(alpha)] on the float32 4-plane RAW stack
 * (models/pipelines.py:190): in (n, h, wd, 4) float32, w (3, 3, 4, 32) float32 HWIO, out (n, h, wd, 32) bf16.  Bit-identical to
 * nimg_conv2d_fwd_smallc_bf16_ex.  wd == 128, h % 4 == 0. */
int nimg_conv3_rows_c4_bf16(const float* in, const float* w, const float* bias, void* out, int n, int h, int wd, int act, float alpha,
                            void* stream);

/* Input gradient of a 3x3 SAME stride-1 convolution whose input was a 2x2 max-pool, written THROUGH that pool (the first
 * convolution of a UNet encoder level, models/pipelines.py:160-173 under the tape), all tensors bf16: dz (n,h,wd,c1) = the
 * convolution's output gradient, wb = its weights in input-gradient form (nimg_conv_weights_bf16 mode 1), act (n,2h,2wd,cout) =
 * the activation the pool read, skip (same shape, optional, may be `out`) = the gradient arriving over the level's skip
 * connection, out (n,2h,2wd,cout) = [route to the first maximum of each window + skip] x LeakyReLU'(act) (apply_mask) - the
 * arithmetic of nimg_conv2d_fwd_bf16_ex(bf16 out) followed by nimg_maxpool2_bwd_bf16, same bits.  c1 % 8 == 0, cout % 8 == 0. */
int nimg_conv2d_dgrad_unpool_out_bf16(const float* dz, int c1, const void* wb, const float* act, const float* skip, float* out,
                                      int cout, int n, int h, int wd, int apply_mask, float alpha, void* stream);
int nimg_conv2d_wgrad_pooled_bf16_ex(const float* in, int cin, const float* g, const unsigned char* idx, int cout,
                                     float* dw, float* db, int n, int h, int wd, int ks, int accumulate, void* workspace,
                                     size_t workspace_bytes, int flags, void* stream);     /* NIMG_BF16_DZ: g is bf16 */
int nimg_conv2d_dgrad_fewin_pooled_bf16_ex(const float* g, const unsigned char* idx, const float* w, float* out, int ci,
                                           int cz, int n, int h, int wd, int ks, int flags, void* stream);
int nimg_maxpool2_unpool_ex(const float* dp, const unsigned char* idx, const float* pooled, float* dz, int n, int ho,
                            int wo, int c, int apply_lrelu_mask, float alpha, int flags, void* stream);
/* Conv2DTranspose(cout, [2,2], [2,2]) forward (pipelines.py:205) in throughput mode: four 1x1 products (one per output
 * phase) on the matrix core in one launch.  wb = nimg_conv_weights_bf16(w, 2, 2, cout, cin, mode 1) of the Keras
 * (2,2,Cout,Cin) kernel; x (n,h,wd,cin) -> y (n,2h,2wd,cout); cin % 8 == 0. */
int nimg_convt2x2_fwd_bf16(const float* x, const void* wb, const float* bias, float* y, int n, int h, int wd, int cin,
                           int cout, void* stream);
/* flags: NIMG_BF16_IN = x is stored as bf16, NIMG_BF16_OUT = y is stored as bf16 (cout % 4 == 0) */
int nimg_convt2x2_fwd_bf16_ex(const float* x, const void* wb, const float* bias, float* y, int n, int h, int wd, int cin,
                              int cout, int flags, void* stream);
/* every bf16 weight image of a model in one launch: `table` = n_entries x 4 int64 on the device,
 * {w pointer, wb pointer, (kh*kw << 32) | mode, (cin << 32) | cout}, each entry as nimg_conv_weights_bf16 would build it */
int nimg_conv_weights_bf16_batch(const void* table, int n_entries, void* stream);
int nimg_conv2d_fwd_bf16(const float* in1, int c1, const float* in2, int c2, const void* wb, const float* bias,
                         float* out1, int o1, float* out2, int o2, const float* act_mask, int n, int h, int wd,
                         int ks, int stride, int pad_t, int pad_l, int pad_mode, int hout, int wout, int act,
                         float alpha, void* stream);
size_t nimg_conv2d_wgrad_bf16_workspace_bytes(int cin, int cout, int ks_h, int ks_w, int n, int hout, int wout);
int nimg_conv2d_wgrad_bf16(const float* in1, int c1, const float* in2, int c2, const float* dz, int cout, float* dw,
                           float* db, int n, int h, int wd, int ks, int stride, int pad_t, int pad_l, int pad_mode,
                           int hout, int wout, int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* FAN front end in throughput mode (models/forensics.py:69, the 3-channel side of the first convolution):
 * few INPUT channels (cin 3 or 4; float32 HWIO weights are converted in-kernel), K = (tap, ci) packed; and the input
 * gradient of a (ks,ks,3,32) SAME stride-1 convolution with the kx loop folded into the MFMA N dimension (w = the
 * FORWARD kernel as stored).  nimg_conv2d_wgrad_bf16 picks the (tap, ci)-packed weight-gradient kernel by itself. */
int nimg_conv2d_fwd_smallc_bf16(const float* in, int cin, const float* w, const float* bias, float* out, int cout,
                                int n, int h, int wd, int ks, int pad_mode, int act, float alpha, void* stream);
/* flags: NIMG_BF16_OUT = out is stored as bf16 (cout % 4 == 0): the UNet's first convolution (pipelines.py:191, 4 -> 32) */
int nimg_conv2d_fwd_smallc_bf16_ex(const float* in, int cin, const float* w, const float* bias, float* out, int cout,
                                   int n, int h, int wd, int ks, int pad_mode, int act, float alpha, int flags, void* stream);
int nimg_conv2d_dgrad_fewin_bf16(const float* dz, const float* w, float* out, int ci, int cz, int n, int h, int wd,
                                 int ks, void* stream);

/* manipulation_awgn / _gamma / _median, helpers/tf_helpers.py:79-110.  awgn takes the noise tensor from the caller
 * (tf.random.normal is not reproducible); its mask is one byte per ELEMENT.  median: kernel odd <= 9,
 * REFLECT pad, sel (n,h,w,3) uint8 = window index of the selected element; nimg_median_bwd scatters with atomic adds into
 * a ZEROED dx. */
int nimg_awgn_fwd(const float* x, const float* noise, float* y, uint8_t* mask, long count, float strength,
                  void* stream);
int nimg_awgn_bwd(const float* x, const float* noise, const float* dy, const uint8_t* mask, float* dx, long count,
                  float strength, void* stream);
int nimg_gamma_fwd(const float* x, float* y, long count, float gamma, void* stream);
int nimg_gamma_bwd(const float* x, const float* dy, float* dx, long count, float gamma, void* stream);
int nimg_median_fwd(const float* x, float* y, uint8_t* sel, int n, int h, int w, int kernel, void* stream);
int nimg_median_bwd(const float* dy, const uint8_t* sel, float* dx, int n, int h, int w, int kernel, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * l3ic bitstream of the learned codec - replaces the per-layer host coding of compression/codec.py:87-185 (compress) and
 * :188-265 (decompress).  The container is the reference's; a compressed layer holds interleaved rANS instead of FSE
 * (format: DESIGN.md "l3ic bitstream").  A stream is one feature layer of one image: n_sym = h * w codebook indices.
 *   quantise  z (n,h,w,c) float32 -> idx (n,c,h*w) uint8, the nearest codebook entry as scipy.cluster.vq.vq finds it on
 *             float32 (squared difference, ties to the lower index); *err |= 1 for a non-finite value (zero *err first).
 *             codebook_size <= 256.
 *   encode    idx (n_streams, n_sym) uint8 -> out: the payloads of all streams back to back (capacity n_streams * n_sym),
 *             lengths[n_streams] their byte counts (a payload starts at the sum of the lengths before it).  hist / freq
 *             (optional, [n_streams][256] uint32) receive each stream's histogram and normalised frequencies.  4 <= n_sym
 *             <= 65535.  The workspace (nimg_l3ic_workspace_bytes) holds one worst-case slot per stream.
 *   decode    the payload of stream s = image s / c, layer s % c at data + offsets[s], lengths[s] bytes -> codebook[index]
 *             written into z (n,h,w,c) float32; err[s] = NIMG_L3IC_E_* bits (0 = valid).  No read leaves a payload. */
#define NIMG_L3IC_E_READ 1      /* a read past the end of the payload (truncated stream, or longer than a RAW layer) */
#define NIMG_L3IC_E_LANES 2     /* lane count outside 1..64 */
#define NIMG_L3IC_E_RANGE 4     /* first symbol > last symbol, or either has a zero frequency */
#define NIMG_L3IC_E_SYMBOL 8    /* a symbol index >= codebook_size */
#define NIMG_L3IC_E_FREQ 16     /* frequencies do not sum to 4096 */
#define NIMG_L3IC_E_VARINT 32   /* a frequency longer than 2 bytes */
#define NIMG_L3IC_E_ODD 64      /* odd number of word bytes */
#define NIMG_L3IC_E_UNUSED 128  /* words left over after the last symbol */
#define NIMG_L3IC_E_STATE 256   /* a final decoder state other than 2^16 */
#define NIMG_L3IC_E_RLE 512     /* an RLE count other than n_sym */
size_t nimg_l3ic_workspace_bytes(int n_streams, int n_sym);
int nimg_l3ic_quantise(const float* z, const float* codebook, int codebook_size, uint8_t* idx, int* err, int n, int h,
                       int w, int c, void* stream);
int nimg_l3ic_encode(const uint8_t* idx, int n_streams, int n_sym, uint8_t* out, uint32_t* lengths, uint32_t* hist,
                     uint32_t* freq, void* workspace, size_t workspace_bytes, void* stream);
int nimg_l3ic_decode(const uint8_t* data, const uint32_t* offsets, const uint32_t* lengths, const float* codebook,
                     int codebook_size, float* z, uint32_t* err, int n, int h, int w, int c, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Baseline JPEG codec - replaces the imageio / libjpeg round trip of compress_batch, compression/jpeg_helpers.py:82-114, and with
 * it the 'libjpeg' codec of JPEG.process, models/jpeg.py:227-233.  The format is libjpeg's with default settings, byte for byte
 * (DESIGN.md section 4c): one interleaved scan, Annex K Huffman tables, the IJG tables of `quality` 1..100.  A batch shares one
 * size (h, w in 1..4096), one quality and one sub-sampling (hs, vs) = (1,1) 4:4:4 | (2,1) 4:2:2 | (2,2) 4:2:0; n <= 65535.
 * Coefficients: int16 [image][Y | Cb | Cr][block row][block col][64 in zig-zag order], the REAL blocks of a component only:
 * ceil(ceil(w * hc / hs) / 8) columns with hc = hs for Y and 1 for chroma, rows alike.  One workspace size serves all three calls.
 *   transform    x (n,h,w,3) float32 (is_u8 = 0) or uint8 (is_u8 = 1) -> coef.  Float input goes through the reference's conversion
 *                (jpeg_helpers.py:92-97): divided by 255 first if any value of the batch exceeds 1, then (255 * x) in float32,
 *                truncated; clamped to 0..255 where numpy's cast would wrap.
 *   encode       coef -> out: the entropy-coded segments of all images back to back (stuffed, padded with 1-bits; the 623-byte
 *                header and EOI are the caller's), lengths[n] their byte counts (jpeg_helpers.py:97-99, imageio.imsave).  No byte
 *                is written at or beyond out_capacity: a caller that finds sum(lengths) > out_capacity calls again with more.  A
 *                segment never exceeds 2 * ceil(blocks-in-scan * 1658 / 8) bytes.  Coefficients beyond the baseline range are
 *                clamped (DC difference to +-2047, AC to +-1023).
 *   reconstruct  coef -> y (n,h,w,3) float32 = float32(byte) / 255 of the image libjpeg decodes (jpeg_helpers.py:98,101,
 *                imageio.imread): islow inverse DCT, fancy chroma up-sampling. */
size_t nimg_jpeg_workspace_bytes(int n, int h, int w, int hs, int vs);
int nimg_jpeg_transform(const void* x, int is_u8, int n, int h, int w, int hs, int vs, int quality, int16_t* coef, void* workspace,
                        size_t workspace_bytes, void* stream);
int nimg_jpeg_encode(const int16_t* coef, int n, int h, int w, int hs, int vs, uint8_t* out, size_t out_capacity, uint32_t* lengths,
                     void* workspace, size_t workspace_bytes, void* stream);
int nimg_jpeg_reconstruct(const int16_t* coef, int n, int h, int w, int hs, int vs, int quality, float* y, void* workspace,
                          size_t workspace_bytes, void* stream);
/* The item forms: one quality per image, for quality sweeps and per-image searches in one launch.  quality (device, n_items bytes):
 * item j is coded with libjpeg's tables of quality[j], read from a bank of all 100 built at compile time by the arithmetic of the
 * single-quality entry points.  A byte outside 1..100 is clamped to that range - no read leaves the bank - and *err (device, zeroed
 * by the caller) |= 1.  Workspace: nimg_jpeg_workspace_bytes(n_items, ...); nimg_jpeg_encode serves any coefficient tensor as it is.
 *   transform_items    item j = source image j % n_src of x (n_src,h,w,3): a quality-major sweep of Q qualities over N images
 *                      (n_items = Q * N) reads the N images in place.  Coefficients as above, n_items images.  The "any value above
 *                      1" flag of float input stays one per call, taken over the n_src source images.
 *   reconstruct_items  coef of n_items images -> y (n_items,h,w,3), item j dequantised with the tables of quality[j]. */
int nimg_jpeg_transform_items(const void* x, int is_u8, int n_src, int h, int w, int hs, int vs, const uint8_t* quality, int n_items,
                              int16_t* coef, int* err, void* workspace, size_t workspace_bytes, void* stream);
int nimg_jpeg_reconstruct_items(const int16_t* coef, int n_items, int h, int w, int hs, int vs, const uint8_t* quality, float* y, int* err,
                                void* workspace, size_t workspace_bytes, void* stream);

/* Decoding baseline JPEG files.  The caller parses the headers; the device takes the entropy-coded segments
 * of n files of one geometry and their Huffman tables and leaves the coefficient tensor described above.
 *   ecd        (device) the segments back to back, as they stand in the files (stuffed); segment i = bytes ecd_off[i] .. ecd_off[i+1]
 *   ecd_off    (device) n + 1 ascending byte offsets; ecd_off[n] <= the ecd_bytes the workspace was sized for, and ecd is readable
 *              up to ecd_off[n].  There is no ecd_bytes argument: the device checks the offsets against the largest total the given
 *              workspace could serve, so a workspace larger than nimg_jpeg_decode_workspace_bytes asked for loosens that check (and
 *              lengthens the clearing of the un-stuffed buffer) - pass the size that was asked for
 *   huffman    (device) [n][6][16 + 256] bytes: per image the tables Y-DC, Y-AC, Cb-DC, Cb-AC, Cr-DC, Cr-AC, each the 16 counts of
 *              its DHT body followed by the symbols in code order (unused symbol bytes are ignored)
 *   subseq_bits  the stream of an image is decoded by one thread per subsequence of this many bits: a multiple of 32 up to 2^30,
 *              0 = the default (2048); a value at least as large as the stream is a sequential decode
 *   status     (device) [n], written: 0 = decoded, else bits 1 marker inside the segment | 2 invalid code | 4 zig-zag index past 63 |
 *              8 category out of range | 16 bits needed beyond the end | 32 fewer blocks than the scan has | 64 DC outside int16 |
 *              128 DHT counts that are no prefix code | 256 bad offsets.  Nothing is read or written out of bounds whatever the
 *              bits say; coefficients of an image with a non-zero status are unspecified.
 *   rounds     (device, optional) [n]: synchronisation rounds image i took, at most its number of subsequences - 1
 * nimg_jpeg_reconstruct_tables is nimg_jpeg_reconstruct with the quantisation tables given per image and component instead of a
 * quality: qtabs (device) [n][3][64] uint16 in natural order; y is (n,h,w,3) uint8 - the decoded bytes - when out_u8, else float32
 * = float32(byte) / 255.  Its workspace is nimg_jpeg_workspace_bytes. */
size_t nimg_jpeg_decode_workspace_bytes(int n, int h, int w, int hs, int vs, size_t ecd_bytes, int subseq_bits);
int nimg_jpeg_decode(const uint8_t* ecd, const uint64_t* ecd_off, const uint8_t* huffman, int n, int h, int w, int hs, int vs,
                     int subseq_bits, int16_t* coef, uint32_t* status, uint32_t* rounds, void* workspace, size_t workspace_bytes,
                     void* stream);
int nimg_jpeg_reconstruct_tables(const int16_t* coef, int n, int h, int w, int hs, int vs, const uint16_t* qtabs, void* y, int out_u8,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* Writing files with optimised Huffman tables - what imageio.imsave writes with libjpeg's optimize_coding in
 * compression/jpeg_helpers.py:97.  A table is 16 + 256 bytes: the 16 counts of a DHT body, then the symbols in code order, unused
 * symbol bytes 0 - the layout nimg_jpeg_decode takes; the four tables of an image stand in DHT-id order 00 (Y DC), 10 (Y AC),
 * 01 (chroma DC), 11 (chroma AC), Cb and Cr sharing the last two.  Geometry and coefficients as above.
 *   histogram       coef -> hist (device) [n][4][257] uint32, zeroed by the call: how often nimg_jpeg_encode would emit each symbol
 *                   of each table (its clamps included; a dummy block counts its DC category and one end-of-block).  Entry 256 is 0.
 *                   (jpeg_helpers.py:97, imageio.imsave: libjpeg's statistics pass.)
 *   optimal_tables  hist (device) [n_tables][257] -> tables (device) [n_tables][272] by libjpeg's jpeg_gen_optimal_table: entry 256
 *                   is not read (the pseudo-symbol counts 1), ties go to the larger index, sizes are limited to 16 as Annex K.3.
 *                   status (device) [n_tables], written: 0, or 1 = a code size above 32, 2 = a histogram total of 2^32 or more (the
 *                   pseudo-symbol counted); such a table is all zeros, as is the table of an all-zero histogram (status 0).
 *                   n_tables <= 4 * 65535.  (jpeg_helpers.py:97, imageio.imsave: jpeg_gen_optimal_table.)
 *   encode_tables   nimg_jpeg_encode with the tables of each image read from `tables` (device) [n][4][272]: out, out_capacity and
 *                   lengths as there.  status (device) [n], written: 0, or bits 1 = counts that are no prefix code of lengths
 *                   1..16 with at most 256 symbols (nothing is emitted for the image, its length is 0) | 2 = a symbol that occurs
 *                   in the image has no code (it and its value bits are left out).  A DC table's symbols above 15 are ignored; of a
 *                   symbol listed twice the last code counts.  Every store stays inside the image's slot whatever the tables say.
 *                   A segment never exceeds 2 * ceil(blocks-in-scan * 1665 / 8) bytes (a DC code may take 16 bits here).  The
 *                   workspace is nimg_jpeg_encode_tables_workspace_bytes - larger than nimg_jpeg_workspace_bytes by the code
 *                   words.  (jpeg_helpers.py:97, imageio.imsave: the output pass.) */
int nimg_jpeg_histogram(const int16_t* coef, int n, int h, int w, int hs, int vs, uint32_t* hist, void* stream);
int nimg_jpeg_optimal_tables(const uint32_t* hist, int n_tables, uint8_t* tables, uint32_t* status, void* stream);
size_t nimg_jpeg_encode_tables_workspace_bytes(int n, int h, int w, int hs, int vs);
int nimg_jpeg_encode_tables(const int16_t* coef, int n, int h, int w, int hs, int vs, const uint8_t* tables, uint8_t* out,
                            size_t out_capacity, uint32_t* lengths, uint32_t* status, void* workspace, size_t workspace_bytes,
                            void* stream);

/* Writing files with any quantisation tables: the tables are an input of the transform instead of a quality.
 *   transform_tables   nimg_jpeg_transform_items with qtabs (device) [n_items][3][64] uint16 in natural order - the layout of
 *                      nimg_jpeg_reconstruct_tables - in place of the qualities: item j = source image j % n_src of x (n_src,h,w,3)
 *                      divided by its own three tables (Y, Cb, Cr).  One table set for a batch is n_items = n_src, K sets over N
 *                      images n_items = K * N.  An entry outside 1..255 is clamped to that range - no thread divides by zero - and
 *                      *err (device, zeroed by the caller) |= 1.  The "any value above 1" flag of float input is one per call, over
 *                      the n_src source images.  Workspace: nimg_jpeg_workspace_bytes(n_items, ...).  nimg_jpeg_encode,
 *                      nimg_jpeg_encode_tables and nimg_jpeg_reconstruct_tables serve the result as they are.
 *   tables_from_float  t (device) float32 [n_sets][n_tabs][64], natural order, n_tabs 2 (luma, chroma) or 3 (Y, Cb, Cr) -> qtabs
 *                      (device) uint16 [n_sets][3][64]; with two tables component 2 takes table 1.  An entry becomes rintf(v) (ties
 *                      to even) clamped to 1..255.  status (device) [n_sets], written: bits 1 = an entry was raised to 1 | 2 = an
 *                      entry was lowered to 255 | 4 = a non-finite entry (NaN and -inf become 1, +inf 255).  n_sets <= 65535. */
int nimg_jpeg_transform_tables(const void* x, int is_u8, int n_src, int h, int w, int hs, int vs, const uint16_t* qtabs, int n_items,
                               int16_t* coef, int* err, void* workspace, size_t workspace_bytes, void* stream);
int nimg_jpeg_tables_from_float(const float* t, int n_sets, int n_tabs, uint16_t* qtabs, uint32_t* status, void* stream);

/* The real codec as the forward of a training step (purely added, NIMG_ABI_VERSION stays): x (n,h,w,3) float32
 * and ONE table set qtabs (device) [3][64] uint16, natural order (Y, Cb, Cr) ->
 *   y     (n,h,w,3) float32 = float32(byte) / 255 of the image libjpeg decodes from the file it would write for x: bit-identical to
 *         nimg_jpeg_transform_tables + nimg_jpeg_reconstruct_tables for every x with all values in [0, 1].  The input conversion is
 *         255 * v in float32, truncated, clamped to 0..255 per value: there is NO batch-wide "any value above 1" flag, a value above 1
 *         is 255 (the transform would divide the whole batch by 255 instead).
 *   mask  (n,h,w) uint8 or NULL (not written), the layout nimg_djpeg_fwd writes and nimg_djpeg_bwd / nimg_djpeg_sub_bwd read: bit c is
 *         set iff output channel c (R, G, B after libjpeg's YCC -> RGB) lies in 0..255 before its range limit.  The range limit that
 *         ends the inverse DCT is not part of the mask.
 *   err   (device int, zeroed by the caller) |= 1 when a table entry outside 1..255 was clamped, as in nimg_jpeg_transform_tables.
 * (hs, vs) = (1,1), (2,1) or (2,2); whole MCUs only: h % (8 vs) == 0 and w % (8 hs) == 0.  One launch at 4:4:4; a chroma and a luma
 * launch otherwise, with the reconstructed reduced planes in the caller's workspace (nimg_jpeg_ste_workspace_bytes: 2 n h w / (hs vs)
 * bytes; 0 at 4:4:4 and for an empty or refused shape).  No allocation, no synchronisation, no atomics, nothing read back: capturable.
 * n == 0 is a no-op.  NIMG_ERR_ARG before any launch: a null x / qtabs / y / err, other factors, a ragged shape, sizes outside the
 * limits of nimg_jpeg_transform.  NIMG_ERR_WORKSPACE before any launch: a short workspace. */
size_t nimg_jpeg_ste_workspace_bytes(int n, int h, int w, int hs, int vs);
int nimg_jpeg_ste_fwd(const float* x, const uint16_t* qtabs, int n, int h, int w, int hs, int vs, float* y, uint8_t* mask, int* err,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Writing files with restart intervals (libjpeg's restart_interval, Pillow's restart_marker_blocks): the
 * writing entry points above with `restart_interval` = Ri MCUs in scan order, 0..65535 (anything else is NIMG_ERR_ARG).  Behind every
 * Ri MCUs that another MCU follows the coder fills the current byte up with 1-bits, writes the marker FF D0 .. FF D7 (the k-th is
 * D(k mod 8), never stuffed) and predicts the next DC value of every component from 0.  Ri = 0, and the entry points without the
 * argument, write no marker: the same bytes as before.  Purely added: NIMG_ABI_VERSION stays.
 *   encode_restart          nimg_jpeg_encode with the markers in `out` and counted in `lengths`; the DRI segment of the header is the
 *                           caller's.  A segment is at most 4 bytes per marker longer than without.  The workspace is
 *                           nimg_jpeg_encode_restart_workspace_bytes, which nimg_jpeg_transform and nimg_jpeg_reconstruct accept too.
 *   histogram_restart       nimg_jpeg_histogram of the symbols nimg_jpeg_encode_restart emits: the DC differences at the start of an
 *                           interval differ, as in libjpeg's statistics pass.
 *   encode_tables_restart   nimg_jpeg_encode_tables with the markers; workspace nimg_jpeg_encode_tables_restart_workspace_bytes.  An
 *                           image whose tables are refused (status bit 1) is its markers alone.
 *   decode_restart          nimg_jpeg_decode of segments that carry the markers of `restart_interval` (the file's DRI value; all images
 *                           of a call share it).  The markers are taken out while the stuffing is, and every interval is an entry
 *                           point: its first subsequence starts from a known state, subsequences never straddle an interval, and
 *                           `rounds` is at most the subsequences of the image's longest interval - 1 (0 where every interval fits one
 *                           subsequence).  A run ends with its interval's blocks; what stands between them and the marker is skipped,
 *                           as libjpeg skips it.  Status bit 512: restart markers missing, surplus or out of sequence (the k-th must
 *                           be FF D(k mod 8), and there must be ceil(MCUs / Ri) - 1); the other bits as nimg_jpeg_decode's, "fewer
 *                           blocks" (32) and "bits beyond the end" (16) per interval.  Workspace:
 *                           nimg_jpeg_decode_restart_workspace_bytes.  restart_interval = 0 is nimg_jpeg_decode, where FF D0 .. D7
 *                           are markers like any other (bit 1). */
/* Writing progressive files (libjpeg's jpeg_simple_progression, Pillow's progressive=True): the ten scans of
 * one set of coefficients - DC first (Al 1, interleaved), Y 1-5 (Al 2), Cr 1-63 (Al 1), Cb 1-63 (Al 1), Y 6-63 (Al 2), Y 1-63 refine
 * (Al 1), DC refine (interleaved), Cr, Cb, Y 1-63 refine (Al 0) - each coded with a table of its own.  The ten tables of an image stand
 * in the order of the file's DHT segments: DC 00 (Y), DC 01 (Cb and Cr), then the AC tables of the scans 2, 3, 4, 5, 6, 8, 9, 10.
 * Geometry, coefficients, table layout and restart_interval as above; n <= 16383, and n == 0 does nothing.  A DC coefficient outside
 * +-2047 and an AC coefficient outside +-1023 are clamped to that before the point transform.  In a single-component scan the restart
 * interval counts blocks.  Purely added: NIMG_ABI_VERSION stays.
 *   progressive_histogram   coef -> hist (device) [n][10][257] uint32, zeroed by the call: how often each symbol of each table is
 *                           emitted, the EOBn symbols of the end-of-band runs included.  Entry 256 is 0.  nimg_jpeg_optimal_tables on
 *                           the 10 n histograms gives the tables libjpeg writes.
 *   encode_progressive      out: the ten entropy-coded segments of every image back to back - stuffed, padded, the restart markers
 *                           inside; headers, DHT, SOS and EOI are the caller's - none at or beyond out_capacity; lengths (device)
 *                           [n][10]: the bytes of each segment, capacity or not.  status (device) [n] as nimg_jpeg_encode_tables':
 *                           bits 1 = one of the ten tables is no prefix code (the image's segments are empty, or its markers alone) |
 *                           2 = a symbol that occurs has no code (it and its value bits are left out).  A block never exceeds 27
 *                           bits in a DC scan and 1580 in an AC scan; every store stays inside the workspace whatever the tables say. */
size_t nimg_jpeg_progressive_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval);
int nimg_jpeg_progressive_histogram(const int16_t* coef, int n, int h, int w, int hs, int vs, int restart_interval, uint32_t* hist,
                                    void* stream);
int nimg_jpeg_encode_progressive(const int16_t* coef, int n, int h, int w, int hs, int vs, int restart_interval, const uint8_t* tables,
                                 uint8_t* out, size_t out_capacity, uint32_t* lengths, uint32_t* status, void* workspace,
                                 size_t workspace_bytes, void* stream);

size_t nimg_jpeg_encode_restart_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval);
int nimg_jpeg_encode_restart(const int16_t* coef, int n, int h, int w, int hs, int vs, int restart_interval, uint8_t* out,
                             size_t out_capacity, uint32_t* lengths, void* workspace, size_t workspace_bytes, void* stream);
int nimg_jpeg_histogram_restart(const int16_t* coef, int n, int h, int w, int hs, int vs, int restart_interval, uint32_t* hist,
                                void* stream);
size_t nimg_jpeg_encode_tables_restart_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval);
int nimg_jpeg_encode_tables_restart(const int16_t* coef, int n, int h, int w, int hs, int vs, int restart_interval, const uint8_t* tables,
                                    uint8_t* out, size_t out_capacity, uint32_t* lengths, uint32_t* status, void* workspace,
                                    size_t workspace_bytes, void* stream);
size_t nimg_jpeg_decode_restart_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval, size_t ecd_bytes,
                                                int subseq_bits);
int nimg_jpeg_decode_restart(const uint8_t* ecd, const uint64_t* ecd_off, const uint8_t* huffman, int n, int h, int w, int hs, int vs,
                             int restart_interval, int subseq_bits, int16_t* coef, uint32_t* status, uint32_t* rounds, void* workspace,
                             size_t workspace_bytes, void* stream);

/* Reading progressive files: the entropy-coded segments of every scan of n files -> the coefficients of
 * nimg_jpeg_transform, with any legal scan script (T.81 G.1.1.1).  All images of a call share the geometry, the restart interval and
 * the script; tables and segments are per image.
 *   ecd, ecd_off   the segments back to back as they stand in the files (stuffed, restart markers inside), image-major: segment
 *                  image * n_scans + scan is the bytes [ecd_off[.], ecd_off[. + 1]) - n * n_scans + 1 offsets on the device.
 *   script         HOST, n_scans x 6 int32: component mask (bit c = component c; 7 = all three interleaved, DC scans only), Ss, Se,
 *                  Ah, Al, level.  1 <= n_scans <= 64.  A DC scan (Ss = Se = 0) holds one component or all three, an AC scan
 *                  (1 <= Ss <= Se <= 63) one; a coefficient's first scan has Ah = 0, every later one Ah = the Al before it and
 *                  Al = Ah - 1; a component's DC first scan precedes its AC scans; every coefficient of every component reaches
 *                  Al = 0; level = 1 + the highest level of an earlier scan of a shared component whose band overlaps (a scan reads
 *                  only what lower levels wrote; the scans of a level run side by side).  Anything else is NIMG_ERR_ARG before any
 *                  launch, as is a workspace too short for the batch.
 *   huffman        (device) [n][n_scans][3][272]: slot c = the table of the scan's c-th component (DC tables in a DC scan, the AC
 *                  table in an AC scan), 16 counts + 256 symbols; zero where the scan has none (DC refine scans have no symbols).
 *   coef, status   as nimg_jpeg_decode_restart; an image's status is the OR over its scans, the bits those of nimg_jpeg_decode and
 *                  512, and 1024: an end-of-band run beyond the blocks of its scan (of its restart interval).  In a single-component
 *                  scan the restart interval counts blocks.
 *   rounds         (device) [n][n_scans]: the synchronisation rounds of every first scan (Ah = 0), 0 for a refinement.
 * subseq_bits as nimg_jpeg_decode.  Purely added: NIMG_ABI_VERSION stays. */
size_t nimg_jpeg_decode_progressive_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval, int n_scans,
                                                    size_t ecd_bytes, int subseq_bits);
int nimg_jpeg_decode_progressive(const uint8_t* ecd, const uint64_t* ecd_off, const int32_t* script, int n_scans, const uint8_t* huffman,
                                 int n, int h, int w, int hs, int vs, int restart_interval, int subseq_bits, int16_t* coef,
                                 uint32_t* status, uint32_t* rounds, void* workspace, size_t workspace_bytes, void* stream);

/* Grey-scale files: a frame of ONE component, which imageio.imsave / imread (jpeg_helpers.py:97-101) write
 * and read for a mode 'L' image.  One entry per operation over the launchers of the colour entry points above, with
 *   no sampling factors   a one-component scan is never interleaved: one block is one MCU, the blocks stand in raster order over
 *                         ceil(h / 8) x ceil(w / 8), the right and bottom edges replicated; a restart interval counts blocks
 *   restart_interval      0..65535 on every coding entry, 0 = none (there is no _restart twin)
 *   x, y                  (n,h,w,1): the sample is the byte - no colour conversion, no up-sampling; float input through the same
 *                         conversion and batch-wide "any value above 1" flag as nimg_jpeg_transform
 *   coef                  int16 [image][block row][block col][64 zig-zag]
 *   qtabs                 (device) [.][1][64] uint16, natural order: the one table of the frame
 *   hist, tables          [n][2][257] and [n][2][272]: DC then AC (the DHT ids 00 10)
 *   huffman (decode)      [n][2][272]: DC, AC; (decode_progressive) [n][n_scans][3][272] with slot 0 alone in use, every scan's mask 1
 * Everything else - arguments, limits, status bits, rounds, what is clamped, the bounds of a segment - is that of the entry point named:
 *   grey_workspace_bytes                      nimg_jpeg_encode_restart_workspace_bytes (serves transform*, encode, reconstruct_tables)
 *   grey_transform                            nimg_jpeg_transform
 *   grey_transform_tables                     nimg_jpeg_transform_tables
 *   grey_encode                               nimg_jpeg_encode_restart (Annex K luma tables)
 *   grey_histogram                            nimg_jpeg_histogram_restart; nimg_jpeg_optimal_tables takes its 2 n histograms as they are
 *   grey_encode_tables (_workspace_bytes)     nimg_jpeg_encode_tables_restart (_workspace_bytes)
 *   grey_decode (_workspace_bytes)            nimg_jpeg_decode_restart (_workspace_bytes)
 *   grey_reconstruct_tables                   nimg_jpeg_reconstruct_tables
 *   grey_decode_progressive (_workspace_bytes)  nimg_jpeg_decode_progressive (_workspace_bytes)
 * No allocation, no synchronisation, capturable; n == 0 (n_src == n_items == 0) is a no-op; NIMG_ERR_ARG and NIMG_ERR_WORKSPACE come
 * before any launch.  Purely added: NIMG_ABI_VERSION stays, and every entry point above answers every argument as before. */
size_t nimg_jpeg_grey_workspace_bytes(int n, int h, int w, int restart_interval);
int nimg_jpeg_grey_transform(const void* x, int is_u8, int n, int h, int w, int quality, int16_t* coef, void* workspace,
                             size_t workspace_bytes, void* stream);
int nimg_jpeg_grey_transform_tables(const void* x, int is_u8, int n_src, int h, int w, const uint16_t* qtabs, int n_items, int16_t* coef,
                                    int* err, void* workspace, size_t workspace_bytes, void* stream);
int nimg_jpeg_grey_encode(const int16_t* coef, int n, int h, int w, int restart_interval, uint8_t* out, size_t out_capacity,
                          uint32_t* lengths, void* workspace, size_t workspace_bytes, void* stream);
int nimg_jpeg_grey_histogram(const int16_t* coef, int n, int h, int w, int restart_interval, uint32_t* hist, void* stream);
size_t nimg_jpeg_grey_encode_tables_workspace_bytes(int n, int h, int w, int restart_interval);
int nimg_jpeg_grey_encode_tables(const int16_t* coef, int n, int h, int w, int restart_interval, const uint8_t* tables, uint8_t* out,
                                 size_t out_capacity, uint32_t* lengths, uint32_t* status, void* workspace, size_t workspace_bytes,
                                 void* stream);
size_t nimg_jpeg_grey_decode_workspace_bytes(int n, int h, int w, int restart_interval, size_t ecd_bytes, int subseq_bits);
int nimg_jpeg_grey_decode(const uint8_t* ecd, const uint64_t* ecd_off, const uint8_t* huffman, int n, int h, int w, int restart_interval,
                          int subseq_bits, int16_t* coef, uint32_t* status, uint32_t* rounds, void* workspace, size_t workspace_bytes,
                          void* stream);
int nimg_jpeg_grey_reconstruct_tables(const int16_t* coef, int n, int h, int w, const uint16_t* qtabs, void* y, int out_u8, void* workspace,
                                      size_t workspace_bytes, void* stream);
size_t nimg_jpeg_grey_decode_progressive_workspace_bytes(int n, int h, int w, int restart_interval, int n_scans, size_t ecd_bytes,
                                                         int subseq_bits);
int nimg_jpeg_grey_decode_progressive(const uint8_t* ecd, const uint64_t* ecd_off, const int32_t* script, int n_scans, const uint8_t* huffman,
                                      int n, int h, int w, int restart_interval, int subseq_bits, int16_t* coef, uint32_t* status,
                                      uint32_t* rounds, void* workspace, size_t workspace_bytes, void* stream);

/* Scaled reconstruction: nimg_jpeg_reconstruct_tables at libjpeg's scale_num / scale_denom = 1 / scale, scale
 * 1, 2, 4 or 8 - the image libjpeg (Pillow's draft()) decodes from the same file at that scale, byte for byte: per component the
 * reduced inverse DCT of jidctred.c at the block size jdmaster.c gives it, for 4:2:2 the 2:1 up-sampling jdsample.c then chooses, the
 * unchanged colour conversion.
 *   y              (n, ceil(h / scale), ceil(w / scale), 3) - grey: (.., .., 1) -, uint8 if out_u8, else float32 = byte / 255
 *   coef, qtabs    as nimg_jpeg_reconstruct_tables (nimg_jpeg_grey_reconstruct_tables)
 *   _grey          the one-component form, without sampling factors, as the nimg_jpeg_grey_* entries are to theirs; the nimg_jpeg_grey_
 *                  names themselves stay the closed set of section 4p - one per operation of the full-size codec
 *   workspace      nimg_jpeg_reconstruct_scaled_workspace_bytes of the same geometry and scale; 0 = a geometry or scale not served
 * scale 1 IS nimg_jpeg_reconstruct_tables: its launches, its workspace size, its bytes.  A scale outside {1, 2, 4, 8} or a null pointer
 * is NIMG_ERR_ARG, a short workspace NIMG_ERR_WORKSPACE, both before any launch.  No allocation, no synchronisation, capturable; the
 * _grey forms take n == 0 as a no-op.  Purely added: NIMG_ABI_VERSION stays. */
size_t nimg_jpeg_reconstruct_scaled_workspace_bytes(int n, int h, int w, int hs, int vs, int scale);
int nimg_jpeg_reconstruct_scaled(const int16_t* coef, int n, int h, int w, int hs, int vs, const uint16_t* qtabs, int scale, void* y,
                                 int out_u8, void* workspace, size_t workspace_bytes, void* stream);
size_t nimg_jpeg_reconstruct_scaled_grey_workspace_bytes(int n, int h, int w, int scale);
int nimg_jpeg_reconstruct_scaled_grey(const int16_t* coef, int n, int h, int w, const uint16_t* qtabs, int scale, void* y, int out_u8,
                                      void* workspace, size_t workspace_bytes, void* stream);

/* Any sampling: the operations that read a file and write it again, over the same launchers, for colour files
 * whose luma sampling factors are 1x2 (4:4:0), 4x1 (4:1:1), 4x2 (4:1:0), 1x4 or 2x4 over 1x1 chroma - next to 1x1, 2x1 and 2x2, which
 * these entries serve with the launches and the bytes of their namesakes.  Every other entry point refuses the five as it did.  A
 * sampling outside the eight (a factor of 3, 4x4, ...) is NIMG_ERR_ARG before any launch; the size functions then return 0.
 *   sampling_decode                 nimg_jpeg_decode_restart, and its workspace size
 *   sampling_decode_progressive     nimg_jpeg_decode_progressive, and its workspace size
 *   sampling_reconstruct_tables     nimg_jpeg_reconstruct_tables: 1x2 is brought up by libjpeg's h1v2 triangle filter, the other four by
 *                                   replication; workspace nimg_jpeg_sampling_reconstruct_scaled_workspace_bytes at scale 1
 *   sampling_reconstruct_scaled     nimg_jpeg_reconstruct_scaled, and its workspace size: the chroma block may have up to 8 samples a
 *                                   side at any scale, and is brought up by the h2v1 or h1v2 filter or by replication as jdsample.c
 *                                   chooses for its ratios; scale 1 is nimg_jpeg_sampling_reconstruct_tables
 *   sampling_histogram              nimg_jpeg_histogram_restart
 *   sampling_encode_tables          nimg_jpeg_encode_tables_restart, and its workspace size
 * Arguments, results and error codes are their namesakes'.  Purely added: NIMG_ABI_VERSION stays. */
size_t nimg_jpeg_sampling_decode_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval, size_t ecd_bytes,
                                                 int subseq_bits);
int nimg_jpeg_sampling_decode(const uint8_t* ecd, const uint64_t* ecd_off, const uint8_t* huffman, int n, int h, int w, int hs, int vs,
                              int restart_interval, int subseq_bits, int16_t* coef, uint32_t* status, uint32_t* rounds, void* workspace,
                              size_t workspace_bytes, void* stream);
size_t nimg_jpeg_sampling_decode_progressive_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval, int n_scans,
                                                             size_t ecd_bytes, int subseq_bits);
int nimg_jpeg_sampling_decode_progressive(const uint8_t* ecd, const uint64_t* ecd_off, const int32_t* script, int n_scans,
                                          const uint8_t* huffman, int n, int h, int w, int hs, int vs, int restart_interval, int subseq_bits,
                                          int16_t* coef, uint32_t* status, uint32_t* rounds, void* workspace, size_t workspace_bytes,
                                          void* stream);
int nimg_jpeg_sampling_reconstruct_tables(const int16_t* coef, int n, int h, int w, int hs, int vs, const uint16_t* qtabs, void* y,
                                          int out_u8, void* workspace, size_t workspace_bytes, void* stream);
size_t nimg_jpeg_sampling_reconstruct_scaled_workspace_bytes(int n, int h, int w, int hs, int vs, int scale);
int nimg_jpeg_sampling_reconstruct_scaled(const int16_t* coef, int n, int h, int w, int hs, int vs, const uint16_t* qtabs, int scale, void* y,
                                          int out_u8, void* workspace, size_t workspace_bytes, void* stream);
int nimg_jpeg_sampling_histogram(const int16_t* coef, int n, int h, int w, int hs, int vs, int restart_interval, uint32_t* hist,
                                 void* stream);
size_t nimg_jpeg_sampling_encode_tables_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval);
int nimg_jpeg_sampling_encode_tables(const int16_t* coef, int n, int h, int w, int hs, int vs, int restart_interval, const uint8_t* tables,
                                     uint8_t* out, size_t out_capacity, uint32_t* lengths, uint32_t* status, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* Lossless transforms: the coefficients of n files of one geometry -> the coefficients of the files jpegtran
 * makes of them by a flip, a transposition, a rotation or an aligned crop, in one launch that moves every block once.  (The name:
 * nimg_jpeg_transform is the forward DCT.)
 *   coef           (n, real blocks, 64) int16 as nimg_jpeg_transform / nimg_jpeg_decode leave them: [Y | Cb | Cr][block row][block col][zig-zag]
 *   h, w, hs, vs   the source's geometry; nc = 3 with any of the eight luma samplings of the nimg_jpeg_sampling_* entries, or nc = 1, a
 *                  grey-scale file, with hs = vs = 1 (its iMCU is 8 x 8 whatever the file declares)
 *   op             0 none, 1 hflip, 2 vflip, 3 transpose, 4 transverse (the flip about the anti-diagonal), 5 rot90 (clockwise, jpegtran
 *                  -rotate 90), 6 rot180, 7 rot270.  As jtransform.c does it: a horizontal mirroring reverses the block columns of every
 *                  component and negates the coefficients of odd horizontal frequency, a vertical one the rows and odd vertical
 *                  frequencies, a transposition swaps block rows with columns and transposes every block; the rotations and transverse
 *                  are compositions of these, each carried out as one gather.  Negation is two's complement on 16 bits (-(-32768) stays);
 *                  the DC is never negated.  The four transposing operations swap h with w and hs with vs, and the caller transposes
 *                  every quantisation table.
 *   crop_*         a region of the source, cut before the operation; crop_w == 0 (all four 0): none.  crop_x must be a multiple of
 *                  8 hs and crop_y of 8 vs (jpegtran moves an unaligned origin silently: here it is refused), the region must lie inside
 *                  the image with crop_w, crop_h >= 1; the blocks at a new right or bottom edge keep their contents, as jpegtran's do.
 *   trim           a transform moves whole iMCUs, so (after the crop) hflip and rot270 need w % (8 hs) == 0, vflip and rot90
 *                  h % (8 vs) == 0, rot180 and transverse both - jtransform.c's trim_right_edge / trim_bottom_edge, restated on the
 *                  source.  0 (jpegtran -perfect): a file that does not is refused; 1 (-trim): that dimension is first cut down to the
 *                  multiple below it.  jpegtran's third way, the strip left in place untransformed, is not offered.
 *   out            (n, real blocks of the output geometry, 64) int16; out_h, out_w, out_hs, out_vs: that geometry (host ints)
 * nimg_jpeg_lossless_geometry computes the four on the host alone; a caller sizes `out` by it.  NIMG_ERR_ARG before any launch, with
 * `out` and the four untouched: an unknown op, factors outside the eight (or nc = 1 with others than 1 x 1), an unaligned crop or one
 * outside the image, a partial iMCU with trim == 0, a result of no pixels, a null pointer, n outside 1..65535 (nc = 1 takes n == 0 as a
 * no-op, as the nimg_jpeg_grey_* entries do).  No workspace, no allocation, no synchronisation, capturable.  Purely added:
 * NIMG_ABI_VERSION stays. */
int nimg_jpeg_lossless_geometry(int h, int w, int hs, int vs, int nc, int op, int crop_x, int crop_y, int crop_w, int crop_h, int trim,
                                int* out_h, int* out_w, int* out_hs, int* out_vs);
int nimg_jpeg_lossless(const int16_t* coef, int n, int h, int w, int hs, int vs, int nc, int op, int crop_x, int crop_y, int crop_w,
                       int crop_h, int trim, int16_t* out, int* out_h, int* out_w, int* out_hs, int* out_vs, void* stream);

/* Sign planes of the FAN's bf16-stored pooled activations: all that a layer's input gradient reads of the
 * activation in front of it is LeakyReLU', one bit per value.  A plane is (n, h, w, c / 8) bytes next to a bf16 tensor (n, h, w, c),
 * c % 8 == 0: bit e of byte c' / 8 is 1 iff the STORED bf16 value of channel c' + e is > 0 (-0, +0 and NaN give 0) - the predicate of
 * the act_mask arguments, so results do not change by a bit.  Purely added: the entry points without the argument are the ones with
 * a null plane, NIMG_ABI_VERSION stays.
 *   conv1_pool_fwd_c4_sign     nimg_conv1_pool_fwd_c4 + pool_sign (n, h/2, wd/2, 4), optional; needs out_bf16.
 *   conv2d_pool_fwd_bf16_sign  nimg_conv2d_pool_fwd_bf16_ex + pool_sign (n, h/2, wd/2, cout / 8), optional.  Only the 5x5 ring kernels
 *                              write it: NIMG_ERR_ARG where nimg_conv2d_pool_sign_ok(the same arguments) is 0.
 *   conv2d_fwd_bf16_unpool_sign  nimg_conv2d_fwd_bf16_unpool + act_sign, the plane of act_mask (optional; act_mask stays required and
 *                              bf16, the output bf16, o1 % 8 == 0, else NIMG_ERR_ARG).  The ring kernels read the plane instead of
 *                              the mask - a sixteenth of the bytes -, every other route reads the mask. */
int nimg_conv1_pool_fwd_c4_sign(const void* c4, const float* w, const float* bias, void* pooled, unsigned char* pool_idx,
                                unsigned char* pool_sign, int n, int h, int wd, float alpha, int out_bf16, void* stream);
int nimg_conv2d_pool_sign_ok(int cin, int cout, int n, int h, int wd, int ks, int flags);
int nimg_conv2d_pool_fwd_bf16_sign(const float* in, int cin, const float* w, const void* wb, const float* bias,
                                   float* pool_out, unsigned char* pool_idx, unsigned char* pool_sign, int cout, int n, int h,
                                   int wd, int ks, int act, float alpha, int flags, void* stream);
int nimg_conv2d_fwd_bf16_unpool_sign(const void* in_pooled, const unsigned char* in_idx, int c1, const void* wb, const float* bias,
                                     float* out1, int o1, const float* act_mask, const unsigned char* act_sign, int n, int h, int wd,
                                     int ks, int pad_t, int pad_l, int hout, int wout, int act, float alpha, int flags,
                                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NIMG_H */
