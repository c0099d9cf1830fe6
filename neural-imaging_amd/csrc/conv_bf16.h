// Shared by the conv_bf16*.hip translation units (throughput mode of the convolutions, see conv_bf16.hip): the kernel
// parameter block and the vector epilogue of the forward / input-gradient kernels, and the host functions that cross those
// files (the weight gradient's share: conv_bf16_wgrad.h).  The kernel templates live in conv_bf16_tile.h / _ring.h / _dma.h; each
// conv_bf16_k*.hip instantiates the dispatch of its own kernel sizes and nothing else.
#pragma once
#include <stdlib.h>

#include <cstdlib>
#include "common.h"

// The fields of ConvParamsB, with external linkage: what conv_bf16_dispatch / conv_bf16_launch_16x16 carry from one
// translation unit to another.  The kernels keep taking the file-local ConvParamsB below (their names do not change).
struct ConvArgsB {
    const float* in1;
    const float* in2;
    const __bf16* wb;     // [CinP/16][KS*KS][Cout][16]
    const float* bias;
    float* out1;
    float* out2;
    const float* act1;
    float* pool_out;            // optional fused activation + 2x2 max-pool output (replaces out1), see common.h
    unsigned char* pool_idx;
    int C1, C2, O1, O2, CinP;
    int N, H, W, Hout, Wout, pad_t, pad_l;
    int tiles_y, tiles_x, act, pad_mode;
    float alpha;
    int convt;            // 1: Conv2DTranspose(2x2, stride 2) as four 1x1 products; workgroup id & 3 = output phase (dy, dx)
    int flags;            // NIMG_BF16_IN: in1 (and in2) hold bf16; _OUT: out1 / out2 / pool_out are bf16; _MASK: act1 is bf16
    const unsigned char* in_idx;   // UNP kernels: in1 is the POOLED tensor (N, H/2, W/2, C1) bf16 and in_idx its arg-max bytes;
                                   // the convolution runs on their 2x2 un-pooling (H x W), built while staging
    const float* res;              // optional float32 tensor of out1's shape added to the result (after bias, activation and mask):
                                   // the skip connection of a residual block, forward and backward (3x3, float32 output)
    float* out1b;                  // optional SECOND copy of out1 as bf16 (float32 out1 only): the running float32 sum of a residual
                                   // stream stays exact while its consumers - convolutions and weight gradients, which round to
                                   // bf16 anyway - read half the bytes through the bf16-input kernels
    // Sign planes of bf16-stored pooled activations, (N, H, W, C / 8) bytes: bit e of byte c / 8 = (value of channel c + e > 0), the
    // predicate of the LeakyReLU' mask (-0, +0 and NaN give 0).  Ring kernels only (conv_bf16_ring.h); null = not used.
    unsigned char* pool_sign = nullptr;         // written next to pool_out (bf16-stored), from the values as stored
    const unsigned char* act_sign = nullptr;    // read INSTEAD of act1 (which stays set: every other route masks with it)
};

namespace {

using namespace nimg;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ bf16x8 pack8(const float (&f)[8]) {
    bf16x8 r;
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = (__bf16)f[k];
    return r;
}

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store4_bf16(float* base_as_bf16, long elem, float4 v) {
    bf16x4 o;
    o[0] = (__bf16)v.x; o[1] = (__bf16)v.y; o[2] = (__bf16)v.z; o[3] = (__bf16)v.w;
    *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(base_as_bf16) + elem) = o;
}
__device__ __forceinline__ float4 load4_bf16(const float* base_as_bf16, long elem) {
    const bf16x4 o = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const __bf16*>(base_as_bf16) + elem);
    return make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
}

struct ConvParamsB : ConvArgsB {};      // what the kernels and their launch functions take

__device__ __forceinline__ unsigned unp_eq_bytes(unsigned k, unsigned pos) {          // 0xFF in every byte of k equal to pos
    const unsigned x = k ^ (pos * 0x01010101u);
    return (((x | (x >> 1)) & 0x01010101u) ^ 0x01010101u) * 0xFFu;
}
__device__ __forceinline__ uint4 unp_route(uint4 g, unsigned k0, unsigned k1, unsigned pos) {
    const unsigned m0 = unp_eq_bytes(k0, pos), m1 = unp_eq_bytes(k1, pos);
    return make_uint4(g.x & __builtin_amdgcn_perm(m0, m0, 0x01010000u), g.y & __builtin_amdgcn_perm(m0, m0, 0x03030202u),
                      g.z & __builtin_amdgcn_perm(m1, m1, 0x01010000u), g.w & __builtin_amdgcn_perm(m1, m1, 0x03030202u));
}

// Vector epilogue shared by the convolution kernels: the accumulators of a wave (MI x NI fragments of 32 pixels x 32 channels)
// are turned around through the wave's LDS scratch so that each lane stores 16 B along the NHWC channel axis; bias, activation,
// previous-layer LeakyReLU' mask, residual, bf16 copy and the depth_to_space / space_to_depth output layouts are applied on the
// way (ConvParamsB).  Requires O1 % 4 == 0 and O2 % 4 == 0; contains one workgroup barrier (the scratch aliases the tiles).
// The eight biases a lane adds in the 8-wide epilogue below are the same on every call (channels 8 (lane % (4 NI)) .. + 7 of the
// wave's strip): the kernels request them at their START (EpiBias), so the epilogue of a workgroup that has its SIMDs to itself
// does not open with a memory round trip (conv3_rows.hip: that round trip was 20 % of a byte-bound layer).
struct EpiBias { float b[8]; };
template <int NI>
__device__ __forceinline__ EpiBias epi_bias_preload(const ConvParamsB& p, int lane, int wn, int co0, int Cout) {
    EpiBias r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r.b[e] = 0.f;
    const int co = co0 + wn * NI * 32 + (lane % (NI * 4)) * 8;
    if (p.bias && co + 7 < Cout) {
        const int cb = (p.flags & NIMG_D2S_CONVT) ? co % (p.O1 >> 2) : co;
        const float4 b0 = *reinterpret_cast<const float4*>(p.bias + cb), b1 = *reinterpret_cast<const float4*>(p.bias + cb + 4);
        r.b[0] = b0.x; r.b[1] = b0.y; r.b[2] = b0.z; r.b[3] = b0.w; r.b[4] = b1.x; r.b[5] = b1.y; r.b[6] = b1.z; r.b[7] = b1.w;
    }
    return r;
}

// Which tile pixel row P of the workgroup's M dimension is (fragment P >> 5, lane P & 31).  PMAP 0: row-major over (image, y, x) -
// a fragment = 32 consecutive tile pixels (two rows of a 16-wide tile).  PMAP 1 (conv3_dma_kernel's plane layout): a 16 x 16
// tile's fragment = 8 columns x 4 rows (fragment = column half + 2 x row group), an 8 x 8 x 4-image tile's fragment = ONE row
// of all four images (lane = 8 image + x) - the maps whose 16-lane ds_read_b128 groups meet 16 different bank quads.
template <int TH, int TW, int NB, int PMAP>
__device__ __forceinline__ void tile_pixel(int P, int& img, int& dy, int& dx) {
    if constexpr (PMAP == 0) {
        img = P / (TH * TW);
        const int rem = P % (TH * TW);
        dy = rem / TW;
        dx = rem % TW;
    } else if constexpr (NB == 1) {
        static_assert(TH == 16 && TW == 16, "plane layout: 16 x 16 tile");
        const int f = P >> 5, l = P & 31;
        img = 0;
        dy = 4 * (f >> 1) + (l >> 3);
        dx = 8 * (f & 1) + (l & 7);
    } else {
        static_assert(TH == 8 && TW == 8 && NB == 4, "plane layout: 8 x 8 x 4 tile");
        img = (P & 31) >> 3;
        dy = P >> 5;
        dx = P & 7;
    }
}

template <int KS, int TH, int TW, int NB, int MI, int NI, int PMAP = 0>
__device__ __forceinline__ void conv_epilogue_vec(const f32x16 (&acc)[MI][NI], const ConvParamsB& p, unsigned char* smem_raw,
                                                  int wave, int lane, int wm, int wn, int co0, int Cout, int ty0, int tx0,
                                                  int grp, int phase, const EpiBias& pre_) {
#ifdef NIMG_NO_EPI_PRELOAD                      // A/B: the biases requested where the epilogue starts, as before round 5
    const EpiBias pre = epi_bias_preload<NI>(p, lane, wn, co0, Cout);
    (void)pre_;
#else
    const EpiBias& pre = pre_;
#endif
    float* elds = reinterpret_cast<float*>(smem_raw) + wave * (32 * (NI * 32 + EPI_PAD));
    __syncthreads();                    // the scratch aliases the tiles: everyone is done reading them; from here on every
                                        // wave works in its own region (wave-level ordering only)
#ifndef NIMG_NO_EPI8
    // bf16-stored outputs (and mask) in the plain layout - the UNet's and the codec's inner layers: eight channels per lane,
    // 16-byte stores / mask loads (the store-issue rate, not the bytes, bounds a row-per-lane epilogue)
    // NIMG_UNPOOL_OUT: the result is the gradient of a 2x2 max-pool's OUTPUT (the UNet's encoder levels, pipelines.py:160-173
    // backward): every value goes to the first maximum of its window of the stored activation act1 (n, 2 hout, 2 wout, o1), the
    // skip gradient `res` (same shape, bf16, optional; may be out1 itself) is added to all four positions, LeakyReLU'(act1)
    // applied (act == 1) - maxpool2_bwd_bf16_kernel's arithmetic on the value this kernel would have stored as bf16
    if (p.flags & NIMG_UNPOOL_OUT) {
        const __bf16* ya = reinterpret_cast<const __bf16*>(p.act1);
        const __bf16* sk = reinterpret_cast<const __bf16*>(p.res);
        __bf16* dzo = reinterpret_cast<__bf16*>(p.out1);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            epilogue_via_lds8<NI>(acc[mi], elds, lane, [&](int row, int c, float4 lo, float4 hi) {
                const int co = co0 + wn * NI * 32 + c;
                if (co >= Cout) return;
                const int P = (wm * MI + mi) * 32 + row;
                int img, dy_, dx_;
                tile_pixel<TH, TW, NB, PMAP>(P, img, dy_, dx_);
                const int oy = ty0 + dy_, ox = tx0 + dx_, n = grp * NB + img;
                if (n >= p.N || oy >= p.Hout || ox >= p.Wout) return;
                const float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                const long W2 = 2L * p.Wout;
                const long base = (((long)n * 2 * p.Hout + 2 * oy) * W2 + 2 * ox) * p.O1 + co;
                const long offs[4] = {0, (long)p.O1, W2 * p.O1, W2 * p.O1 + p.O1};
                bf16x8 v[4], a[4], o[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[q] = *reinterpret_cast<const bf16x8*>(ya + base + offs[q]);
                    if (sk) a[q] = *reinterpret_cast<const bf16x8*>(sk + base + offs[q]);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float g = (float)(__bf16)f[e];
                    const float v0 = (float)v[0][e], v1 = (float)v[1][e], v2 = (float)v[2][e], v3 = (float)v[3][e];
                    const float m = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
                    const int sel = v0 == m ? 0 : (v1 == m ? 1 : (v2 == m ? 2 : 3));
                    const float vv[4] = {v0, v1, v2, v3};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float t = (q == sel) ? g : 0.f;
                        if (sk) t += (float)a[q][e];
                        if (p.act == 1) t *= (vv[q] > 0.f ? 1.0f : p.alpha);
                        o[q][e] = (__bf16)t;
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) *reinterpret_cast<bf16x8*>(dzo + base + offs[q]) = o[q];
            });
        }
        return;
    }
    // NIMG_D2S_CONVT: Conv2DTranspose(2x2, stride 2) as one 1x1 product over 4 x cout columns (nimg_convt2x2_fwd_bf16_ex) - column
    // block b holds output phase 3 - b (the weight image lists the taps flipped), which goes to pixel (2 y + dy, 2 x + dx)
    if (p.flags & NIMG_D2S_CONVT) {
        const int cd = p.O1 >> 2;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            epilogue_via_lds8<NI>(acc[mi], elds, lane, [&](int row, int c, float4 lo, float4 hi) {
                const int co = co0 + wn * NI * 32 + c;
                if (co >= Cout) return;
                const int P = (wm * MI + mi) * 32 + row;
                int img, dy_, dx_;
                tile_pixel<TH, TW, NB, PMAP>(P, img, dy_, dx_);
                const int oy = ty0 + dy_, ox = tx0 + dx_, n = grp * NB + img;
                if (n >= p.N || oy >= p.Hout || ox >= p.Wout) return;
                const int blk = co / cd, cc = co - blk * cd, ph = 3 - blk;
                const long o = (((long)n * 2 * p.Hout + 2 * oy + (ph >> 1)) * (2 * p.Wout) + 2 * ox + (ph & 1)) * cd + cc;
                float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                if (p.bias) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] += pre.b[e];
                }
                *reinterpret_cast<bf16x8*>(reinterpret_cast<__bf16*>(p.out1) + o) = pack8(f);
            });
        }
        return;
    }
    if ((p.flags & NIMG_BF16_OUT) && !(p.flags & (NIMG_D2S_OUT | NIMG_S2D_OUT)) && !p.res && !p.out1b &&
        (!p.act1 || (p.flags & NIMG_BF16_MASK)) && (p.O1 & 7) == 0 && (p.O2 & 7) == 0) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            epilogue_via_lds8<NI>(acc[mi], elds, lane, [&](int row, int c, float4 lo, float4 hi) {
                const int co = co0 + wn * NI * 32 + c;
                if (co >= Cout) return;
                const int P = (wm * MI + mi) * 32 + row;
                int img, dy_, dx_;
                tile_pixel<TH, TW, NB, PMAP>(P, img, dy_, dx_);
                const int oy = ty0 + dy_, ox = tx0 + dx_, n = grp * NB + img;
                if (n >= p.N || oy >= p.Hout || ox >= p.Wout) return;
                const long pixoff = (KS == 1 && p.convt)
                    ? ((long)n * 2 * p.Hout + 2 * oy + (phase >> 1)) * (2 * p.Wout) + 2 * ox + (phase & 1)
                    : ((long)n * p.Hout + oy) * p.Wout + ox;
                float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                if (p.bias) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] += pre.b[e];
                }
                if (p.act == 1) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] = lrelu(f[e], p.alpha);
                }
                if (co < p.O1) {
                    const long o = pixoff * p.O1 + co;
                    if (p.act1) {
                        const bf16x8 m = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const __bf16*>(p.act1) + o);
#pragma unroll
                        for (int e = 0; e < 8; ++e) f[e] *= (float)m[e] > 0.f ? 1.0f : p.alpha;
                    }
                    *reinterpret_cast<bf16x8*>(reinterpret_cast<__bf16*>(p.out1) + o) = pack8(f);
                } else {
                    *reinterpret_cast<bf16x8*>(reinterpret_cast<__bf16*>(p.out2) + pixoff * p.O2 + (co - p.O1)) = pack8(f);
                }
            });
            // NIMG_POOL_ALSO: the 2x2 max-pooled tensor next to the full one (the UNet's encoder keeps the full tensor for its skip
            // connection and feeds the pooled one to the next level): a fragment = two rows of 16 pixels = 8 windows per channel
            if constexpr (TW == 16 && NB == 1 && PMAP == 0)
                if (p.pool_out) {
                    const int Hp = p.Hout >> 1, Wp = p.Wout >> 1, py = (ty0 >> 1) + wm * MI + mi;
                    pool_in_regs8<NI>(acc[mi], elds, lane, p.act == 1 ? p.alpha : 1.0f,
                        [&](int c) { const int co = co0 + wn * NI * 32 + c; return (p.bias && co < Cout) ? p.bias[co] : 0.f; },
                        [&](int pc, int c, float4 lo, float4 hi, uint2 k) {
                            const int co = co0 + wn * NI * 32 + c, px = (tx0 >> 1) + pc;
                            if (co >= Cout || grp >= p.N || py >= Hp || px >= Wp) return;
                            const long o = (((long)grp * Hp + py) * Wp + px) * Cout + co;
                            const float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                            *reinterpret_cast<bf16x8*>(reinterpret_cast<__bf16*>(p.pool_out) + o) = pack8(f);
                            if (p.pool_idx) *reinterpret_cast<uint2*>(p.pool_idx + o) = k;
                        });
                }
        }
        return;
    }
#endif
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        epilogue_via_lds<NI, false>(acc[mi], elds, lane, [&](int row, int c, float4 v) {
            const int co = co0 + wn * NI * 32 + c;
            if (co >= Cout) return;
            const int P = (wm * MI + mi) * 32 + row;
            int img, dy_, dx_;
            tile_pixel<TH, TW, NB, PMAP>(P, img, dy_, dx_);
            const int oy = ty0 + dy_, ox = tx0 + dx_, n = grp * NB + img;
            if (n >= p.N || oy >= p.Hout || ox >= p.Wout) return;
            const long pixoff = (KS == 1 && p.convt)
                ? ((long)n * 2 * p.Hout + 2 * oy + (phase >> 1)) * (2 * p.Wout) + 2 * ox + (phase & 1)
                : ((long)n * p.Hout + oy) * p.Wout + ox;
            if (p.bias) {
                const float4 b = *reinterpret_cast<const float4*>(p.bias + co);
                v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
            }
            if (p.act == 1) {
                v.x = lrelu(v.x, p.alpha); v.y = lrelu(v.y, p.alpha); v.z = lrelu(v.z, p.alpha); v.w = lrelu(v.w, p.alpha);
            }
            if (co < p.O1) {
                long o = pixoff * p.O1 + co;
                const long om_conv = o;            // NIMG_MASK_CONV: the mask keeps the convolution's own layout
                if (p.flags & NIMG_D2S_OUT) {      // depth_to_space(2): channel block (2 dy + dx) of pixel (oy, ox) is pixel
                    const int cd = p.O1 >> 2, blk = co / cd;                 // (2 oy + dy, 2 ox + dx) of the output
                    o = (((long)n * 2 * p.Hout + 2 * oy + (blk >> 1)) * (2 * p.Wout) + 2 * ox + (blk & 1)) * cd + (co - blk * cd);
                }
                if (p.act1) {
                    const long om = (p.flags & NIMG_MASK_CONV) ? om_conv : o;
                    const float4 m = (p.flags & NIMG_BF16_MASK) ? load4_bf16(p.act1, om)
                                                                : *reinterpret_cast<const float4*>(p.act1 + om);
                    v.x *= m.x > 0.f ? 1.0f : p.alpha; v.y *= m.y > 0.f ? 1.0f : p.alpha;
                    v.z *= m.z > 0.f ? 1.0f : p.alpha; v.w *= m.w > 0.f ? 1.0f : p.alpha;
                }
                if (p.res) {
                    const float4 r = *reinterpret_cast<const float4*>(p.res + o);
                    v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
                }
                if (p.flags & NIMG_S2D_OUT)        // space_to_depth(2): pixel (oy, ox) is channel block 2 (oy & 1) + (ox & 1) of
                    o = (((long)n * (p.Hout >> 1) + (oy >> 1)) * (p.Wout >> 1) + (ox >> 1)) * (4 * p.O1) +    // pixel (oy/2, ox/2);
                        (2 * (oy & 1) + (ox & 1)) * p.O1 + co;                  // mask and residual keep the convolution's layout
                if (p.out1b) {
                    float4 c = v;
                    if (p.flags & NIMG_COPY_LRELU) { c.x = lrelu(c.x, p.alpha); c.y = lrelu(c.y, p.alpha); c.z = lrelu(c.z, p.alpha); c.w = lrelu(c.w, p.alpha); }
                    store4_bf16(p.out1b, o, c);
                }
                if (p.flags & NIMG_BF16_OUT) store4_bf16(p.out1, o, v);
                else *reinterpret_cast<float4*>(p.out1 + o) = v;
            } else {
                if (p.flags & NIMG_BF16_OUT) store4_bf16(p.out2, pixoff * p.O2 + (co - p.O1), v);
                else *reinterpret_cast<float4*>(p.out2 + pixoff * p.O2 + (co - p.O1)) = v;
            }
        });
    }
}

}  // namespace

// ---- host functions that cross the conv_bf16*.hip files --------------------------------------------------------------
// dispatch_b_t<KS, STRIDE, INB> (conv_bf16_tile.h) of one kernel size; instantiated in conv_bf16_k*.hip
template <int KS, int STRIDE, bool INB>
int conv_bf16_dispatch(const ConvArgsB& a, hipStream_t s);
// launch_conv_b<KS, 1, 16, 16, 1, tn32 ? 32 : 64, INB>: the tile the fused conv + pool entry (conv_bf16_packed.hip) asks for
template <int KS, bool INB>
int conv_bf16_launch_16x16(const ConvArgsB& a, bool tn32, hipStream_t s);
// the TN of the ring kernel conv_bf16_launch_16x16<5, true> hands this layer to, 0 if it goes elsewhere (who may ask for pool_sign)
int conv_bf16_pool_ring_tn(const ConvArgsB& a, bool tn32);
