// The generic tile kernel of the throughput-mode convolutions (conv_fwd_bf16_kernel) and the dispatch over all forward /
// input-gradient kernels: launch_conv_b picks ring, LDS-DMA or tile kernel for one tile shape, dispatch_b_t the tile shape.
// Included by the conv_bf16_k*.hip files only: every instantiation of these templates is a kernel to compile.
#pragma once
#include "conv_bf16_dma.h"
#include "conv_bf16_ring.h"

namespace {

// INB: in1 is stored as bf16 (compile-time: a run-time branch around the prefetch loads makes the backend wait for them at
// the join, which serialises the staging latency the async-stage split hides)
// BUF (with INB, one input tensor, Cin % 16 == 0, Cout % TN == 0, tensors < 2 GB): the prefetch goes through buffer
// descriptors - per-lane byte offsets resolved once per tile, the channel chunk in the scalar offset, padding pixels as
// out-of-range offsets that the hardware answers with zeros.  hipcc wraps every predicated flat load in s_and_saveexec /
// branch / zero-fill / 64-bit address arithmetic (~9 instructions x 17 loads per thread and chunk, issued in front of the
// MFMA loop); a buffer load is one instruction.
// UNP (with BUF): in1 is a POOLED gradient + arg-max bytes; a halo pixel (y, x) reads pooled pixel (y/2, x/2) and keeps channel
// c iff argmax == 2 (y & 1) + (x & 1) - the MaxPool2D routing as a packed byte-mask operation on the staged 16 bytes, so the
// full-resolution gradient (4x the bytes, 3/4 of them zeros) is never written to HBM nor read back.
template <int KS, int STRIDE, int TH, int TW, int NB, int TN, bool INB, bool BUF = false, bool UNP = false, int CKT = 16>
__global__ __launch_bounds__(256) void conv_fwd_bf16_kernel(const ConvParamsB p) {
    // K chunk: 16 channels (one MFMA k-step per tap).  -DNIMG_CK32 stages 32 channels (two k-steps, half the barriers) for the
    // 3x3 layers with float32 tensors (UNet / TwitterDCN) - measured on the bench step: the 8x8 bottleneck variant gains 12 %
    // (43 -> 38 us) but the 16x16 variants LOSE 4-22 % (47 -> 49 / 58 us: twice the LDS per workgroup and 84 staging registers
    // cost more than the halved barrier count returns), -5 % on the whole step - so it stays an experiment switch.
    // CKT = 64 (1x1 kernels with Cin % 64 == 0: FAN conv5, the UNet's Conv2DTranspose): a 1x1 layer has ONE tap per chunk, i.e.
    // 4 MFMAs per wave between two barriers with 16-channel chunks; 64 channels make it 16.
#ifdef NIMG_CK32
    constexpr int CK = CKT != 16 ? CKT : ((KS == 3 && !INB && !BUF) ? 32 : 16);
#else
    constexpr int CK = CKT;
#endif
    static_assert(CK == 16 || CK == 32 || (CK == 64 && KS == 1 && !BUF), "K chunk");
    constexpr int CKH = CK / 8;                          // 16-byte slots (8 channels) per pixel / weight row
    static_assert(!UNP || (INB && BUF && STRIDE == 1), "un-pooling input: bf16 buffer-load path only");
    constexpr int THH = (TH - 1) * STRIDE + KS, TWH = (TW - 1) * STRIDE + KS;
    constexpr int NPIXH = NB * THH * TWH;
    constexpr int MFRAGS = NB * TH * TW / 32, NFRAGS = TN / 32;
    constexpr int WAVES_M = MFRAGS >= 4 ? 4 : MFRAGS, WAVES_N = 4 / WAVES_M;
    constexpr int MI = MFRAGS / WAVES_M, NI = NFRAGS / WAVES_N;
    constexpr int TAPS = KS * KS;
    static_assert(NI >= 1 && MFRAGS % WAVES_M == 0, "bad tile configuration");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    // A tile layouts.  PLANAR (stride 1, 16-wide tiles): [k-half][row][32 columns] - 16 consecutive lanes read 256
    // contiguous bytes, the row stride is a multiple of 256 bytes so the four 16-lane groups of a ds_read_b128 each cover
    // all 64 banks exactly once, and a tap is a compile-time offset (ky*32 + kx) on one per-fragment base register.
    // Otherwise: [pixel][2] 16-byte halves, XOR-swizzled by pixel.
    constexpr bool PLANAR = (STRIDE == 1 && TW == 16 && NB == 1 && KS == 5);   // 3x3: the extra registers cost a wave per SIMD
    constexpr int PLSZ = THH * 32, A_ENTRIES = PLANAR ? 2 * PLSZ : NPIXH * CKH;
    uint4* sA = reinterpret_cast<uint4*>(smem_raw);
    uint4* sB = sA + A_ENTRIES;                                           // [TAPS*TN][CKH]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WAVES_M, wn = wave / WAVES_M;
    const int Cin = p.C1 + p.C2, Cout = p.O1 + p.O2;
    const int cot = (Cout + TN - 1) / TN;
    int bid = xcd_order(blockIdx.x);
    int phase = 0;                                       // Conv2DTranspose: which of the 2x2 output phases
    if (KS == 1 && p.convt) { phase = bid & 3; bid >>= 2; }
    const int co0 = (bid % cot) * TN;
    bid /= cot;
    const int tiles = p.tiles_y * p.tiles_x;
    const int tile = bid % tiles, grp = bid / tiles;
    const int ty0 = (tile / p.tiles_x) * TH, tx0 = (tile % p.tiles_x) * TW;
    const int iy0 = ty0 * STRIDE - p.pad_t, ix0 = tx0 * STRIDE - p.pad_l;
    const int half = lane >> 5;
    const EpiBias epi_pre = epi_bias_preload<NI>(p, lane, wn, co0, Cout);       // in flight under the whole main loop

    int abase[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int P = (wm * MI + mi) * 32 + (lane & 31);
        const int img = P / (TH * TW), rem = P % (TH * TW);
        abase[mi] = PLANAR ? half * PLSZ + (rem / TW) * 32 + (rem % TW)
                           : img * (THH * TWH) + (rem / TW) * STRIDE * TWH + (rem % TW) * STRIDE;
    }
    f32x16 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[mi][ni][j] = 0.0f;

    // Async-stage split (issue early / write late): the global loads of chunk c+1 are issued into registers before the
    // MFMA loop of chunk c and committed to LDS after it, so HBM/L2 latency hides under the matrix work.
    constexpr int AP = (NPIXH * CKH + 255) / 256, BP = (TAPS * TN * CKH + 255) / 256;
    float4 preA[AP][2];
    uint4 preB[BP];
    // The halo-pixel -> image-pixel map (padding mode, tile clipping, image index) does not depend on the channel chunk:
    // resolve it ONCE per workgroup.  Left inside fetch() it was ~700 instructions of branchy address arithmetic per
    // chunk in front of every MFMA loop (in-order issue: as long as the 100 MFMAs themselves).
    int apix[AP];
    unsigned upos[UNP ? AP : 1];                         // UNP: position of the halo pixel inside its 2x2 pooling window
    typedef unsigned int u32x2k __attribute__((ext_vector_type(2)));
    u32x2k preK[UNP ? AP : 1];                           // UNP: the 8 arg-max bytes of the staged 8 channels
#pragma unroll
    for (int q = 0; q < AP; ++q) {
        const int item = tid + q * 256;
        const int pix = item / CKH;
        const int img = pix / (THH * TWH), rem = pix % (THH * TWH);
        int gy = iy0 + rem / TWH, gx = ix0 + rem % TWH;
        const int n = grp * NB + img;
        const bool ok = item < NPIXH * CKH && n < p.N && map_coord(gy, p.H, p.pad_mode) && map_coord(gx, p.W, p.pad_mode);
        if constexpr (UNP) {
            apix[q] = ok ? (n * (p.H >> 1) + (gy >> 1)) * (p.W >> 1) + (gx >> 1) : -1;
            upos[q] = (unsigned)(((gy & 1) << 1) | (gx & 1));
        } else {
            apix[q] = ok ? (n * p.H + gy) * p.W + gx : -1;
        }
    }
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    unsigned aoff[AP];                                   // BUF: byte offset of this thread's 16 B inside the input tensor
    unsigned boff0 = 0, boff_last = 0;
    if constexpr (BUF) {
        static_assert(INB && 128 % TN == 0, "buffer prefetch: bf16-stored input, TN divides 128");
#pragma unroll
        for (int q = 0; q < AP; ++q)
            aoff[q] = apix[q] >= 0 ? (unsigned)((apix[q] * p.C1 + (tid & 1) * 8) * 2) : 0x80000000u;
        const int row = tid >> 1;
        boff0 = (unsigned)((((row / TN) * Cout + co0 + row % TN) * 16 + (tid & 1) * 8) * 2);
        boff_last = (tid + (BP - 1) * 256 < TAPS * TN * 2) ? boff0 : 0x80000000u;
    }
    auto fetch = [&](int c0) {
        if constexpr (BUF) {
            const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float*>(p.in1), 0, (int)(((long)p.N * p.H * p.W * p.C1 * 2) >> (UNP ? 2 : 0)), 0x00020000);
            const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<__bf16*>(p.wb), 0, (int)((long)(p.CinP >> 4) * TAPS * 16 * Cout * 2), 0x00020000);
#pragma unroll
            for (int q = 0; q < AP; ++q) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(ra, aoff[q], c0 * 2, 0);
                preA[q][0] = *reinterpret_cast<const float4*>(&v);
            }
            if constexpr (UNP) {
                const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<unsigned char*>(p.in_idx), 0, (int)(((long)p.N * p.H * p.W * p.C1) >> 2), 0x00020000);
#pragma unroll
                for (int q = 0; q < AP; ++q)        // byte offsets are half the bf16 offsets; padding stays out of range
                    preK[q] = __builtin_amdgcn_raw_buffer_load_b64(rk, aoff[q] >= 0x80000000u ? 0x80000000u : aoff[q] >> 1, c0, 0);
            }
            const int chunk_base = (c0 >> 4) * (TAPS * 16 * 2) * Cout, qstride = (128 / TN) * Cout * 32;
#pragma unroll
            for (int q = 0; q < BP; ++q) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rb, q == BP - 1 ? boff_last : boff0,
                                                                      chunk_base + q * qstride, 0);
                preB[q] = *reinterpret_cast<const uint4*>(&v);
            }
            return;
        }
        const int c = c0 + (tid & (CKH - 1)) * 8;       // item = tid + 256 q: the 8-channel slot is fixed per thread
#pragma unroll
        for (int q = 0; q < AP; ++q) {
            preA[q][0] = preA[q][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (apix[q] >= 0 && c < Cin) {
                const long pixoff = apix[q];
                if constexpr (INB) {                 // the tensors already hold bf16: 16 bytes = this item's 8 channels
                    const __bf16* src = c < p.C1 ? reinterpret_cast<const __bf16*>(p.in1) + pixoff * p.C1 + c
                                                 : reinterpret_cast<const __bf16*>(p.in2) + pixoff * p.C2 + (c - p.C1);
                    preA[q][0] = *reinterpret_cast<const float4*>(src);
                } else {
                    const float* src = c < p.C1 ? p.in1 + pixoff * p.C1 + c : p.in2 + pixoff * p.C2 + (c - p.C1);
                    preA[q][0] = *reinterpret_cast<const float4*>(src);
                    if (c + 4 < Cin) preA[q][1] = *reinterpret_cast<const float4*>(src + 4);     // Cin % 8 == 4: a 4-channel tail
                }
            }
        }
        // wave-uniform base of this K chunk (the transposed convolution reads tap slot 3 - phase of a 4-tap image)
        const int h8 = tid & (CKH - 1), c16 = (c0 >> 4) + (h8 >> 1);       // this thread's 16-channel image of the chunk
        const __bf16* wchunk = (KS == 1 && p.convt) ? p.wb + ((long)c16 * 4 + (3 - phase)) * 16 * Cout
                                                    : p.wb + (long)c16 * (TAPS * 16) * Cout;
        const bool wok = c16 * 16 < p.CinP;
#pragma unroll
        for (int q = 0; q < BP; ++q) {
            const int item = tid + q * 256;
            const int row = item / CKH, j = row % TN, tap = row / TN;
            preB[q] = make_uint4(0u, 0u, 0u, 0u);
            if (item < TAPS * TN * CKH && co0 + j < Cout && wok)
                preB[q] = *reinterpret_cast<const uint4*>(wchunk + (unsigned)((tap * Cout + co0 + j) * 16 + (h8 & 1) * 8));
        }
    };
    // Diagnostic builds only (-DNIMG_GEN_ABLATE=<bits>, results are wrong): 1 no prefetch after the first chunk, 2 no commit (LDS
    // writes) after the first chunk, 4 no barriers in the loop, 16 no epilogue stores.
#ifndef NIMG_GEN_ABLATE
#define NIMG_GEN_ABLATE 0
#endif
    constexpr int GABL = NIMG_GEN_ABLATE;
    fetch(0);
    for (int ci0 = 0; ci0 < Cin; ci0 += CK) {
        if (!(GABL & 4) || ci0 == 0) __syncthreads();
        if (!(GABL & 2) || ci0 == 0)
#pragma unroll
        for (int q = 0; q < AP; ++q) {
            const int item = tid + q * 256;
            if (item < NPIXH * CKH) {
                const int pix = item / CKH, h8 = item % CKH;
                uint4 packed;
                if constexpr (INB) {
                    packed = *reinterpret_cast<const uint4*>(&preA[q][0]);
                    if constexpr (UNP) packed = unp_route(packed, preK[q][0], preK[q][1], upos[q]);
                } else {
                    const float f[8] = {preA[q][0].x, preA[q][0].y, preA[q][0].z, preA[q][0].w,
                                        preA[q][1].x, preA[q][1].y, preA[q][1].z, preA[q][1].w};
                    const bf16x8 b = pack8(f);
                    packed = *reinterpret_cast<const uint4*>(&b);
                }
                if constexpr (PLANAR) sA[h8 * PLSZ + (pix / TWH) * 32 + pix % TWH] = packed;
                else if constexpr (CKH == 2) sA[pix * 2 + (h8 ^ ((pix >> 3) & 1))] = packed;
                else if constexpr (CKH == 4) sA[pix * 4 + (h8 ^ ((pix >> 2) & 3))] = packed;
                else sA[pix * 8 + (h8 ^ ((pix >> 1) & 7))] = packed;     // 128-byte rows: a b128 lane group = 8 even + 8 odd
                                                                         // pixels, (pix >> 1) & 7 distinct inside each set
            }
        }
        if (!(GABL & 2) || ci0 == 0)
#pragma unroll
        for (int q = 0; q < BP; ++q) {
            const int item = tid + q * 256;
            if (item < TAPS * TN * CKH) {
                const int h8 = item % CKH, row = item / CKH;
                if constexpr (CKH == 2) sB[row * 2 + (h8 ^ ((row >> 3) & 1))] = preB[q];
                else if constexpr (CKH == 4) sB[row * 4 + (h8 ^ ((row >> 2) & 3))] = preB[q];
                else sB[row * 8 + (h8 ^ ((row >> 1) & 7))] = preB[q];
            }
        }
        if (!(GABL & 4) || ci0 == 0) __syncthreads();
        if (ci0 + CK < Cin && !(GABL & 1)) fetch(ci0 + CK);
        // one kernel row unrolled: the next taps' ds_reads overlap the MFMAs.  The 32-channel tiles of the small kernels (the
        // UNet's deep and narrow layers: one or two workgroups per CU, nobody else to cover an LDS round trip) unroll ALL
        // taps - one exposed read latency per chunk instead of one per kernel row: ec42 / ec52 / dc11 -9 ... -13 %; the 64-channel
        // tiles lose 2 - 3 % with it (profiles/r03_m_conv3_unroll_ab.txt)
#pragma unroll(KS <= 3 && TN == 32 ? KS : 1)
        for (int ky = 0; ky < KS; ++ky)
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            const int tap = ky * KS + kx;
            const int toff = PLANAR ? ky * 32 + kx : ky * TWH + kx;
#pragma unroll
            for (int ks2 = 0; ks2 < CKH / 2; ++ks2) {        // MFMA k-steps of this chunk (16 channels each)
                bf16x8 a[MI], b[NI];
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    const int pix = abase[mi] + toff;
                    const uint4 v = PLANAR ? sA[pix] : (CKH == 2 ? sA[pix * 2 + (half ^ ((pix >> 3) & 1))]
                                             : (CKH == 4 ? sA[pix * 4 + ((2 * ks2 + half) ^ ((pix >> 2) & 3))]
                                                         : sA[pix * 8 + ((2 * ks2 + half) ^ ((pix >> 1) & 7))]));
                    a[mi] = *reinterpret_cast<const bf16x8*>(&v);
                }
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) {
                    const int row = tap * TN + (wn * NI + ni) * 32 + (lane & 31);
                    const uint4 v = CKH == 2 ? sB[row * 2 + (half ^ ((row >> 3) & 1))]
                                             : (CKH == 4 ? sB[row * 4 + ((2 * ks2 + half) ^ ((row >> 2) & 3))]
                                                         : sB[row * 8 + ((2 * ks2 + half) ^ ((row >> 1) & 7))]);
                    b[ni] = *reinterpret_cast<const bf16x8*>(&v);
                }
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
            }
        }
    }
    if constexpr ((GABL & 16) != 0) {          // keep the accumulators alive without storing them
        float sacc = 0.f;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int j = 0; j < 16; ++j) sacc += acc[mi][ni][j];
        if (sacc == 123.456f) p.out1[0] = sacc;
        return;
    }
    // ---- epilogue, fused activation + 2x2 max-pool (16x16 tiles; the entry point guarantees even Hout/Wout, Cout % 4 == 0)
    if constexpr (TW == 16 && NB == 1 && STRIDE == 1) {
        if (p.pool_out && !(p.flags & NIMG_POOL_ALSO)) {
            float* elds = reinterpret_cast<float*>(smem_raw) + wave * (32 * (NI * 32 + EPI_PAD));
            const int Hp = p.Hout >> 1, Wp = p.Wout >> 1;
            const float al = p.act == 1 ? p.alpha : 1.0f;
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const int py = (ty0 >> 1) + wm * MI + mi;
                pool_via_lds<NI>(acc[mi], elds, lane, al,
                    [&](int c) {
                        const int co = co0 + wn * NI * 32 + c;
                        return (p.bias && co < Cout) ? *reinterpret_cast<const float4*>(p.bias + co)
                                                     : make_float4(0.f, 0.f, 0.f, 0.f);
                    },
                    [&](int pc, int c, float4 v, uchar4 k) {
                        const int co = co0 + wn * NI * 32 + c, px = (tx0 >> 1) + pc;
                        if (co >= Cout || grp >= p.N || py >= Hp || px >= Wp) return;
                        const long o = (((long)grp * Hp + py) * Wp + px) * Cout + co;
                        if (p.flags & NIMG_BF16_OUT) store4_bf16(p.pool_out, o, v);
                        else *reinterpret_cast<float4*>(p.pool_out + o) = v;
                        if (p.pool_idx) *reinterpret_cast<uchar4*>(p.pool_idx + o) = k;
                    });
            }
            return;
        }
    }
    // ---- epilogue, vector form: accumulators turned around through LDS so each lane stores 16 B along the channels
    if ((p.O1 & 3) == 0 && (p.O2 & 3) == 0) {
        conv_epilogue_vec<KS, TH, TW, NB, MI, NI>(acc, p, smem_raw, wave, lane, wm, wn, co0, Cout, ty0, tx0, grp, phase, epi_pre);
        return;
    }
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
        const int co = co0 + (wn * NI + ni) * 32 + (lane & 31);
        if (co >= Cout) continue;
        const float bv = p.bias ? p.bias[co] : 0.f;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int row = (j & 3) + 8 * (j >> 2) + 4 * half;
                const int P = (wm * MI + mi) * 32 + row;
                const int img = P / (TH * TW), rem = P % (TH * TW);
                const int oy = ty0 + rem / TW, ox = tx0 + rem % TW, n = grp * NB + img;
                if (n >= p.N || oy >= p.Hout || ox >= p.Wout) continue;
                const long pixoff = (KS == 1 && p.convt)
                    ? ((long)n * 2 * p.Hout + 2 * oy + (phase >> 1)) * (2 * p.Wout) + 2 * ox + (phase & 1)
                    : ((long)n * p.Hout + oy) * p.Wout + ox;
                float v = acc[mi][ni][j] + bv;
                if (p.act == 1) v = lrelu(v, p.alpha);
                if (co < p.O1) {
                    if (p.act1) v *= (p.act1[pixoff * p.O1 + co] > 0.f ? 1.0f : p.alpha);
                    p.out1[pixoff * p.O1 + co] = v;
                } else {
                    p.out2[pixoff * p.O2 + (co - p.O1)] = v;
                }
            }
    }
}

// The ring kernel (its TN: 128 or 64; 0 = none) that launch_conv_b<5, 1, 16, 16, 1, 64, true> hands a layer to.  One function, so
// that who has to know the route BEFORE the launch (the fused conv + pool entry, which lets only the ring epilogue write a sign
// plane) asks exactly what the dispatch asks.
inline int conv5_ring_tn(const ConvParamsB& p) {
    static const bool no_buf = getenv("NIMG_NO_BUFFER_LOADS") != nullptr;
    static const bool no_ring = getenv("NIMG_NO_CONV5_RING") != nullptr;
    static const bool no_ring64 = getenv("NIMG_NO_CONV5_RING64") != nullptr;
    static const bool tn64 = getenv("NIMG_RING_TN64") != nullptr;      // A/B: 512 pixels x 64 channels per workgroup
    const int Cin = p.C1 + p.C2, Cout = p.O1 + p.O2;
    const long in_bytes = ((long)p.N * p.H * p.W * p.C1 * 2) >> (p.in_idx ? 2 : 0);
    const long w_bytes = (long)(p.CinP >> 4) * 25 * 16 * Cout * 2;
    if (no_buf || p.C2 != 0 || Cin % 16 != 0 || Cout % 64 != 0 || p.convt || in_bytes >= (1l << 31) - 65536 ||
        w_bytes >= (1l << 31) - 65536)
        return 0;
    // the ring kernels' epilogue knows bias / activation / mask / pooling only: a second bf16 copy (out1b), a
    // residual or a layout flag stays with the generic kernel, whose epilogue writes them
    const bool plain_epi = !p.res && !p.out1b && !(p.flags & (NIMG_D2S_OUT | NIMG_S2D_OUT | NIMG_COPY_LRELU));
    if (no_ring || !plain_epi || p.O2 != 0 || p.pad_t != 2 || p.pad_l != 2 || p.Hout != p.H || p.Wout != p.W) return 0;
    if (Cout % 128 == 0 && !(tn64 && p.Hout >= 32)) return 128;
    if (!no_ring64 && p.Hout >= 32) return 64;
    return 0;
}

template <int KS, int STRIDE, int TH, int TW, int NB, int TN, bool INB = false, bool BUF = false, int CKT = 16>
int launch_conv_b(const ConvParamsB& p, hipStream_t stream) {
    if constexpr (KS == 1 && !BUF && CKT == 16) {          // 1x1: 64-channel K chunks when the channels allow
        static const bool no_ck64 = getenv("NIMG_NO_CK64") != nullptr;
        if (!no_ck64 && (p.C1 + p.C2) % 64 == 0 && (p.C2 == 0 || p.C1 % 64 == 0))
            return launch_conv_b<KS, STRIDE, TH, TW, NB, TN, INB, false, 64>(p, stream);
    }
    if constexpr (INB && !BUF && KS == 3 && STRIDE == 1 && CKT == 16 && (TN == 32 || TN == 64)) {
        // both tiles by LDS-DMA (conv3_dma_kernel): bf16-stored input(s) whose channel counts are whole 16-channel chunks, the
        // vector epilogue's output shapes; descriptors cover < 2 GB tensors
        static const bool no_dma = getenv("NIMG_NO_CONV3_DMA") != nullptr || getenv("NIMG_NO_BUFFER_LOADS") != nullptr;
        const long px = (long)p.N * p.H * p.W;
        const long w_bytes = (long)(p.CinP >> 4) * KS * KS * 16 * (p.O1 + p.O2) * 2;
        // where it pays (profiles/r04_k_conv3_dma_ab.txt): the two-tensor inputs of the UNet's decoder (the register prefetch has
        // no buffer-descriptor form for them) and the layers with a long K loop over small images (levels 3 - 5: -6 ... -13 %);
        // the large-image layers with 2 - 4 chunks lose 10 - 20 % to the doubled LDS footprint (two instead of four
        // workgroups per CU cover each other's prologue / epilogue)
        static const long max_hw = getenv("NIMG_CONV3_DMA_MAXHW") ? atol(getenv("NIMG_CONV3_DMA_MAXHW")) : 1024;
        const bool pays = p.C2 > 0 || (long)p.Hout * p.Wout <= max_hw;
        if (!no_dma && pays && !p.convt && !p.in_idx && (!p.pool_out || (p.flags & NIMG_POOL_ALSO)) && p.C1 % 16 == 0 && p.C2 % 16 == 0 && (p.O1 & 3) == 0 &&
            (p.O2 & 3) == 0 && px * p.C1 * 2 < (1l << 31) - 65536 && px * p.C2 * 2 < (1l << 31) - 65536 &&
            w_bytes < (1l << 31) - 65536)
            return launch_conv3_dma<TH, TW, NB, TN>(p, stream);
    }
    if constexpr (INB && !BUF && (KS == 5 || KS == 3) && STRIDE == 1 && 128 % TN == 0) {
        static const bool no_buf = getenv("NIMG_NO_BUFFER_LOADS") != nullptr;
        const int Cin = p.C1 + p.C2, Cout = p.O1 + p.O2;
        const long in_bytes = ((long)p.N * p.H * p.W * p.C1 * 2) >> (p.in_idx ? 2 : 0);
        const long w_bytes = (long)(p.CinP >> 4) * KS * KS * 16 * Cout * 2;
        if (!no_buf && p.C2 == 0 && Cin % 16 == 0 && Cout % TN == 0 && !p.convt && in_bytes < (1l << 31) - 65536 &&
            w_bytes < (1l << 31) - 65536) {
            if constexpr (KS == 3 && TH == 16 && TW == 16 && NB == 1 && TN == 64) {
                // ring form at kernel size 3 (conv5_ring_kernel<128, false, 4, 3>: 16 x 16 pixels x 128 channels, 2 x 4 fragments
                // per wave, weights by LDS-DMA one kernel row at a time): the big 3x3 layers - the codec's 128 -> 128 residual
                // blocks at 64 x 64 - where the generic kernel's 2 x 2 fragment block reads as many operands as it multiplies.
                // OPT-IN (NIMG_CONV3_RING_MIN=<workgroups>, default off): stand-alone the 128 -> 128 layer gains 4 - 7 % at B = 48 ... 80
                // (profiles/r04_p_conv3_ring_codec.txt), but the config-3 step LOSES 5 % (5.02 -> 5.27 ms): two 67 KB workgroups per
                // CU leave the side streams' weight-gradient kernels no LDS to run beside them.
                static const long ring3_min = getenv("NIMG_CONV3_RING_MIN") ? atol(getenv("NIMG_CONV3_RING_MIN")) : -1;
                const long rblocks = (long)(Cout / 128) * cdiv(p.Hout, 16) * cdiv(p.Wout, 16) * p.N;
                if (ring3_min >= 0 && Cout % 128 == 0 && p.O2 == 0 && (p.O1 & 7) == 0 && p.pad_t == 1 && p.pad_l == 1 && p.Hout == p.H &&
                    p.Wout == p.W && !p.pool_out && !p.in_idx && rblocks >= ring3_min)
                    return launch_conv5_ring<128, 4, 3>(p, stream);
            }
            if constexpr (KS == 5 && TH == 16 && TW == 16 && NB == 1 && TN == 64) {
                const int ring = conv5_ring_tn(p);
                if (ring == 128) return launch_conv5_ring<128>(p, stream);
                if (ring == 64) return launch_conv5_ring<64>(p, stream);
            }
            return launch_conv_b<KS, STRIDE, TH, TW, NB, TN, true, true>(p, stream);
        }
    }
    constexpr int THH = (TH - 1) * STRIDE + KS, TWH = (TW - 1) * STRIDE + KS;
    constexpr bool PLANAR = (STRIDE == 1 && TW == 16 && NB == 1 && KS == 5);   // 3x3: the extra registers cost a wave per SIMD
#ifdef NIMG_CK32
    constexpr int CKH = CKT != 16 ? CKT / 8 : ((KS == 3 && !INB && !BUF) ? 4 : 2);     // the kernel's K chunk in 8-channel slots
#else
    constexpr int CKH = CKT / 8;
#endif
    constexpr size_t a_entries = PLANAR ? (size_t)2 * THH * 32 : (size_t)NB * THH * TWH * CKH;
    constexpr size_t lds_tiles = (a_entries + (size_t)KS * KS * TN * CKH) * sizeof(uint4);
    constexpr size_t lds_epi = (size_t)4 * 32 * (TN + EPI_PAD) * sizeof(float);
    constexpr size_t lds = lds_tiles > lds_epi ? lds_tiles : lds_epi;
    ConvParamsB q = p;
    q.tiles_y = cdiv(p.Hout, TH);
    q.tiles_x = cdiv(p.Wout, TW);
    const long blocks = (long)cdiv(p.O1 + p.O2, TN) * q.tiles_y * q.tiles_x * cdiv(p.N, NB) * (p.convt ? 4 : 1);
    auto kern = conv_fwd_bf16_kernel<KS, STRIDE, TH, TW, NB, TN, INB, BUF, false, CKT>;
    if (p.in_idx) {                     // the input is a pooled tensor + arg-max bytes: only the buffer-load variants un-pool
        if constexpr (INB && BUF && STRIDE == 1 && CKT == 16) kern = conv_fwd_bf16_kernel<KS, STRIDE, TH, TW, NB, TN, true, true, true>;
        else return NIMG_ERR_ARG;
    }
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, stream, q);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

template <int KS, int STRIDE, bool INB>
int dispatch_b_t(const ConvParamsB& p, hipStream_t s) {
    const int Cout = p.O1 + p.O2;
    const bool small = (p.Hout <= 8 && p.Wout <= 8);
    const long blocks64 = (long)cdiv(Cout, 64) * cdiv(p.Hout, small ? 8 : 16) * cdiv(p.Wout, small ? 8 : 16) *
                          cdiv(p.N, small ? 4 : 1);
    // few workgroups = few co-resident ones per CU to cover each other's staging latency: below the threshold the 32-channel
    // tile (twice the workgroups) wins (NIMG_TN32_BELOW overrides it for A/B runs)
    static const long tn32_below = getenv("NIMG_TN32_BELOW") ? atol(getenv("NIMG_TN32_BELOW")) : 384;
    const bool tn32 = (Cout <= 32) || (blocks64 < 512 && Cout % 64 != 0) || (blocks64 < tn32_below);
    if (small)
        return tn32 ? launch_conv_b<KS, STRIDE, 8, 8, 4, 32, INB>(p, s) : launch_conv_b<KS, STRIDE, 8, 8, 4, 64, INB>(p, s);
    // narrow outputs (Cout <= 32) of big images: a 32x16-pixel tile keeps 64 accumulator registers per wave (4 x 1
    // fragments) and stages a third fewer bytes per pixel than 16x16
    if constexpr (STRIDE == 1 && KS == 5) {
        if constexpr (INB) {                // ring form for exactly 32 output channels (FAN conv2 input gradient)
            static const bool no_ring32 = getenv("NIMG_NO_CONV5_RING32") != nullptr || getenv("NIMG_NO_CONV5_RING") != nullptr ||
                                          getenv("NIMG_NO_BUFFER_LOADS") != nullptr;
            const long in_bytes = ((long)p.N * p.H * p.W * p.C1 * 2) >> (p.in_idx ? 2 : 0);
            if (!no_ring32 && !p.res && !p.out1b && !(p.flags & NIMG_COPY_LRELU) && Cout == 32 && p.O2 == 0 && p.C2 == 0 && p.C1 % 16 == 0 && !p.convt && p.pad_t == 2 && p.pad_l == 2 &&
                p.Hout == p.H && p.Wout == p.W && p.Hout >= 32 && in_bytes < (1l << 31) - 65536)
                return launch_conv5_ring<32>(p, s);
        }
        if (Cout <= 32 && !p.pool_out && p.Hout % 32 == 0 && (long)cdiv(p.Hout, 32) * cdiv(p.Wout, 16) * p.N >= 2048)
            return launch_conv_b<KS, STRIDE, 32, 16, 1, 32, INB>(p, s);
    }
    return tn32 ? launch_conv_b<KS, STRIDE, 16, 16, 1, 32, INB>(p, s) : launch_conv_b<KS, STRIDE, 16, 16, 1, 64, INB>(p, s);
}

}  // namespace

// the cross-file entries declared in conv_bf16.h; conv_bf16_k*.hip instantiate them explicitly, each for its kernel sizes
template <int KS, int STRIDE, bool INB>
int conv_bf16_dispatch(const ConvArgsB& a, hipStream_t s) {
    return dispatch_b_t<KS, STRIDE, INB>(ConvParamsB{a}, s);
}
template <int KS, bool INB>
int conv_bf16_launch_16x16(const ConvArgsB& a, bool tn32, hipStream_t s) {
    const ConvParamsB p{a};
    return tn32 ? launch_conv_b<KS, 1, 16, 16, 1, 32, INB>(p, s) : launch_conv_b<KS, 1, 16, 16, 1, 64, INB>(p, s);
}
