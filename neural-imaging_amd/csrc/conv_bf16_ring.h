// Ring form of the 5x5 (and, opt-in, 3x3) stride-1 convolution over bf16-stored activations: conv5_ring_kernel, its LDS-DMA
// helpers (shared with conv_bf16_dma.h) and launch_conv5_ring.  Included through conv_bf16_tile.h.
#pragma once
#include "conv_bf16.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// Ring form of the 5x5 stride-1 convolution over bf16-stored activations with Cout % 64 == 0 (FAN conv2 / conv3 / conv4
// forward, conv4 / conv3 input gradient): 4 waves x 8 accumulator fragments per workgroup -
//     TN = 128: 16 x 16 pixels x 128 output channels, 2 x 4 fragments per wave;  TN = 64: 32 x 16 pixels x 64, 4 x 2;
//     TN = 32 (conv2's input gradient, 64 -> 32): 32 x 16 pixels x 32, 4 x 1 fragments - 64 accumulator registers, three
//     workgroups per CU (47 KB of LDS).
// conv_fwd_bf16_kernel stages the whole 25-tap weight tile of a 16-channel chunk through registers (52 VGPRs, 13
// ds_write_b128 per thread and chunk, 51 KB of LDS for 64 output channels) behind two barriers per chunk.  Here the weights
// arrive one KERNEL ROW at a time (5 taps x TN co x 16 ci = 20 / 10 KB) by LDS-DMA (buffer_load_dwordx4 ... lds: no staging
// registers, no write pass) into a two-slot ring - row r + 1 lands while the MFMAs of row r run, one barrier per row - and
// the halo tile of the next chunk (12.5 / 22.5 KB, through registers: padding, un-pool routing) is committed to the second
// of two A buffers (TN = 128) or between two barriers at the chunk boundary (TN = 64: one buffer, LDS budget).  The freed
// registers hold the 8-fragment block: 6 ds_read_b128 per 8 MFMAs instead of 4 per 4, the halo tile is staged once per
// 128 channels (or per 512 pixels) instead of once per 64 x 256, and half as many workgroups pay the prologue / epilogue.
// LDS-DMA writes base + 16 lane: the ring image is lane-linear per 1 KB piece and the XOR swizzle of the 16-byte halves
// (conflict-free ds_read_b128) is applied on the SOURCE address.  LDS: 80 KB (TN = 128) / 56 KB -> two workgroups per CU.
//
// One LDS-DMA piece: 64 lanes x 16 B from buffer `rsrc` (per-lane byte offset voff + scalar soff) to LDS bytes
// [lds_addr, lds_addr + 1024), lane-linear.  Issued as inline asm on purpose: hipcc orders the builtin form
// (__builtin_amdgcn_raw_ptr_buffer_load_lds) against every later ds_read - it emits s_waitcnt vmcnt(0) right behind the
// issue, which serialises the transfer with the MFMA loop it is meant to run under.  The asm form is invisible to the
// compiler's counters (its own waits only become conservative: loads retire in order); the kernel waits for the DMA itself
// (dma_wait) in front of the barrier that publishes the slot.
typedef unsigned int r_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void glds16(r_u32x4 rsrc, unsigned lds_addr, unsigned voff, int soff) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_addr), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
template <int N>
__device__ __forceinline__ void dma_wait_leave() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }   // loads retire in order

// Diagnostic builds only (tools/build_variant.sh + tools/ring_time.py; results are WRONG with any bit set): what the main loop of
// the ring kernels spends where.  1: no weight DMA after the first kernel row; 2: no input fetch / commit after the first chunk;
// 4: no barrier / DMA wait in the loop; 8: the operand fragments are read once, before the loop; 16: the epilogue stores nothing.
#ifndef NIMG_RING_ABLATE
#define NIMG_RING_ABLATE 0
#endif

// NW = waves per workgroup, stacked along the pixels: 4 (a 256- or 512-pixel tile, two or three workgroups per CU) or 8 (twice
// the pixels against the SAME weight ring, one workgroup per CU = still two waves per SIMD).  The weights are 8x the bytes of
// the input tile per K chunk (25 taps x 16 ci x TN co against one halo tile reused by all 25 taps), every workgroup streams
// ALL of them from L2, and the stream is what the main loop loses most to (profiles/r04_b_ring_ablation.txt: without the
// weight DMA the TN = 128 layers run 20 - 26 % faster, without the input fetch 6 %): doubling the pixels per workgroup halves
// the DMA pieces and the L2 bytes per matrix instruction.
template <int TN, int NW = 4, int KS = 5>
struct RingGeom {
    static constexpr int NI = TN / 32, MI = NI == 1 ? 4 : 8 / NI;   // fragment block of a wave (NW waves stacked along the pixels)
    static constexpr int NT = 64 * NW;
    static constexpr int TH = 2 * NW * MI, TW = 16, THH = TH + KS - 1, TWH = TW + KS - 1;
    static constexpr int NPIXH = THH * TWH, AP = (NPIXH * 2 + NT - 1) / NT;
    static constexpr int PLSZ = THH * 32;                    // uint4 entries of one k-half plane of the halo tile
    static constexpr int ABUF = 2 * PLSZ;                    // one A buffer
    static constexpr bool ADBL = TN == 128;                  // two A buffers
    static constexpr int SLOT = KS * TN * 2;                 // one ring slot: [KS taps x TN co][2 halves]
    static constexpr int PIECES = KS * NI, NPW = (PIECES + NW - 1) / NW;   // 1 KB DMA pieces per kernel row, per wave
    // ring depth.  3 (with NW = 8, where the LDS of the one resident workgroup has the room): the row requested in phase r is
    // needed in phase r + 2, so the wait at the end of a phase leaves the youngest row's transfers in flight (counted vmcnt)
    // instead of draining the queue - a weight row gets two phases to arrive from L2 instead of one.
#ifdef NIMG_RING_SLOTS2
    static constexpr int NSLOT = 2;
#else
    static constexpr int NSLOT = (NW == 8 && KS == 5) ? 3 : 2;
#endif
    static constexpr size_t LDS_TILES = (size_t)(NSLOT * SLOT + (ADBL ? 2 : 1) * ABUF) * sizeof(uint4);
    static constexpr size_t LDS_EPI = (size_t)NW * 32 * (TN + EPI_PAD) * sizeof(float);
    static constexpr size_t LDS = LDS_TILES > LDS_EPI ? LDS_TILES : LDS_EPI;
};

template <int TN, bool UNP, int NW = 4, int KS = 5>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : (TN == 32 ? 3 : 2)) void conv5_ring_kernel(const ConvParamsB p) {
    using G = RingGeom<TN, NW, KS>;
    static_assert(KS == 5 || (KS == 3 && !UNP && NW == 4), "kernel size 3: plain input, four waves");
    constexpr int NT = G::NT;
    constexpr int NI = G::NI, MI = G::MI, TH = G::TH, TW = G::TW, TWH = G::TWH, NPIXH = G::NPIXH, AP = G::AP;
    constexpr int PLSZ = G::PLSZ, ABUF = G::ABUF, SLOT = G::SLOT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint4* sB = reinterpret_cast<uint4*>(smem_raw);          // ring first: the LDS-DMA base (M0) stays below 64 KB
    uint4* sA = sB + G::NSLOT * SLOT;
    const unsigned sB_addr = (unsigned)(unsigned long)(__attribute__((address_space(3))) unsigned char*)smem_raw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Cout = p.O1;
    const int cot = Cout / TN;
    int bid = xcd_order(blockIdx.x);
    const int co0 = (bid % cot) * TN;
    bid /= cot;
    const int tiles = p.tiles_y * p.tiles_x;
    const int tile = bid % tiles, grp = bid / tiles;
    const int ty0 = (tile / p.tiles_x) * TH, tx0 = (tile % p.tiles_x) * TW;
    const int iy0 = ty0 - p.pad_t, ix0 = tx0 - p.pad_l;
    const int half = lane >> 5;

    int abase[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int P = (wave * MI + mi) * 32 + (lane & 31);
        abase[mi] = half * PLSZ + (P / TW) * 32 + (P % TW);
    }
    const int bbase = (lane & 31) * 2 + (half ^ (((lane & 31) >> 3) & 1));
    f32x16 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[mi][ni][j] = 0.0f;

    // halo tile: NPIXH pixels x 2 eight-channel slots, items of 16 B, item = tid + 256 q (the slot is fixed per thread)
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef unsigned int u32x2k __attribute__((ext_vector_type(2)));
    unsigned aoff[AP], upos[UNP ? AP : 1];
    int adst[AP];
#pragma unroll
    for (int q = 0; q < AP; ++q) {
        const int item = tid + q * NT, pix = item >> 1;
        int gy = iy0 + pix / TWH, gx = ix0 + pix % TWH;
        const bool ok = (item < NPIXH * 2) & (grp < p.N) & map_coord(gy, p.H, p.pad_mode) & map_coord(gx, p.W, p.pad_mode);
        int apix;
        if constexpr (UNP) {
            apix = (grp * (p.H >> 1) + (gy >> 1)) * (p.W >> 1) + (gx >> 1);
            upos[q] = (unsigned)(((gy & 1) << 1) | (gx & 1));
        } else {
            apix = (grp * p.H + gy) * p.W + gx;
        }
        aoff[q] = ok ? (unsigned)((apix * p.C1 + (tid & 1) * 8) * 2) : 0x80000000u;
        adst[q] = (tid & 1) * PLSZ + (pix / TWH) * 32 + pix % TWH;
    }
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.in1), 0, (int)(((long)p.N * p.H * p.W * p.C1 * 2) >> (UNP ? 2 : 0)), 0x00020000);
    const unsigned long wb_addr = (unsigned long)p.wb;
    const r_u32x4 rb = {(unsigned)wb_addr, (unsigned)(wb_addr >> 32) & 0xffffu,
                        (unsigned)((long)(p.CinP >> 4) * KS * KS * 16 * Cout * 2), 0x00020000u};
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(UNP ? p.in_idx : reinterpret_cast<const unsigned char*>(p.in1)), 0,
        (int)(((long)p.N * p.H * p.W * p.C1) >> 2), 0x00020000);
    uint4 preA[AP];
    u32x2k preK[UNP ? AP : 1];
    auto fetchA = [&](int c0) {
#pragma unroll
        for (int q = 0; q < AP; ++q) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(ra, aoff[q], c0 * 2, 0);
            preA[q] = *reinterpret_cast<const uint4*>(&v);
            if constexpr (UNP)
                preK[q] = __builtin_amdgcn_raw_buffer_load_b64(rk, aoff[q] >= 0x80000000u ? 0x80000000u : aoff[q] >> 1, c0, 0);
        }
    };
    auto commitA = [&](int buf) {                       // buf: entry offset of the A buffer
#pragma unroll
        for (int q = 0; q < AP; ++q) {
            if (tid + q * NT < NPIXH * 2) {
                uint4 v = preA[q];
                if constexpr (UNP) v = unp_route(v, preK[q][0], preK[q][1], upos[q]);
                sA[buf + adst[q]] = v;
            }
        }
    };
    // weights wb[chunk][tap][co][16]: one kernel row of a chunk = 5 taps x TN co x 32 B = 5 NI pieces of 1 KB (piece k =
    // tap k / NI, 32-channel block k % NI, at ring byte 1024 k); wave w moves the pieces w, w + 4, ...  Lane l of a piece
    // writes 16-byte position l: row l >> 1, and position parity (l & 1) must hold half h = (l & 1) ^ (row >> 3 & 1) - the
    // swizzle the fragment reads undo.
    const unsigned bvoff = (unsigned)(((co0 + (lane >> 1)) * 16 + (((lane & 1) ^ ((lane >> 4) & 1)) * 8)) * 2);
    auto gldsB = [&](int chunk, int ky, int slot) {
#pragma unroll
        for (int j = 0; j < G::NPW; ++j) {
            const int k = wave + NW * j;
            if (G::PIECES % NW == 0 || k < G::PIECES) {
                const int soff = ((chunk * KS * KS + ky * KS + k / NI) * Cout + (k % NI) * 32) * 32;
                glds16(rb, sB_addr + (unsigned)((slot * SLOT + k * 64) * 16), bvoff, soff);
            }
        }
    };
    const int chunks = p.C1 >> 4;
    gldsB(0, 0, 0);
    if constexpr (G::NSLOT == 3) gldsB(0, 1, 1);
    fetchA(0);
    commitA(0);
    dma_wait();
    __syncthreads();
    constexpr int ABL = NIMG_RING_ABLATE;
    bf16x8 a0[MI], b0[NI];
    if constexpr (ABL & 8) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) { const uint4 v = sA[abase[mi]]; a0[mi] = *reinterpret_cast<const bf16x8*>(&v); }
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) { const uint4 v = sB[bbase + ni * 64]; b0[ni] = *reinterpret_cast<const bf16x8*>(&v); }
    }
    if constexpr (G::NSLOT == 3) {
        static_assert(G::ADBL, "the three-slot ring is written for the double-buffered input tile");
        // transfers of ONE wave per kernel row: waves below PIECES % NW move one piece more
        constexpr int NLO = G::PIECES / NW, NREM = G::PIECES % NW;
        constexpr int NA = AP * (UNP ? 2 : 1);             // the input prefetch of phase 0: loads queued BEHIND that phase's row
        int s0 = 0;                                        // slot of kernel row 0 of this chunk = (5 c) % 3
        for (int c = 0; c < chunks; ++c) {
            const int ab = (c & 1) * ABUF;
            const bool more = c + 1 < chunks;
#pragma unroll
            for (int ky = 0; ky < 5; ++ky) {
                const int slot = (s0 + ky) % 3, slot2 = (s0 + ky + 2) % 3;
                if (ky == 2 && more) commitA(ab ^ ABUF);   // (the compiler drains the queue for the prefetched registers here)
                const bool issue = ky < 3 || more;         // row r + 2 exists
                if (ky < 3) gldsB(c, ky + 2, slot2);
                else if (more) gldsB(c + 1, ky - 3, slot2);
                if (ky == 0 && more) fetchA((c + 1) * 16);
                const uint4* sBs = sB + slot * SLOT + bbase;
#pragma unroll
                for (int kx = 0; kx < 5; ++kx) {
                    bf16x8 a[MI], b[NI];
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi) {
                        const uint4 v = sA[ab + abase[mi] + ky * 32 + kx];
                        a[mi] = *reinterpret_cast<const bf16x8*>(&v);
                    }
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni) {
                        const uint4 v = sBs[(kx * TN + ni * 32) * 2];
                        b[ni] = *reinterpret_cast<const bf16x8*>(&v);
                    }
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                        for (int ni = 0; ni < NI; ++ni)
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
                }
                // row r + 1 must have landed; what may stay in flight is younger: this phase's row and, in phases 0 / 1 of a
                // chunk, the input prefetch queued behind phase 0's row
                if (!issue) dma_wait();
                else if (ky < 2 && more) {
                    if (NREM && wave < NREM) dma_wait_leave<NLO + 1 + NA>();
                    else dma_wait_leave<NLO + NA>();
                } else {
                    if (NREM && wave < NREM) dma_wait_leave<NLO + 1>();
                    else dma_wait_leave<NLO>();
                }
                // raw barrier: __syncthreads() may drain the memory queue for its fence - the youngest row has to stay in flight.
                // What has to be ordered here is LDS only: this wave's tile writes (lgkmcnt) and its landed transfers (above).
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
            s0 = (s0 + 2) % 3;
        }
    } else
    for (int c = 0; c < chunks; ++c) {
        const int ab = G::ADBL ? (c & 1) * ABUF : 0;
        const bool more = c + 1 < chunks;
#pragma unroll
        for (int ky = 0; ky < KS; ++ky) {
            const int slot = (c + ky) & 1;                 // (KS c + ky) & 1, KS odd
            if constexpr (!(ABL & 1)) {
                if (ky < KS - 1) gldsB(c, ky + 1, slot ^ 1);
                else if (more) gldsB(c + 1, 0, slot ^ 1);
            }
            if constexpr (!(ABL & 2)) if (ky == 0 && more) fetchA((c + 1) * 16);
            const uint4* sBs = sB + slot * SLOT + bbase;
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
                bf16x8 a[MI], b[NI];
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    if constexpr (ABL & 8) { a[mi] = a0[mi]; continue; }
                    const uint4 v = sA[ab + abase[mi] + ky * 32 + kx];
                    a[mi] = *reinterpret_cast<const bf16x8*>(&v);
                }
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) {
                    if constexpr (ABL & 8) { b[ni] = b0[ni]; continue; }
                    const uint4 v = sBs[(kx * TN + ni * 32) * 2];
                    b[ni] = *reinterpret_cast<const bf16x8*>(&v);
                }
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
            }
            if constexpr (!(ABL & 2)) if (G::ADBL && ky == KS - 1 && more) commitA(ab ^ ABUF);
            if constexpr (!(ABL & 4)) {
                dma_wait();                                // the next kernel row has landed ...
                __syncthreads();                           // ... and everyone is done with this one (slot and A buffer free)
            }
            if constexpr (!(ABL & 2)) if (!G::ADBL && ky == KS - 1 && more) {
                commitA(0);
                if constexpr (!(ABL & 4)) __syncthreads();
            }
        }
    }
    if constexpr (ABL & 4) { dma_wait(); __syncthreads(); }
    if constexpr (ABL & 16) {              // keep the accumulators alive without storing them
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
    if constexpr (KS == 3) {        // the 3x3 layers (codec, UNet): every epilogue option of conv_fwd_bf16_kernel, same code
        conv_epilogue_vec<3, TH, TW, 1, MI, NI>(acc, p, smem_raw, wave, lane, wave, 0, co0, Cout, ty0, tx0, grp, 0,
                                                epi_bias_preload<NI>(p, lane, 0, co0, Cout));
        return;
    }
    // epilogue: per-wave private LDS scratch (the loop's last barrier released the tiles) -> wave-level ordering only
    float* elds = reinterpret_cast<float*>(smem_raw) + wave * (32 * (NI * 32 + EPI_PAD));
    if (p.pool_out) {                                      // fused activation + 2x2 max-pool (even Hout / Wout)
        const int Hp = p.Hout >> 1, Wp = p.Wout >> 1;
        const float al = p.act == 1 ? p.alpha : 1.0f;
        if (p.flags & NIMG_BF16_OUT) {                     // bf16-stored: 16-byte stores of 8 channels (+ 8 arg-max bytes)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const int py = (ty0 >> 1) + wave * MI + mi;
                pool_in_regs8<NI>(acc[mi], elds, lane, al,
                    [&](int c) { return p.bias ? p.bias[co0 + c] : 0.f; },
                    [&](int pc, int c, float4 lo, float4 hi, uint2 k) {
                        const int px = (tx0 >> 1) + pc;
                        if (grp >= p.N || py >= Hp || px >= Wp) return;
                        const long o = (((long)grp * Hp + py) * Wp + px) * Cout + co0 + c;
                        const float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                        const bf16x8 pk = pack8(f);
                        *reinterpret_cast<bf16x8*>(reinterpret_cast<__bf16*>(p.pool_out) + o) = pk;
                        if (p.pool_idx) *reinterpret_cast<uint2*>(p.pool_idx + o) = k;
                        if (p.pool_sign) {                 // one bit per value AS STORED: what the next layer's input gradient
                            const uint4 pw = __builtin_bit_cast(uint4, pk);      // would have derived from the bf16 tensor
                            const unsigned sb = bf16x2_positive(pw.x) | (bf16x2_positive(pw.y) << 1) | (bf16x2_positive(pw.z) << 2) |
                                                (bf16x2_positive(pw.w) << 3);
                            p.pool_sign[o >> 3] = (unsigned char)sign_bits_interleave(sb);
                        }
                    });
            }
            return;
        }
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int py = (ty0 >> 1) + wave * MI + mi;
            pool_in_regs<NI>(acc[mi], elds, lane, al,
                [&](int c) { return p.bias ? p.bias[co0 + c] : 0.f; },
                [&](int pc, int c, float4 v, uchar4 k) {
                    const int co = co0 + c, px = (tx0 >> 1) + pc;
                    if (grp >= p.N || py >= Hp || px >= Wp) return;
                    const long o = (((long)grp * Hp + py) * Wp + px) * Cout + co;
                    if (p.flags & NIMG_BF16_OUT) store4_bf16(p.pool_out, o, v);
                    else *reinterpret_cast<float4*>(p.pool_out + o) = v;
                    if (p.pool_idx) *reinterpret_cast<uchar4*>(p.pool_idx + o) = k;
                });
        }
        return;
    }
    if ((p.flags & NIMG_BF16_OUT) && (!p.act1 || (p.flags & NIMG_BF16_MASK))) {     // bf16-stored output (and mask): 16-byte rows
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            epilogue_via_lds8<NI>(acc[mi], elds, lane, [&](int row, int c, float4 lo, float4 hi) {
                const int P = (wave * MI + mi) * 32 + row;
                const int oy = ty0 + P / TW, ox = tx0 + P % TW;
                if (grp >= p.N || oy >= p.Hout || ox >= p.Wout) return;
                const long o = (((long)grp * p.Hout + oy) * p.Wout + ox) * Cout + co0 + c;
                float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                if (p.bias) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] += p.bias[co0 + c + e];
                }
                if (p.act == 1) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] = lrelu(f[e], p.alpha);
                }
                if (p.act_sign) {                  // the mask's sign plane: one byte instead of the activation's 16
                    const unsigned sb = p.act_sign[o >> 3];
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] *= ((sb >> e) & 1u) ? 1.0f : p.alpha;
                } else if (p.act1) {
                    const bf16x8 m = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const __bf16*>(p.act1) + o);
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] *= (float)m[e] > 0.f ? 1.0f : p.alpha;
                }
                *reinterpret_cast<bf16x8*>(reinterpret_cast<__bf16*>(p.out1) + o) = pack8(f);
            });
        }
        return;
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        epilogue_via_lds<NI, false>(acc[mi], elds, lane, [&](int row, int c, float4 v) {
            const int co = co0 + c;
            const int P = (wave * MI + mi) * 32 + row;
            const int oy = ty0 + P / TW, ox = tx0 + P % TW;
            if (grp >= p.N || oy >= p.Hout || ox >= p.Wout) return;
            const long o = (((long)grp * p.Hout + oy) * p.Wout + ox) * Cout + co;
            if (p.bias) {
                const float4 b = *reinterpret_cast<const float4*>(p.bias + co);
                v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
            }
            if (p.act == 1) {
                v.x = lrelu(v.x, p.alpha); v.y = lrelu(v.y, p.alpha); v.z = lrelu(v.z, p.alpha); v.w = lrelu(v.w, p.alpha);
            }
            if (p.act1) {
                const float4 m = (p.flags & NIMG_BF16_MASK) ? load4_bf16(p.act1, o) : *reinterpret_cast<const float4*>(p.act1 + o);
                v.x *= m.x > 0.f ? 1.0f : p.alpha; v.y *= m.y > 0.f ? 1.0f : p.alpha;
                v.z *= m.z > 0.f ? 1.0f : p.alpha; v.w *= m.w > 0.f ? 1.0f : p.alpha;
            }
            if (p.flags & NIMG_BF16_OUT) store4_bf16(p.out1, o, v);
            else *reinterpret_cast<float4*>(p.out1 + o) = v;
        });
    }
}

template <int TN, int NW = 4, int KS = 5>
int launch_conv5_ring(const ConvParamsB& p, hipStream_t stream) {
    using G = RingGeom<TN, NW, KS>;
    if constexpr (NW == 4 && TN == 128 && KS == 5) {
        // NIMG_RING_NW8=1 (A/B switch, not the product path): eight waves on a 32 x 16 tile against one three-slot weight ring.
        // Measured (profiles/r04_ring_*.txt): half the weight DMA per matrix instruction raises the clock the chip sustains
        // (1.81 -> 1.94 GHz on conv3) but the single resident workgroup loses more to its lock-step phases (MFMA pipe busy
        // 0.665 -> 0.568): 436 -> 459 us.  The four-wave form with two independent workgroups per CU stays.
        static const bool nw8 = getenv("NIMG_RING_NW8") != nullptr;
        if (nw8 && p.Hout % 32 == 0) return launch_conv5_ring<TN, 8>(p, stream);
    }
    ConvParamsB q = p;
    q.tiles_y = cdiv(p.Hout, G::TH);
    q.tiles_x = cdiv(p.Wout, G::TW);
    const long blocks = (long)(p.O1 / TN) * q.tiles_y * q.tiles_x * p.N;
    auto kern = conv5_ring_kernel<TN, false, NW, KS>;
    if constexpr (KS == 5) { if (p.in_idx) kern = conv5_ring_kernel<TN, true, NW, KS>; }
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(G::NT), G::LDS, stream, q);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

}  // namespace
