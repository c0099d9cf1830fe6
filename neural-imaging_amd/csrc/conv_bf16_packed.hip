// FAN front end in throughput mode (the 3-channel side of the first convolution, models/forensics.py:69): the three
// passes that touch the 256x256x32 tensor are HBM-bound (2.7 GB per 320-image batch each), so they must not waste the
// matrix core on channel padding nor the LDS on re-reads.  Here: the few-channel ("packed") forward, weight-gradient and
// input-gradient kernels with their entry points; the weight gradient is reached through conv_bf16_wgrad.hip's dispatch.
#include "conv_bf16_wgrad.h"

namespace {

// ---- forward, Cin <= 4: K = (tap, ci) packed (75 -> 80), A gathered from f32 channel planes, B = [co][k] bf16 ---------
template <int KS, int CINP, int TN>
__global__ __launch_bounds__(256) void conv_fwd_packed_bf16_kernel(const float* __restrict__ in,
                                                                   const float* __restrict__ w,
                                                                   const float* __restrict__ bias,
                                                                   float* __restrict__ out,
                                                                   float* __restrict__ pool_out,
                                                                   unsigned char* __restrict__ pool_idx, int N, int H,
                                                                   int W, int Cout, int pad_mode, int act, float alpha,
                                                                   int tiles_y, int tiles_x, int tiles_per_wg,
                                                                   int out_bf16) {
    constexpr int TH = 16, TW = 16, THH = TH + KS - 1, TWH = TW + KS - 1, P = (KS - 1) / 2;
    constexpr int NPIXH = THH * TWH, PS = ((NPIXH + 31) / 32) * 32 + 2;
    constexpr int KTOT = KS * KS * CINP, KSTEPS = (KTOT + 15) / 16, KP = KSTEPS * 16;
    constexpr int NI = TN / 32, MI = 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* sA = reinterpret_cast<float*>(smem_raw);                           // [CINP][PS] f32
    constexpr int A_BYTES = (CINP * PS * 4 + 15) / 16 * 16;
    __bf16* sB = reinterpret_cast<__bf16*>(smem_raw + A_BYTES);               // [TN][KP] bf16, 16-byte aligned
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cot = (Cout + TN - 1) / TN;
    const int xbid = xcd_order(blockIdx.x);
    const int co0 = (xbid % cot) * TN, wg = xbid / cot;
    const int tiles = tiles_y * tiles_x;
    const long total_tiles = (long)tiles * N;
    for (int item = tid; item < TN * KP; item += 256) {
        const int k = item % KP, j = item / KP;
        sB[item] = (__bf16)((k < KTOT && co0 + j < Cout) ? w[(long)k * Cout + co0 + j] : 0.f);
    }
    int koff[KSTEPS][8];
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int k = s * 16 + half * 8 + j;
            k = k < KTOT ? k : 0;                                  // padded slots meet zero weights
            const int tap = k / CINP, ci = k - tap * CINP;
            koff[s][j] = ci * PS + (tap / KS) * TWH + (tap % KS);
        }
    int abase[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int Pp = (wave * MI + mi) * 32 + (lane & 31);
        abase[mi] = (Pp / TW) * TWH + (Pp % TW);
    }
    // the halo of tile t+1 is fetched into registers while tile t is computed and stored (the tiles are tiny, so the
    // loop is otherwise a chain of exposed HBM latencies)
    constexpr int PPT = (NPIXH + 255) / 256;
    float pre[PPT][CINP];
    auto fetch = [&](long gt) {
        const int n_ = (int)(gt / tiles), tile_ = (int)(gt % tiles);
        const int ty_ = (tile_ / tiles_x) * TH, tx_ = (tile_ % tiles_x) * TW;
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int pix = tid + q * 256;
            int gy = ty_ - P + pix / TWH, gx = tx_ - P + pix % TWH;
            const bool ok = pix < NPIXH && map_coord(gy, H, pad_mode) && map_coord(gx, W, pad_mode);
            const float* src = in + (((long)n_ * H + gy) * W + gx) * CINP;
#pragma unroll
            for (int c = 0; c < CINP; ++c) pre[q][c] = ok ? src[c] : 0.f;
        }
    };
    const long gt0 = (long)wg * tiles_per_wg;
    if (gt0 < total_tiles) fetch(gt0);
    for (int tt = 0; tt < tiles_per_wg; ++tt) {
        const long gt = gt0 + tt;
        if (gt >= total_tiles) break;
        const int n = (int)(gt / tiles), tile = (int)(gt % tiles);
        const int ty0 = (tile / tiles_x) * TH, tx0 = (tile % tiles_x) * TW;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            const int pix = tid + q * 256;
            if (pix < NPIXH) {
#pragma unroll
                for (int c = 0; c < CINP; ++c) sA[c * PS + pix] = pre[q][c];
            }
        }
        __syncthreads();
        if (tt + 1 < tiles_per_wg && gt + 1 < total_tiles) fetch(gt + 1);
        f32x16 acc[MI][NI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[mi][ni][j] = 0.0f;
        // an opaque per-tile copy of the pixel bases: otherwise all KSTEPS*8*MI gather addresses (loop invariant) are
        // hoisted out of the tile loop and pinned in ~80 VGPRs, which drops the kernel to one wave per SIMD
        int ab[MI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            ab[mi] = abase[mi];
            asm volatile("" : "+v"(ab[mi]));
        }
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            bf16x8 b[NI];
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
                b[ni] = *reinterpret_cast<const bf16x8*>(sB + (ni * 32 + (lane & 31)) * KP + s * 16 + half * 8);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                float f[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = sA[koff[s][j] + ab[mi]];
                const bf16x8 a = pack8(f);
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[ni], acc[mi][ni], 0, 0, 0);
            }
            // keep the gathers of later k-steps from being hoisted up here: that costs ~250 VGPRs (one wave per SIMD);
            // with the fence the kernel fits 3-4 waves per SIMD, which is what hides the LDS gather latency
            __builtin_amdgcn_sched_barrier(0);
        }
        if (pool_out) {                 // fused activation + 2x2 max-pool (common.h); private per-wave scratch
            float* elds = reinterpret_cast<float*>(smem_raw + A_BYTES + TN * KP * 2) + wave * (32 * (NI * 32 + EPI_PAD));
            const int Hp = H >> 1, Wp = W >> 1;
            const float al = act == 1 ? alpha : 1.0f;
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const int py = (ty0 >> 1) + wave * MI + mi;
                pool_via_lds<NI, false>(acc[mi], elds, lane, al,
                    [&](int c) {
                        return (bias && co0 + c < Cout) ? *reinterpret_cast<const float4*>(bias + co0 + c)
                                                        : make_float4(0.f, 0.f, 0.f, 0.f);
                    },
                    [&](int pc, int c, float4 v, uchar4 k) {
                        const int co = co0 + c, px = (tx0 >> 1) + pc;
                        if (co >= Cout || py >= Hp || px >= Wp) return;
                        const long o = (((long)n * Hp + py) * Wp + px) * Cout + co;
                        if (out_bf16) store4_bf16(pool_out, o, v);
                        else *reinterpret_cast<float4*>(pool_out + o) = v;
                        if (pool_idx) *reinterpret_cast<uchar4*>(pool_idx + o) = k;
                    });
            }
            continue;
        }
        if ((Cout & 3) == 0) {          // vector epilogue: 16 B per lane along the channels (common.h)
            float* elds = reinterpret_cast<float*>(smem_raw + A_BYTES + TN * KP * 2) + wave * (32 * (NI * 32 + EPI_PAD));
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                epilogue_via_lds<NI, false>(acc[mi], elds, lane, [&](int row, int c, float4 v) {
                    const int co = co0 + c;
                    if (co >= Cout) return;
                    const int Pp = (wave * MI + mi) * 32 + row;
                    const int oy = ty0 + Pp / TW, ox = tx0 + Pp % TW;
                    if (oy >= H || ox >= W) return;
                    if (bias) {
                        const float4 b4 = *reinterpret_cast<const float4*>(bias + co);
                        v.x += b4.x; v.y += b4.y; v.z += b4.z; v.w += b4.w;
                    }
                    if (act == 1) {
                        v.x = lrelu(v.x, alpha); v.y = lrelu(v.y, alpha); v.z = lrelu(v.z, alpha); v.w = lrelu(v.w, alpha);
                    }
                    const long o = (((long)n * H + oy) * W + ox) * Cout + co;
                    if (out_bf16) store4_bf16(out, o, v);
                    else *reinterpret_cast<float4*>(out + o) = v;
                });
            }
            continue;
        }
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const int co = co0 + ni * 32 + (lane & 31);
            if (co >= Cout) continue;
            const float bv = bias ? bias[co] : 0.f;
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int Pp = (wave * MI + mi) * 32 + (j & 3) + 8 * (j >> 2) + 4 * half;
                    const int oy = ty0 + Pp / TW, ox = tx0 + Pp % TW;
                    if (oy >= H || ox >= W) continue;
                    float v = acc[mi][ni][j] + bv;
                    if (act == 1) v = lrelu(v, alpha);
                    out[(((long)n * H + oy) * W + ox) * Cout + co] = v;
                }
        }
    }
}

// ---- weight gradient, Cin <= 4: M = (tap, ci) packed, K = 16 pixels per MFMA, operands gathered from f32 tiles --------
// ZMODE 0: dz at full resolution (float32); 1: POOLED gradient (float32) + arg-max bytes, un-pooled while staging;
// 2: the same with the pooled gradient stored as bf16.  Compile-time, so the prefetch loads sit in straight-line code.
// No __launch_bounds__: while this kernel shared a file with its dispatch, a forward declaration without one stood in front of
// the launches and decided the attributes of every instantiation - the (256) written here never took effect, and the kernels are
// compiled for up to 1024 threads (128 VGPRs; the 5x5 forms spill).  Stating it changes all 24 code objects: a change of its own.
template <int KS, int CINP, int NI, int ZMODE>
__global__ void conv_wgrad_packed_bf16_kernel(const WgradParamsB p) {
    constexpr int TAPS = KS * KS, TPF = 32 / CINP, MF = (TAPS + TPF - 1) / TPF;
    constexpr int THH = B_TH + KS - 1, TWH = B_TW + KS - 1, NPIXH = THH * TWH, NPIX = B_TH * B_TW, COT = 32 * NI;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sI = smem;                    // [NPIXH][CINP]
    float* sZ = smem + NPIXH * CINP;     // [NPIX][COT]
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cob = (p.Cout + COT - 1) / COT;
    const int xbid = xcd_order(blockIdx.x);
    const int co0 = (xbid % cob) * COT, split = xbid / cob;
    int aoff[MF];
#pragma unroll
    for (int f = 0; f < MF; ++f) {
        const int i = lane & 31, tl = i / CINP, ci = i % CINP, tap = f * TPF + tl;
        aoff[f] = (tl < TPF && tap < TAPS) ? ((tap / KS) * TWH + (tap % KS)) * CINP + ci : -1;
    }
    f32x16 acc[MF][NI];
#pragma unroll
    for (int f = 0; f < MF; ++f)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[f][ni][j] = 0.0f;
    const int tiles = p.tiles_y * p.tiles_x;
    const int work_total = p.N * tiles;                 // < 2^31 (checked by the entry point)
    const int w_begin = split * p.work_per_split, w_end = min(work_total, w_begin + p.work_per_split);
    const bool do_bias = p.db_partial != nullptr;
    float bsum = 0.f;
    // register prefetch of the next tile (both operands) while the current one is multiplied
    constexpr int IPT = (NPIXH + 255) / 256, ZPT = NPIX * (COT / 4) / 256;
    float prei[IPT][CINP];
    float4 prez[ZPT];
    unsigned int prek[ZPT];
    const bool vec_z = (p.Cout % 4 == 0);
    auto fetch = [&](int wk_) {
        const int n_ = (int)(wk_ / tiles), tile_ = (int)(wk_ % tiles);
        const int ty_ = (tile_ / p.tiles_x) * B_TH, tx_ = (tile_ % p.tiles_x) * B_TW;
#pragma unroll
        for (int q = 0; q < IPT; ++q) {
            const int pix = tid + q * 256;
            int gy = ty_ - p.pad_t + pix / TWH, gx = tx_ - p.pad_l + pix % TWH;
            const bool ok = pix < NPIXH && map_coord(gy, p.H, p.pad_mode) && map_coord(gx, p.W, p.pad_mode);
            const float* src = p.in1 + (((long)n_ * p.H + gy) * p.W + gx) * CINP;
#pragma unroll
            for (int c = 0; c < CINP; ++c) prei[q][c] = ok ? src[c] : 0.f;
        }
        if (vec_z) {
#pragma unroll
            for (int q = 0; q < ZPT; ++q) {
                const int item = tid + q * 256;
                const int pix = item / (COT / 4), c = co0 + (item % (COT / 4)) * 4;
                const int oy = ty_ + pix / B_TW, ox = tx_ + pix % B_TW;
                prez[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (ZMODE >= 1) {  // pooled gradient + arg-max: this pixel receives it iff it was the window maximum
                    prek[q] = 0xffffffffu;
                    if (oy < p.Hout && ox < p.Wout && c < p.Cout) {
                        const long po = (((long)n_ * (p.Hout >> 1) + (oy >> 1)) * (p.Wout >> 1) + (ox >> 1)) * p.Cout + c;
                        if constexpr (ZMODE == 2) {
                            const uint2 raw = *reinterpret_cast<const uint2*>(reinterpret_cast<const __bf16*>(p.dz) + po);
                            prez[q].x = __uint_as_float(raw.x);          // 4 x bf16, expanded when the tile is committed
                            prez[q].y = __uint_as_float(raw.y);
                        } else {
                            prez[q] = *reinterpret_cast<const float4*>(p.dz + po);
                        }
                        prek[q] = *reinterpret_cast<const unsigned int*>(p.dz_idx + po);
                    }
                } else if (oy < p.Hout && ox < p.Wout && c < p.Cout) {
                    prez[q] = *reinterpret_cast<const float4*>(p.dz + (((long)n_ * p.Hout + oy) * p.Wout + ox) * p.Cout + c);
                }
            }
        }
    };
    if (w_begin < w_end) fetch(w_begin);
    for (int wk = w_begin; wk < w_end; ++wk) {
        const int n = (int)(wk / tiles), tile = (int)(wk % tiles);
        const int ty0 = (tile / p.tiles_x) * B_TH, tx0 = (tile % p.tiles_x) * B_TW;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < IPT; ++q) {
            const int pix = tid + q * 256;
            if (pix < NPIXH) {
#pragma unroll
                for (int c = 0; c < CINP; ++c) sI[pix * CINP + c] = prei[q][c];
            }
        }
        if (vec_z) {
#pragma unroll
            for (int q = 0; q < ZPT; ++q) {
                const int item = tid + q * 256;
                float4 v = prez[q];
                if constexpr (ZMODE == 2) {
                    const unsigned lo = __float_as_uint(prez[q].x), hi = __float_as_uint(prez[q].y);
                    v = make_float4(__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u),
                                    __uint_as_float(hi << 16), __uint_as_float(hi & 0xffff0000u));
                }
                if constexpr (ZMODE >= 1) {
                    const int pix = item / (COT / 4);
                    const unsigned pos = (unsigned)((((ty0 + pix / B_TW) & 1) << 1) | ((tx0 + pix % B_TW) & 1));
                    const unsigned k = prek[q];
                    v.x = (k & 0xffu) == pos ? v.x : 0.f;
                    v.y = ((k >> 8) & 0xffu) == pos ? v.y : 0.f;
                    v.z = ((k >> 16) & 0xffu) == pos ? v.z : 0.f;
                    v.w = (k >> 24) == pos ? v.w : 0.f;
                }
                *reinterpret_cast<float4*>(sZ + (item / (COT / 4)) * COT + (item % (COT / 4)) * 4) = v;
            }
        } else {
            for (int item = tid; item < NPIX * COT; item += 256) {
                const int pix = item / COT, c = co0 + item % COT;
                const int oy = ty0 + pix / B_TW, ox = tx0 + pix % B_TW;
                sZ[item] = (oy < p.Hout && ox < p.Wout && c < p.Cout)
                               ? p.dz[(((long)n * p.Hout + oy) * p.Wout + ox) * p.Cout + c] : 0.f;
            }
        }
        __syncthreads();
        if (wk + 1 < w_end) fetch(wk + 1);
        if (do_bias && tid < COT) {
#pragma unroll 8
            for (int px = 0; px < NPIX; ++px) bsum += sZ[px * COT + tid];
        }
        for (int r = wave; r < B_TH; r += 4) {
            float f8[8];
            bf16x8 b[NI];
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
#pragma unroll
                for (int k = 0; k < 8; ++k) f8[k] = sZ[(r * B_TW + half * 8 + k) * COT + ni * 32 + (lane & 31)];
                b[ni] = pack8(f8);
            }
#pragma unroll
            for (int f = 0; f < MF; ++f) {
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    f8[k] = aoff[f] >= 0 ? sI[(r * TWH + half * 8 + k) * CINP + aoff[f]] : 0.f;
                const bf16x8 a = pack8(f8);
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
                    acc[f][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[ni], acc[f][ni], 0, 0, 0);
            }
        }
    }
    if (do_bias && tid < COT && co0 + tid < p.Cout) p.db_partial[(long)split * p.Cout + co0 + tid] = bsum;
    // the four waves hold row partials of the same (tap, ci) x co block: fold them through LDS (waves 1..3 park theirs, wave 0
    // adds in order) - one slab per workgroup instead of four (4096 slabs of the UNet's first layer took a 42 us reduction)
    constexpr bool FOLD = MF * NI <= 2;              // 3 x MF x NI x 4 KB of scratch: the small (3x3) layers only
    if constexpr (FOLD) {
        __syncthreads();
        float* red = smem;
        if (wave > 0) {
#pragma unroll
            for (int f = 0; f < MF; ++f)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                    for (int j = 0; j < 16; ++j) red[((((wave - 1) * MF + f) * NI + ni) * 16 + j) * 64 + lane] = acc[f][ni][j];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int w = 1; w < 4; ++w)
#pragma unroll
            for (int f = 0; f < MF; ++f)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                    for (int j = 0; j < 16; ++j) acc[f][ni][j] += red[((((w - 1) * MF + f) * NI + ni) * 16 + j) * 64 + lane];
    }
    float* slab = p.partial + ((long)split * (FOLD ? 1 : 4) + (FOLD ? 0 : wave)) * TAPS * CINP * p.Cout;
#pragma unroll
    for (int f = 0; f < MF; ++f)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const int co = co0 + ni * 32 + (lane & 31);
            if (co >= p.Cout) continue;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int i = (j & 3) + 8 * (j >> 2) + 4 * half;
                const int tl = i / CINP, ci = i % CINP, tap = f * TPF + tl;
                if (tl < TPF && tap < TAPS) slab[((long)tap * CINP + ci) * p.Cout + co] = acc[f][ni][j];
            }
        }
}

// ---- input gradient towards FEW channels (CI <= 6 with KS*CI <= 32), from CZ = 32 gradient channels -----------------
//   out[u][v][ci] = sum_{ky,kx,co} dz[u+P-ky][v+P-kx][co] * w[ky][kx][ci][co]
// The kx loop is folded into the MFMA N dimension: T[u][x'][(kx,ci)] = sum_{ky,co} dz[u+P-ky][x'][co] * w[ky][kx][ci][co]
// is one 32 x 32 x (KS*CZ) GEMM per output row (32 positions x', KS*CI <= 32 columns, no padded channels), and
// out[u][v][ci] = sum_kx T[u][v+P-kx][(kx,ci)] is a shift-add through a 2 KB LDS tile.  w is the forward kernel
// (kh,kw,CI,CZ) as stored - its [ky][(kx,ci)][co] order is exactly the B operand.
// ZMODE 0: dz at full resolution (float32); 1: POOLED gradient (float32) + arg-max bytes; 2: pooled gradient as bf16.
template <int KS, int CI, int ZMODE>
__global__ __launch_bounds__(256) void conv_dgrad_fewin_bf16_kernel(const float* __restrict__ dz,
                                                                    const unsigned char* __restrict__ dz_idx,
                                                                    const float* __restrict__ w,
                                                                    float* __restrict__ out, int N, int H, int W,
                                                                    int tiles_y, int tiles_x) {
    constexpr int CZ = 32, P = (KS - 1) / 2, TH = 8, TWO = 32 - (KS - 1);      // TWO output columns per tile
    constexpr int ROWS = TH + KS - 1, NJ = KS * CI;
    static_assert(NJ <= 32, "KS * CI must fit one MFMA N tile");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint4* sD = reinterpret_cast<uint4*>(smem_raw);                           // [ROWS*32 px][4 chunks of 8 co]
    uint4* sW = sD + ROWS * 32 * 4;                                           // [KS*32 rows][4]
    float* sT = reinterpret_cast<float*>(sW + KS * 32 * 4);                   // [4 waves][32 x'][16]
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles = tiles_y * tiles_x;
    const int total_tiles = N * tiles;
    // weights: row (ky, j) = w[(ky*NJ + j)*CZ + co], j < NJ; zero rows above.  Staged ONCE: the workgroup is persistent
    // over tiles (one workgroup per tile re-staged these 10 KB - 160 scalar loads + converts per thread - 102 400 times)
    for (int item = tid; item < KS * 32 * 4; item += 256) {
        const int q = item & 3, row = item >> 2, j = row & 31, ky = row >> 5;
        float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (j < NJ) {
            const float* src = w + ((long)(ky * NJ + j)) * CZ + q * 8;
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = src[e];
        }
        const bf16x8 b = pack8(f);
        sW[row * 4 + (q ^ ((row >> 2) & 3))] = *reinterpret_cast<const uint4*>(&b);
    }
    // the next tile travels HBM/L2 -> registers while the current one is multiplied
    constexpr int NPC = (ROWS * 32 * 4 + 255) / 256;
    uint4 pd0[NPC], pd1[NPC];
    uint2 pk[NPC];
    auto fetch = [&](int gt_) {
        const int n_ = gt_ / tiles, tile_ = gt_ % tiles;
        const int u_ = (tile_ / tiles_x) * TH, v_ = (tile_ % tiles_x) * TWO;
#pragma unroll
        for (int qq = 0; qq < NPC; ++qq) {
            const int item = tid + qq * 256;
            const int q = item & 3, pix = item >> 2, xx = pix & 31, rr = pix >> 5;
            const int gy = u_ + rr - (KS - 1 - P), gx = v_ - (KS - 1 - P) + xx;
            pd0[qq] = pd1[qq] = make_uint4(0u, 0u, 0u, 0u);
            pk[qq] = make_uint2(0xffffffffu, 0xffffffffu);
            if (item < ROWS * 32 * 4 && gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const long off = ZMODE >= 1 ? (((long)n_ * (H >> 1) + (gy >> 1)) * (W >> 1) + (gx >> 1)) * CZ + q * 8
                                            : (((long)n_ * H + gy) * W + gx) * CZ + q * 8;
                if constexpr (ZMODE == 2) {
                    pd0[qq] = *reinterpret_cast<const uint4*>(reinterpret_cast<const __bf16*>(dz) + off);
                } else {
                    pd0[qq] = *reinterpret_cast<const uint4*>(dz + off);
                    pd1[qq] = *reinterpret_cast<const uint4*>(dz + off + 4);
                }
                if constexpr (ZMODE >= 1) pk[qq] = *reinterpret_cast<const uint2*>(dz_idx + off);
            }
        }
    };
    const int first_tile = xcd_order(blockIdx.x);      // every round hands each XCD one contiguous range of tiles
    if (first_tile < total_tiles) fetch(first_tile);
    for (int gt = first_tile; gt < total_tiles; gt += gridDim.x) {
    const int n = gt / tiles, tile = gt % tiles;
    const int u0 = (tile / tiles_x) * TH, v0 = (tile % tiles_x) * TWO;
    __syncthreads();                                 // previous tile fully consumed (and the weights staged)
    // dz tile: rows u0-P .. (row index rr <-> image row u0 + rr - (KS-1-P)), 32 column positions from v0-(KS-1-P)
#pragma unroll
    for (int qq = 0; qq < NPC; ++qq) {
        const int item = tid + qq * 256;
        if (item < ROWS * 32 * 4) {
            const int q = item & 3, pix = item >> 2, xx = pix & 31, rr = pix >> 5;
            float f[8];
            if constexpr (ZMODE == 2) {
                const bf16x8 gb = *reinterpret_cast<const bf16x8*>(&pd0[qq]);
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = (float)gb[e];
            } else {
                f[0] = __uint_as_float(pd0[qq].x); f[1] = __uint_as_float(pd0[qq].y);
                f[2] = __uint_as_float(pd0[qq].z); f[3] = __uint_as_float(pd0[qq].w);
                f[4] = __uint_as_float(pd1[qq].x); f[5] = __uint_as_float(pd1[qq].y);
                f[6] = __uint_as_float(pd1[qq].z); f[7] = __uint_as_float(pd1[qq].w);
            }
            if constexpr (ZMODE >= 1) {              // un-pool: this pixel receives the gradient iff it was the window maximum
                const int gy = u0 + rr - (KS - 1 - P), gx = v0 - (KS - 1 - P) + xx;
                const unsigned pos = (unsigned)(((gy & 1) << 1) | (gx & 1));
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    f[e] = ((pk[qq].x >> (8 * e)) & 0xffu) == pos ? f[e] : 0.f;
                    f[4 + e] = ((pk[qq].y >> (8 * e)) & 0xffu) == pos ? f[4 + e] : 0.f;
                }
            }
            const bf16x8 b = pack8(f);
            sD[pix * 4 + (q ^ ((pix >> 2) & 3))] = *reinterpret_cast<const uint4*>(&b);
        }
    }
    __syncthreads();
    if (gt + (int)gridDim.x < total_tiles) fetch(gt + gridDim.x);
    float* myT = sT + wave * 32 * 16;
    for (int ur = wave; ur < TH; ur += 4) {
        f32x16 acc;
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
        // dz row needed for (output row u0+ur, tap ky): image row u0+ur+P-ky  ->  tile row rr = ur + (KS-1) - ky
#pragma unroll
        for (int ky = 0; ky < KS; ++ky) {
            const int pix = (ur + (KS - 1) - ky) * 32 + (lane & 31);
            const int row = ky * 32 + (lane & 31);
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                const int c = h2 * 2 + half;
                const uint4 av = sD[pix * 4 + (c ^ ((pix >> 2) & 3))];
                const uint4 bv = sW[row * 4 + (c ^ ((row >> 2) & 3))];
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&av),
                                                              *reinterpret_cast<const bf16x8*>(&bv), acc, 0, 0, 0);
            }
        }
        // T[x'][j] -> LDS (only the NJ real columns), then the kx shift-add
        if ((lane & 31) < 16) {
#pragma unroll
            for (int j = 0; j < 16; ++j) myT[((j & 3) + 8 * (j >> 2) + 4 * half) * 16 + (lane & 31)] = acc[j];
        }
        __builtin_amdgcn_wave_barrier();             // myT is private to this wave; its LDS operations complete in order
        const int u = u0 + ur;
        for (int o = lane; o < TWO * CI; o += 64) {
            const int vi = o / CI, ci = o % CI, v = v0 + vi;
            float s = 0.f;
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) s += myT[(vi + (KS - 1) - kx) * 16 + kx * CI + ci];
            if (u < H && v < W) out[(((long)n * H + u) * W + v) * CI + ci] = s;
        }
        __builtin_amdgcn_wave_barrier();
    }
    }
}

}  // namespace

// Host side of conv_wgrad_packed_bf16_kernel, called by the weight-gradient dispatch (conv_bf16_wgrad.hip wgrad_bf16_impl).
// Split-K factor: 1024 workgroups' worth, at most one per tile (also what the workspace bound is computed from).
int nimg_internal_wgrad_packed_splits(int cout, int n, int hout, int wout) {
    const long blocks_io = cdiv(cout, cout <= 32 ? 32 : 64);
    const long work = (long)n * cdiv(hout, B_TH) * cdiv(wout, B_TW);
    long splits = (1024 + blocks_io - 1) / blocks_io;
    if (splits > work) splits = work;
    if (splits < 1) splits = 1;
    const long wps = (work + splits - 1) / splits;
    return (int)((work + wps - 1) / wps);
}

template <int KS, int C, int NI>
static int launch_wgrad_packed(const WgradParamsB& q, long pblocks, hipStream_t s) {       // returns the slabs per workgroup
    constexpr size_t lds_t = (size_t)((B_TH + KS - 1) * (B_TW + KS - 1) * C + B_TH * B_TW * 32 * NI) * sizeof(float);
    constexpr int MF = (KS * KS + 32 / C - 1) / (32 / C);
    constexpr bool FOLD = MF * NI <= 2;                     /* as in the kernel */
    constexpr size_t lds_f = FOLD ? (size_t)3 * MF * NI * 16 * 64 * sizeof(float) : 0;
    constexpr size_t lds = lds_t > lds_f ? lds_t : lds_f;
    if (!q.dz_idx)
        hipLaunchKernelGGL((conv_wgrad_packed_bf16_kernel<KS, C, NI, 0>), dim3((unsigned)pblocks), dim3(256), lds, s, q);
    else if (q.flags & NIMG_BF16_DZ)
        hipLaunchKernelGGL((conv_wgrad_packed_bf16_kernel<KS, C, NI, 2>), dim3((unsigned)pblocks), dim3(256), lds, s, q);
    else
        hipLaunchKernelGGL((conv_wgrad_packed_bf16_kernel<KS, C, NI, 1>), dim3((unsigned)pblocks), dim3(256), lds, s, q);
    return FOLD ? 1 : 4;
}

// a: filled by the dispatch (C1 = 3 | 4, C2 = 0, ks = 3 | 5, stride 1; partial = the workspace); tiling, splits and - with want_db -
// db_partial are set here.  Returns the number of dw slabs written (the db slabs: a->splits), -1 on a failed launch.
int nimg_internal_wgrad_packed(WgradArgsB* a, int ks, bool want_db, hipStream_t s) {
    a->tiles_y = cdiv(a->Hout, B_TH); a->tiles_x = cdiv(a->Wout, B_TW);
    a->splits = nimg_internal_wgrad_packed_splits(a->Cout, a->N, a->Hout, a->Wout);
    const long work = (long)a->N * a->tiles_y * a->tiles_x;
    a->work_per_split = (int)((work + a->splits - 1) / a->splits);
    if (want_db) a->db_partial = a->partial + (size_t)4 * a->splits * ks * ks * a->C1 * a->Cout;
    const int ni = a->Cout <= 32 ? 1 : 2;
    const long pblocks = (long)cdiv(a->Cout, 32 * ni) * a->splits;
    const WgradParamsB q{*a};
    int slabs_per_wg;
    if (ks == 5 && q.C1 == 3) slabs_per_wg = ni == 1 ? launch_wgrad_packed<5, 3, 1>(q, pblocks, s) : launch_wgrad_packed<5, 3, 2>(q, pblocks, s);
    else if (ks == 5) slabs_per_wg = ni == 1 ? launch_wgrad_packed<5, 4, 1>(q, pblocks, s) : launch_wgrad_packed<5, 4, 2>(q, pblocks, s);
    else if (q.C1 == 3) slabs_per_wg = ni == 1 ? launch_wgrad_packed<3, 3, 1>(q, pblocks, s) : launch_wgrad_packed<3, 3, 2>(q, pblocks, s);
    else slabs_per_wg = ni == 1 ? launch_wgrad_packed<3, 4, 1>(q, pblocks, s) : launch_wgrad_packed<3, 4, 2>(q, pblocks, s);
    if (hipGetLastError() != hipSuccess) return -1;
    return slabs_per_wg * a->splits;
}

extern "C" {

/* FAN front end in throughput mode.  Few INPUT channels (cin 3|4, float32 HWIO weights, converted in-kernel). */
static int launch_packed_bf16(const float* in, int cin, const float* w, const float* bias, float* out, float* pool_out,
                              unsigned char* pool_idx, int cout, int n, int h, int wd, int ks, int pad_mode, int act,
                              float alpha, hipStream_t s, int out_bf16 = 0) {
    const int ty = cdiv(h, 16), tx = cdiv(wd, 16);
    const long total_tiles = (long)ty * tx * n;
    const int tpw = total_tiles >= 8192 ? 8 : (total_tiles >= 2048 ? 2 : 1);
#define NIMG_FP(KS_, C_, TN_)                                                                                     \
    do {                                                                                                          \
        constexpr int THH = 16 + KS_ - 1, NPIXH = THH * THH, PS = ((NPIXH + 31) / 32) * 32 + 2;                    \
        constexpr int KP = (KS_ * KS_ * C_ + 15) / 16 * 16;                                                       \
        constexpr size_t lds = (size_t)((C_ * PS * 4 + 15) / 16 * 16) + (size_t)TN_ * KP * 2 +                    \
                               (size_t)4 * 32 * (TN_ + EPI_PAD) * sizeof(float);                                  \
        const long blocks = cdiv(total_tiles, tpw) * (long)cdiv(cout, TN_);                                       \
        hipLaunchKernelGGL((conv_fwd_packed_bf16_kernel<KS_, C_, TN_>), dim3((unsigned)blocks), dim3(256), lds, s, \
                           in, w, bias, out, pool_out, pool_idx, n, h, wd, cout, pad_mode, act, alpha, ty, tx, tpw,    \
                           out_bf16);                                                                             \
    } while (0)
    if (ks == 5 && cin == 3) { if (cout > 32) NIMG_FP(5, 3, 64); else NIMG_FP(5, 3, 32); }
    else if (ks == 5 && cin == 4) { if (cout > 32) NIMG_FP(5, 4, 64); else NIMG_FP(5, 4, 32); }
    else if (ks == 3 && cin == 3) { if (cout > 32) NIMG_FP(3, 3, 64); else NIMG_FP(3, 3, 32); }
    else if (ks == 3 && cin == 4) { if (cout > 32) NIMG_FP(3, 4, 64); else NIMG_FP(3, 4, 32); }
    else return NIMG_ERR_ARG;
#undef NIMG_FP
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_conv2d_fwd_smallc_bf16(const float* in, int cin, const float* w, const float* bias, float* out, int cout,
                                int n, int h, int wd, int ks, int pad_mode, int act, float alpha, void* stream) {
    return nimg_conv2d_fwd_smallc_bf16_ex(in, cin, w, bias, out, cout, n, h, wd, ks, pad_mode, act, alpha, 0, stream);
}

/* flags: NIMG_BF16_OUT = out is stored as bf16 (cout % 4 == 0) */
int nimg_conv2d_fwd_smallc_bf16_ex(const float* in, int cin, const float* w, const float* bias, float* out, int cout,
                                   int n, int h, int wd, int ks, int pad_mode, int act, float alpha, int flags, void* stream) {
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    if (!in || !w || !out || n < 0 || h <= 0 || wd <= 0 || cout <= 0 || pad_mode < 0 || pad_mode > 2) return NIMG_ERR_ARG;
    if ((flags & ~NIMG_BF16_OUT) || ((flags & NIMG_BF16_OUT) && (cout & 3))) return NIMG_ERR_ARG;
    return launch_packed_bf16(in, cin, w, bias, out, nullptr, nullptr, cout, n, h, wd, ks, pad_mode, act, alpha,
                              (hipStream_t)stream, (flags & NIMG_BF16_OUT) ? 1 : 0);
}

/* conv (SAME, stride 1) + optional LeakyReLU + 2x2/2 max-pool in one pass, bf16 operands: w = f32 kernel (used when
 * cin <= 4), wb = nimg_conv_weights_bf16(mode 0) image of it (used otherwise) */
int nimg_conv2d_pool_fwd_bf16(const float* in, int cin, const float* w, const void* wb, const float* bias,
                              float* pool_out, unsigned char* pool_idx, int cout, int n, int h, int wd, int ks, int act,
                              float alpha, void* stream) {
    return nimg_conv2d_pool_fwd_bf16_ex(in, cin, w, wb, bias, pool_out, pool_idx, cout, n, h, wd, ks, act, alpha, 0, stream);
}

int nimg_conv2d_pool_fwd_bf16_ex(const float* in, int cin, const float* w, const void* wb, const float* bias,
                                 float* pool_out, unsigned char* pool_idx, int cout, int n, int h, int wd, int ks,
                                 int act, float alpha, int flags, void* stream) {
    return nimg_conv2d_pool_fwd_bf16_sign(in, cin, w, wb, bias, pool_out, pool_idx, nullptr, cout, n, h, wd, ks, act, alpha, flags,
                                          stream);
}

/* The ConvParamsB of the fused conv + pool layer over >= 8 input channels, and whether its tile is the 32-channel one */
static bool pool_fwd_params(ConvParamsB& p, int cin, int cout, int n, int h, int wd, int ks, int act, float alpha, int flags) {
    p.in2 = nullptr; p.out1 = nullptr; p.out2 = nullptr;
    p.act1 = nullptr; p.pool_idx = nullptr; p.convt = 0; p.flags = flags; p.in_idx = nullptr; p.res = nullptr;
    p.out1b = nullptr;
    p.C1 = cin; p.C2 = 0; p.O1 = cout; p.O2 = 0; p.CinP = (cin + 15) / 16 * 16;
    p.N = n; p.H = h; p.W = wd; p.Hout = h; p.Wout = wd; p.pad_t = p.pad_l = (ks - 1) / 2;
    p.tiles_y = p.tiles_x = 0; p.act = act; p.pad_mode = 0; p.alpha = alpha;
    return cout <= 32 || (long)cdiv(cout, 64) * cdiv(h, 16) * cdiv(wd, 16) * n < 384;
}

/* 1 if nimg_conv2d_pool_fwd_bf16_sign with these arguments can write the sign plane (the layer goes to a ring kernel), else 0 */
int nimg_conv2d_pool_sign_ok(int cin, int cout, int n, int h, int wd, int ks, int flags) {
    if (cin <= 0 || cout <= 0 || n <= 0 || h <= 0 || wd <= 0 || (h & 1) || (wd & 1) || ks != 5 || (cin % 8) || (cout & 7)) return 0;
    if ((flags & (NIMG_BF16_IN | NIMG_BF16_OUT)) != (NIMG_BF16_IN | NIMG_BF16_OUT)) return 0;
    ConvParamsB p;
    p.in1 = nullptr; p.wb = nullptr; p.bias = nullptr; p.pool_out = nullptr;
    const bool tn32 = pool_fwd_params(p, cin, cout, n, h, wd, ks, 1, 0.f, flags);
    return conv_bf16_pool_ring_tn(p, tn32) != 0 ? 1 : 0;
}

/* ... and, optionally, the sign plane of the bf16-stored pooled activation (include/nimg.h) */
int nimg_conv2d_pool_fwd_bf16_sign(const float* in, int cin, const float* w, const void* wb, const float* bias,
                                   float* pool_out, unsigned char* pool_idx, unsigned char* pool_sign, int cout, int n, int h,
                                   int wd, int ks, int act, float alpha, int flags, void* stream) {
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    if (!in || !pool_out || cin <= 0 || cout <= 0 || (cout & 3) || n < 0 || h <= 0 || wd <= 0) return NIMG_ERR_ARG;
    if ((h & 1) || (wd & 1) || (ks != 3 && ks != 5) || act < 0 || act > 1) return NIMG_ERR_ARG;
    if (n == 0) return NIMG_OK;
    if (pool_sign && !nimg_conv2d_pool_sign_ok(cin, cout, n, h, wd, ks, flags)) return NIMG_ERR_ARG;    /* no kernel would write it */
    hipStream_t s = (hipStream_t)stream;
    if (cin == 3 || cin == 4) {
        if (!w) return NIMG_ERR_ARG;
        if (flags & NIMG_BF16_IN) return NIMG_ERR_ARG;
        return launch_packed_bf16(in, cin, w, bias, nullptr, pool_out, pool_idx, cout, n, h, wd, ks, 0, act, alpha, s,
                                  (flags & NIMG_BF16_OUT) ? 1 : 0);
    }
    if (!wb || (cin % 8)) return NIMG_ERR_ARG;
    ConvParamsB p;
    const bool tn32 = pool_fwd_params(p, cin, cout, n, h, wd, ks, act, alpha, flags);
    p.in1 = in; p.wb = (const __bf16*)wb; p.bias = bias; p.pool_out = pool_out; p.pool_idx = pool_idx; p.pool_sign = pool_sign;
    if (flags & NIMG_BF16_IN)
        return ks == 3 ? conv_bf16_launch_16x16<3, true>(p, tn32, s) : conv_bf16_launch_16x16<5, true>(p, tn32, s);
    return ks == 3 ? conv_bf16_launch_16x16<3, false>(p, tn32, s) : conv_bf16_launch_16x16<5, false>(p, tn32, s);
}

/* input gradient of a (ks,ks,ci,32) SAME stride-1 convolution towards its ci (= 3) input channels; w = the FORWARD
 * kernel as stored (not flipped) */
static int dgrad_fewin_impl(const float* dz, const unsigned char* dz_idx, int dz_bf16, const float* w, float* out,
                            int ci, int cz, int n, int h, int wd, int ks, void* stream) {
    if (!dz || !w || !out || n < 0 || h <= 0 || wd <= 0) return NIMG_ERR_ARG;
    if (cz != 32 || ci != 3 || ks != 5) return NIMG_ERR_ARG;
    if (n == 0) return NIMG_OK;
    constexpr int KS = 5, TH = 8, TWO = 32 - (KS - 1), ROWS = TH + KS - 1;
    const int ty = cdiv(h, TH), tx = cdiv(wd, TWO);
    constexpr size_t lds = (size_t)(ROWS * 32 * 4 + KS * 32 * 4) * sizeof(uint4) + 4 * 32 * 16 * sizeof(float);
    const long total = (long)n * ty * tx;
    if (total >= (1L << 31)) return NIMG_ERR_ARG;
    const unsigned grid = (unsigned)(total < 4096 ? total : 4096);       // persistent: ~16 workgroups per CU
    hipStream_t s = (hipStream_t)stream;
    if (!dz_idx)
        hipLaunchKernelGGL((conv_dgrad_fewin_bf16_kernel<5, 3, 0>), dim3(grid), dim3(256), lds, s, dz, dz_idx, w, out, n, h, wd,
                           ty, tx);
    else if (dz_bf16)
        hipLaunchKernelGGL((conv_dgrad_fewin_bf16_kernel<5, 3, 2>), dim3(grid), dim3(256), lds, s, dz, dz_idx, w, out, n, h, wd,
                           ty, tx);
    else
        hipLaunchKernelGGL((conv_dgrad_fewin_bf16_kernel<5, 3, 1>), dim3(grid), dim3(256), lds, s, dz, dz_idx, w, out, n, h, wd,
                           ty, tx);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_conv2d_dgrad_fewin_bf16(const float* dz, const float* w, float* out, int ci, int cz, int n, int h, int wd,
                                 int ks, void* stream) {
    return dgrad_fewin_impl(dz, nullptr, 0, w, out, ci, cz, n, h, wd, ks, stream);
}

/* the same input gradient with the output gradient given POOLED (g (n,h/2,wd/2,cz) + arg-max bytes), see
 * nimg_conv2d_wgrad_pooled_bf16 */
int nimg_conv2d_dgrad_fewin_pooled_bf16(const float* g, const unsigned char* idx, const float* w, float* out, int ci,
                                        int cz, int n, int h, int wd, int ks, void* stream) {
    return nimg_conv2d_dgrad_fewin_pooled_bf16_ex(g, idx, w, out, ci, cz, n, h, wd, ks, 0, stream);
}

int nimg_conv2d_dgrad_fewin_pooled_bf16_ex(const float* g, const unsigned char* idx, const float* w, float* out, int ci,
                                           int cz, int n, int h, int wd, int ks, int flags, void* stream) {
    if (!idx || (h & 1) || (wd & 1)) return NIMG_ERR_ARG;
    return dgrad_fewin_impl(g, idx, (flags & NIMG_BF16_DZ) ? 1 : 0, w, out, ci, cz, n, h, wd, ks, stream);
}

}  // extern "C"