// Weight gradient of the throughput-mode convolutions (conv_bf16.hip): bf16 operands on the matrix cores, K = 16 output pixels
// per MFMA, split-K partial sums ("slabs") in a workspace.  The bf16 tiles are staged pixel-major and each lane takes its K-major
// fragment with the LDS transpose read (tr_read8).  Here: the generic kernel, the dispatch over the special families - tiny
// (conv_small.hip), few-channel (conv_bf16_packed.hip), 3x3 / 5x5 all-taps (wgrad3.hip, wgrad5.hip) - and the entry points with
// their ways of carrying the slab reduction (launched, deferred, chained, in-kernel by tickets).
#include "conv_bf16_wgrad.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// ds_read_b64_tr_b16 (gfx950 LDS transpose read).  Measured semantics (tools/probe/tr_probe.hip): inside each 16-lane
// group lane g supplies the 8-byte-aligned address of 4 contiguous bf16; the 16 addresses are read as a 4 x 16 block
// (row = g >> 2, 4-column group = g & 3) and lane g receives COLUMN g of that block: element j = block[j][g].
// With a pixel-major [pixel][channel] tile this hands every lane 4 consecutive PIXELS of its own channel - the K-major
// fragment the weight-gradient GEMM needs - without any transposed copy in LDS.
__device__ __forceinline__ bf16x8 tr_read8(const unsigned char* p0, const unsigned char* p1) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)p0);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)p1);
    s16x8 r;
    r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3]; r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
    return *reinterpret_cast<bf16x8*>(&r);
}

constexpr int B_ZS = 192;      // dz tile row stride in bytes (64 co bf16 = 128 B, padded so 4 rows hit 4 bank quarters)

// NW waves share the taps: 4 for small kernels; 8 for 5x5, where 4 waves would each pin 7 taps x 32 = 224 accumulator
// registers (one wave per SIMD, nothing to hide LDS / barrier latency behind) - with 8 it is 4 taps = 128, two per SIMD.
// TH = output rows per staged tile (8, or 16 for 5x5: the per-tile staging overhead - ~500 instructions of address
// arithmetic, converts and LDS writes - is then amortised over twice as many MFMAs)
// UNP (with DZB): dz is the POOLED gradient (N, Hout/2, Wout/2, Cout) bf16 and p.dz_idx its arg-max bytes; the 2x2 un-pooling
// happens while the dz tile is staged (unp_route: packed byte masks), the full-resolution gradient never exists in HBM.
// NCO = 32-channel output fragments per workgroup: 2 (a 64-wide dz tile) or 1 for layers with Cout <= 32 (UNet level 1), where
// half of the 64-wide tile would be zeros: half the MFMAs, 4 instead of 5 operand reads per pixel row, and the unpadded 64-byte
// tile rows already spread four consecutive pixels over the four bank quarters.
// PAIR (3x3, stride 1, 8 x 8 images - the UNet's bottleneck level): the 8 x 16 tile would be half outside the image (every second
// matrix instruction multiplying zeros).  A tile is then TWO images side by side: columns 0 - 7 = image 2 u, 8 - 15 = image 2 u + 1,
// each with its own zero halo in the input tile ([10][2 x 10] pixels) - the lanes of the second K half read 2 pixels further on.
template <int KS, int STRIDE, int NW, bool INB, bool DZB, int TH, bool UNP = false, int NCO = 2, bool PAIR = false>
__global__ __launch_bounds__(NW * 64, 2) void conv_wgrad_bf16_kernel(const WgradParamsB p) {
    nimg::reduce_entry_inline(p.pre);
    constexpr int TCO = 32 * NCO, ZS = NCO == 2 ? B_ZS : 64, ZI = 4 * NCO;      // dz tile: channels, row stride, 16-byte items per pixel
    static_assert(NCO == 1 || NCO == 2, "one or two output fragments");
    static_assert(!UNP || NCO == 2, "un-pooling dz: 64-wide tile");
    static_assert(!UNP || (DZB && STRIDE == 1), "un-pooling dz: bf16-stored pooled gradient, stride 1");
    constexpr int TAPS = KS * KS, NT = (TAPS + NW - 1) / NW, NTHR = NW * 64;
    static_assert(!PAIR || (KS == 3 && STRIDE == 1 && TH == 8 && INB && DZB && !UNP), "image pairs: the 3x3 layers over 8 x 8 bf16 images");
    constexpr int THH = (TH - 1) * STRIDE + KS, TWH = PAIR ? 20 : (B_TW - 1) * STRIDE + KS;
    constexpr int NPIXH = THH * TWH, NPIX = TH * B_TW;
    static_assert(STRIDE == 1 || STRIDE == 2, "stride");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned char* sI = smem_raw;                   // [NPIXH][32 ci] bf16, 64 B per pixel
    unsigned char* sZ = smem_raw + NPIXH * 64;      // [NPIX][TCO co] bf16, ZS bytes per pixel
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Cin = p.C1 + p.C2;
    const int cib = (Cin + B_CI - 1) / B_CI, cob = (p.Cout + TCO - 1) / TCO;
    int bid = xcd_order(blockIdx.x);
    const int ci0 = (bid % cib) * B_CI;
    bid /= cib;
    const int co0 = (bid % cob) * TCO;
    const int split = bid / cob;
    const int half = lane >> 5, g = lane & 15, sub = (lane >> 4) & 1;

    f32x16 acc[NT][NCO];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int ni = 0; ni < NCO; ++ni)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[t][ni][j] = 0.0f;
    const int tiles = p.tiles_y * p.tiles_x;
    const int work_total = PAIR ? (p.N + 1) / 2 : p.N * tiles;       // < 2^31 (checked by the entry point); PAIR: image pairs
    const int w_begin = split * p.work_per_split;
    const int w_end = min(work_total, w_begin + p.work_per_split);
    const bool do_bias = p.db_partial && ci0 == 0;
    float bacc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // per-lane constant parts of the transpose-read addresses
    const int a_lane = ((half * (PAIR ? 10 : 8) + (g >> 2)) * STRIDE) * 64 + (sub * 16 + (g & 3) * 4) * 2;   // + pixel terms
    const int z_lane = (half * 8 + (g >> 2)) * ZS + (sub * 16 + (g & 3) * 4) * 2;
    // async-stage split: tile t+1 travels HBM -> registers while tile t is multiplied
    constexpr int IP = (NPIXH * 4 + NTHR - 1) / NTHR, ZP = (NPIX * ZI) / NTHR;
    static_assert((NPIX * ZI) % NTHR == 0 && NTHR % ZI == 0, "dz tile must divide over the threads");
    float4 preI[IP][2], preZ[ZP][2];
    uint2 preZK[UNP ? ZP : 1];
    auto fetch = [&](int wk_) {
        const int n_ = (int)(wk_ / tiles), tile_ = (int)(wk_ % tiles);
        const int ty_ = (tile_ / p.tiles_x) * TH, tx_ = (tile_ % p.tiles_x) * B_TW;
        const int iy_ = ty_ * STRIDE - p.pad_t, ix_ = tx_ * STRIDE - p.pad_l;
#pragma unroll
        for (int q = 0; q < IP; ++q) {
            const int item = tid + q * NTHR;
            const int pix = item >> 2, c = ci0 + (item & 3) * 8;
            int gy = iy_ + pix / TWH, gx = ix_ + pix % TWH;
            int ni_ = n_;
            if constexpr (PAIR) {                    // wk_ = image pair: halo columns 0 - 9 image 2 wk_, 10 - 19 image 2 wk_ + 1
                const int hx = pix % TWH;
                ni_ = 2 * wk_ + (hx >= 10 ? 1 : 0);
                gx = (hx >= 10 ? hx - 10 : hx) - 1;
                gy = pix / TWH - 1;
            }
            preI[q][0] = preI[q][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (item < NPIXH * 4 && c < Cin && (!PAIR || ni_ < p.N) && map_coord(gy, p.H, p.pad_mode) && map_coord(gx, p.W, p.pad_mode)) {
                const long pixoff = ((long)ni_ * p.H + gy) * p.W + gx;
                if constexpr (INB) {                 // C1 % 8 == 0, C2 % 8 == 0 (entry point): the 8 channels are one 16-byte load
                    const __bf16* src = c < p.C1 ? reinterpret_cast<const __bf16*>(p.in1) + pixoff * p.C1 + c
                                                 : reinterpret_cast<const __bf16*>(p.in2) + pixoff * p.C2 + (c - p.C1);
                    preI[q][0] = *reinterpret_cast<const float4*>(src);
                } else {
                    const float* src = c < p.C1 ? p.in1 + pixoff * p.C1 + c : p.in2 + pixoff * p.C2 + (c - p.C1);
                    preI[q][0] = *reinterpret_cast<const float4*>(src);
                    if (c + 4 < Cin) preI[q][1] = *reinterpret_cast<const float4*>(src + 4);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < ZP; ++q) {
            const int item = tid + q * NTHR;
            const int pix = item / ZI, c = co0 + (item % ZI) * 8;
            int oy = ty_ + pix / B_TW, ox = tx_ + pix % B_TW, nz_ = n_;
            if constexpr (PAIR) {
                nz_ = 2 * wk_ + ((pix % B_TW) >> 3);
                ox = pix & 7;
                oy = pix / B_TW;
            }
            preZ[q][0] = preZ[q][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (UNP) preZK[q] = make_uint2(0xffffffffu, 0xffffffffu);
            if (oy < p.Hout && ox < p.Wout && c < p.Cout && (!PAIR || nz_ < p.N)) {
                const long zo = UNP ? (((long)n_ * (p.Hout >> 1) + (oy >> 1)) * (p.Wout >> 1) + (ox >> 1)) * p.Cout + c
                                    : (((long)nz_ * p.Hout + oy) * p.Wout + ox) * p.Cout + c;
                if constexpr (UNP) preZK[q] = *reinterpret_cast<const uint2*>(p.dz_idx + zo);
                if constexpr (DZB) {                 // Cout % 8 == 0 (entry point)
                    preZ[q][0] = *reinterpret_cast<const float4*>(reinterpret_cast<const __bf16*>(p.dz) + zo);
                } else {
                    preZ[q][0] = *reinterpret_cast<const float4*>(p.dz + zo);
                    if (c + 4 < p.Cout) preZ[q][1] = *reinterpret_cast<const float4*>(p.dz + zo + 4);
                }
            }
        }
    };
    if (w_begin < w_end) fetch(w_begin);
    for (int wk = w_begin; wk < w_end; ++wk) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < IP; ++q) {
            const int item = tid + q * NTHR;
            if (item < NPIXH * 4) {
                uint4 packed;
                if constexpr (INB) {
                    packed = *reinterpret_cast<const uint4*>(&preI[q][0]);
                } else {
                    const float f[8] = {preI[q][0].x, preI[q][0].y, preI[q][0].z, preI[q][0].w,
                                        preI[q][1].x, preI[q][1].y, preI[q][1].z, preI[q][1].w};
                    const bf16x8 b = pack8(f);
                    packed = *reinterpret_cast<const uint4*>(&b);
                }
                *reinterpret_cast<uint4*>(sI + (item >> 2) * 64 + (item & 3) * 16) = packed;
            }
        }
#pragma unroll
        for (int q = 0; q < ZP; ++q) {
            const int item = tid + q * NTHR;
            float f[8];
            bf16x8 b;
            if constexpr (DZB) {
                if constexpr (UNP) {                 // route: keep a channel iff this pixel was its window's arg-max
                    const int pix_ = item / ZI;      // tile origin (ty, tx) is even: the window position is the pixel's parity
                    const unsigned pos = (unsigned)((((pix_ / B_TW) & 1) << 1) | ((pix_ % B_TW) & 1));
                    const uint4 routed = unp_route(*reinterpret_cast<const uint4*>(&preZ[q][0]), preZK[q].x, preZK[q].y, pos);
                    b = *reinterpret_cast<const bf16x8*>(&routed);
                } else {
                    b = *reinterpret_cast<const bf16x8*>(&preZ[q][0]);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = (float)b[e];
            } else {
                f[0] = preZ[q][0].x; f[1] = preZ[q][0].y; f[2] = preZ[q][0].z; f[3] = preZ[q][0].w;
                f[4] = preZ[q][1].x; f[5] = preZ[q][1].y; f[6] = preZ[q][1].z; f[7] = preZ[q][1].w;
                b = pack8(f);
            }
            if (do_bias) {                      // fused bias gradient in float32: this thread always owns channels q*8..
#pragma unroll
                for (int e = 0; e < 8; ++e) bacc[e] += f[e];
            }
            *reinterpret_cast<uint4*>(sZ + (item / ZI) * ZS + (item % ZI) * 16) = *reinterpret_cast<const uint4*>(&b);
        }
        __syncthreads();
        if (wk + 1 < w_end) fetch(wk + 1);
        // KS == 1 has one tap: the waves share the tile's pixel rows instead (each keeps a partial of the same 32 x 64 block,
        // folded through LDS behind the loop) - with the tap split three of the four waves had nothing to multiply
#pragma unroll 1
        for (int r = (KS == 1 ? wave : 0); r < TH; r += (KS == 1 ? NW : 1)) {
            const unsigned char* zr = sZ + (r * B_TW) * ZS + z_lane;
            bf16x8 bfr[NCO];
#pragma unroll
            for (int ni = 0; ni < NCO; ++ni) bfr[ni] = tr_read8(zr + 64 * ni, zr + 4 * ZS + 64 * ni);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int tap = KS == 1 ? 0 : wave + NW * t;
                if (tap < TAPS) {
                    const unsigned char* ir = sI + ((r * STRIDE + tap / KS) * TWH + (tap % KS)) * 64 + a_lane;
                    const bf16x8 a = tr_read8(ir, ir + 4 * STRIDE * 64);
#pragma unroll
                    for (int ni = 0; ni < NCO; ++ni)
                        acc[t][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bfr[ni], acc[t][ni], 0, 0, 0);
                }
            }
        }
    }
    if (do_bias) {                              // thread t holds channels (t % ZI) * 8 .. + 7: reduce the NTHR / ZI owners
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem_raw);
#pragma unroll
        for (int e = 0; e < 8; ++e) red[tid * 8 + e] = bacc[e];
        __syncthreads();
        if (tid < TCO && co0 + tid < p.Cout) {
            float sum = 0.f;
            for (int o = 0; o < NTHR / ZI; ++o) sum += red[(o * ZI + (tid >> 3)) * 8 + (tid & 7)];
            p.db_partial[(long)split * p.Cout + co0 + tid] = sum;
        }
    }
    if constexpr (KS == 1) {                    // fold the waves' row partials: waves 1.. park theirs in LDS, wave 0 adds in order
        static_assert(NCO == 2 && (NW - 1) * 2 * 16 * 64 * 4 <= NPIXH * 64 + NPIX * B_ZS, "fold scratch fits the tiles");
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem_raw);
        if (wave > 0) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int j = 0; j < 16; ++j) red[(((wave - 1) * 2 + ni) * 16 + j) * 64 + lane] = acc[0][ni][j];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int w = 1; w < NW; ++w)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int j = 0; j < 16; ++j) acc[0][ni][j] += red[(((w - 1) * 2 + ni) * 16 + j) * 64 + lane];
        }
    }
    float* slab = p.partial + (long)split * TAPS * Cin * p.Cout;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int tap = KS == 1 ? 0 : wave + NW * t;
        if (tap >= TAPS || (KS == 1 && wave > 0)) continue;
#pragma unroll
        for (int ni = 0; ni < NCO; ++ni) {
            const int co = co0 + ni * 32 + (lane & 31);
            if (co >= p.Cout) continue;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int ci = ci0 + (j & 3) + 8 * (j >> 2) + 4 * half;
                if (ci < Cin) slab[((long)tap * Cin + ci) * p.Cout + co] = acc[t][ni][j];
            }
        }
    }
    if (p.tickets == nullptr) return;
    // ---- the last workgroup of this (ci block, co block) tile to get here sums the tile over the splits, in a fixed order
    TicketJob job;
    job.cnt = p.tickets + (long)(xcd_order(blockIdx.x) % (cib * cob)) * ticket_words_per_tile_dev(p.splits, p.group);
    job.slab[0] = p.partial; job.stride[0] = (long)TAPS * Cin * p.Cout; job.dst[0] = p.dw;
    job.slab[1] = p.db_partial; job.stride[1] = p.Cout; job.dst[1] = p.db;
    job.splits = p.splits; job.group = p.group; job.accumulate = p.accumulate;
    const int rows = min(B_CI, Cin - ci0), c4n = min(TCO, p.Cout - co0) >> 2, Cout = p.Cout;
    const int witems = TAPS * rows * c4n;
    const int items = witems + ((p.db_partial && ci0 == 0) ? c4n : 0);
    ticket_finish<NTHR>(job, split, items, [=](int it) {
        TicketItem m;
        if (it >= witems) { m.which = 1; m.off = co0 + (it - witems) * 4; return m; }
        const int c4 = it % c4n, row = it / c4n;                 // row = tap * rows + r
        m.which = 0;
        m.off = ((long)(row / rows) * Cin + ci0 + row % rows) * Cout + co0 + c4 * 4;
        return m;
    }, reinterpret_cast<unsigned*>(smem_raw));
}

int splits_for(int cin, int cout, int n, int hout, int wout, int th = B_TH, int target_blocks = 512) {
    const long blocks_io = (long)cdiv(cin, B_CI) * cdiv(cout, B_CO);
    const long work = (long)n * cdiv(hout, th) * cdiv(wout, B_TW);
    long splits = (target_blocks + blocks_io - 1) / blocks_io;
    if (splits > work) splits = work;
    if (splits < 1) splits = 1;
    const long wps = (work + splits - 1) / splits;
    return (int)((work + wps - 1) / wps);
}

}  // namespace

extern "C" {

size_t nimg_conv2d_wgrad_bf16_workspace_bytes(int cin, int cout, int ks_h, int ks_w, int n, int hout, int wout) {
    if (cin <= 0 || cout <= 0 || n <= 0) return 0;
    const size_t slab = (size_t)ks_h * ks_w * cin * cout * sizeof(float);
    const size_t generic = (slab + cout * sizeof(float)) * splits_for(cin, cout, n, hout, wout);
    const size_t packed = cin <= 4 ? (4 * slab + cout * sizeof(float)) * nimg_internal_wgrad_packed_splits(cout, n, hout, wout) : 0;
    const size_t tiny = (cin <= 4 && cout <= 4) ? nimg_internal_wgrad_tiny_bytes(ks_h, cin, cout) : 0;
    const size_t m = generic > packed ? generic : packed;
    return m > tiny ? m : tiny;
}

// What a weight-gradient call does about slab reductions other than launching its own (the plain entries: nothing).
struct ReducePlan {
    nimg::ReduceEntry* defer = nullptr;         // deferred / chained: this call's reduction is described here, not launched
    const nimg::ReduceEntry* pre = nullptr;     // chained: the reduction the PREVIOUS weight gradient of the stream owes
};
static inline void finish_reduce2(const ReducePlan& plan, const float* p1, float* d1, long n1, int splits1, const float* p2,
                                  float* d2, long n2, int splits2, int accumulate, hipStream_t s) {
    if (plan.defer) nimg::fill_reduce_entry(plan.defer, p1, d1, n1, splits1, p2, d2, n2, splits2, accumulate);
    else launch_reduce2(p1, d1, n1, splits1, p2, d2, n2, splits2, accumulate, s);
}
// The owed reduction of a plan runs exactly once: in the prologue of the kernel that carried it (ran_in_kernel(), said once that
// kernel is launched), as a launch of its own otherwise - in front of a path whose kernels have no such prologue (now()), or
// when the call returns before any kernel took it (an argument check, a failed launch).
struct OwedReduction {
    const nimg::ReduceEntry* e;
    hipStream_t s;
    void ran_in_kernel() { e = nullptr; }
    void now() {
        if (e && e->n1 > 0 && e->p1 && e->d1)
            launch_reduce2(e->p1, e->d1, e->n1, e->splits1, e->p2, e->d2, e->n2, e->splits2, e->accumulate, s);
        e = nullptr;
    }
    ~OwedReduction() { now(); }
};

static int wgrad_bf16_impl(const float* in1, int c1, const float* in2, int c2, const float* dz,
                           const unsigned char* dz_idx, int cout, float* dw, float* db, int n, int h, int wd, int ks,
                           int stride, int pad_t, int pad_l, int pad_mode, int hout, int wout, int accumulate,
                           void* workspace, size_t workspace_bytes, int flags, void* stream, const ReducePlan& plan) {
    OwedReduction owed{plan.pre, (hipStream_t)stream};
    if ((flags & NIMG_BF16_IN) && ((c1 & 7) || (c2 & 7))) return NIMG_ERR_ARG;        /* in1 and in2 are both bf16 then */
    if ((flags & NIMG_BF16_DZ) && (cout & 7)) return NIMG_ERR_ARG;
    if (flags && !dz_idx && c2 == 0 && c1 <= 4) return NIMG_ERR_ARG;        /* the packed / tiny kernels stage float32 */
    if (dz_idx && c1 <= 4 && (flags & ~NIMG_BF16_DZ)) return NIMG_ERR_ARG;
    if (dz_idx && c1 > 4 && (flags != (NIMG_BF16_IN | NIMG_BF16_DZ) || stride != 1 || ks != 5 || (hout & 1) || (wout & 1)))
        return NIMG_ERR_ARG;         /* un-pooling dz in the generic kernel: bf16-stored operands of the FAN's 5x5 layers */
    if (!in1 || !dz || !dw || c1 <= 0 || c2 < 0 || cout <= 0 || n <= 0 || h <= 0 || wd <= 0) return NIMG_ERR_ARG;
    if ((c2 > 0 && !in2) || hout <= 0 || wout <= 0 || !workspace || pad_mode < 0 || pad_mode > 2) return NIMG_ERR_ARG;
    const int cin = c1 + c2;
    if (workspace_bytes < nimg_conv2d_wgrad_bf16_workspace_bytes(cin, cout, ks, ks, n, hout, wout)) return NIMG_ERR_WORKSPACE;
    WgradParamsB p;                  // (tiles_y, tiles_x, splits, work_per_split: set by the path that launches)
    p.pre = nimg::empty_reduce_entry();
    p.in1 = in1; p.in2 = in2; p.dz = dz; p.dz_idx = dz_idx; p.partial = (float*)workspace; p.db_partial = nullptr;
    p.flags = flags;
    p.tickets = nullptr; p.dw = dw; p.db = db; p.group = 1; p.accumulate = accumulate;
    p.C1 = c1; p.C2 = c2; p.Cout = cout; p.N = n; p.H = h; p.W = wd; p.Hout = hout; p.Wout = wout;
    p.pad_t = pad_t; p.pad_l = pad_l; p.pad_mode = pad_mode;
    const long count = (long)ks * ks * cin * cout;
    hipStream_t s = (hipStream_t)stream;
    const bool tiny = c2 == 0 && c1 == 3 && cout == 3 && stride == 1 && (ks == 3 || ks == 5) && hout == h && wout == wd &&
                      pad_t == (ks - 1) / 2 && pad_l == pad_t && !db;            // tiny filter: its own kernels (conv_small.hip)
    const bool packed = c2 == 0 && (c1 == 3 || c1 == 4) && stride == 1 && (ks == 3 || ks == 5);      // (tap, ci)-packed M dimension
    // the FAN's conv2..4: all 25 taps in one wave (wgrad5.hip)
    const bool fan5 = dz_idx && ks == 5 && stride == 1 && c2 == 0 && pad_t == 2 && pad_l == 2 && hout == h && wout == wd && pad_mode == 0;
    // the kernels of these three have no prologue for the owed reduction: it is launched in front of them.  Every path behind
    // them hands it to its kernel.
    if (tiny || packed || fan5) owed.now();
    if (tiny)
        return nimg_internal_conv_wgrad_tiny(in1, dz, dw, c1, cout, n, h, wd, ks, pad_t, pad_mode, accumulate, workspace, s,
                                             true);          // throughput mode: bf16 matrix operands
    if (packed) {                  // conv_bf16_packed.hip: one input, slabs only (no in-kernel finish), its own tiling and splits
        p.in2 = nullptr; p.dw = nullptr; p.db = nullptr;
        const int slabs = nimg_internal_wgrad_packed(&p, ks, db != nullptr, s);
        if (slabs < 0) return NIMG_ERR_LAUNCH;
        finish_reduce2(plan, (const float*)workspace, dw, count, slabs, p.db_partial, db, (long)cout, p.splits, accumulate, s);
        NIMG_CHECK_LAUNCH();
        return NIMG_OK;
    }
    if ((c1 % 4) || (c2 % 4) || (cout % 4) || (c2 > 0 && (c1 % 8))) return NIMG_ERR_ARG;
    // arrival counters for the in-kernel finish of the generic kernel's split-K sums (set once p.splits is final)
    auto want_tickets = [&](WgradParamsB& w) {
        if (plan.defer || (((uintptr_t)dw | (uintptr_t)db) & 15)) return;
        w.group = ticket_group(w.splits);
        w.tickets = nimg_internal_tickets((hipStream_t)stream, (size_t)cdiv(cin, B_CI) * cdiv(cout, B_CO) * ticket_words_per_tile(w.splits));
    };
    const int th = (stride == 1 && ks == 5) ? 16 : B_TH;
    p.tiles_y = cdiv(hout, th); p.tiles_x = cdiv(wout, B_TW);
    // the 8-wave 5x5 kernel runs ONE workgroup per CU: 256 workgroups are one full round, and half the slabs to write and reduce
    static const int wg5_env = getenv("NIMG_WGRAD5_BLOCKS") ? atoi(getenv("NIMG_WGRAD5_BLOCKS")) : 256;
    const int wg5 = wg5_env < 32 ? 32 : (wg5_env > 512 ? 512 : wg5_env);        // 512 = what the workspace bound assumes
    p.splits = splits_for(cin, cout, n, hout, wout, th, (stride == 1 && ks == 5) ? wg5 : 512);   // <= splits_for(.., B_TH): the workspace bound holds
    const long work = (long)n * p.tiles_y * p.tiles_x;
    p.work_per_split = (int)((work + p.splits - 1) / p.splits);
    if (fan5) {                    // slabs laid out inside the same workspace bound
        const int max_slabs = splits_for(cin, cout, n, hout, wout);
        float* dbp = db ? (float*)workspace + (size_t)max_slabs * count : nullptr;
        const int slabs = nimg_internal_wgrad5_alltaps(in1, cin, dz, dz_idx, cout, (float*)workspace, dbp, n, h, wd, max_slabs, s);
        if (slabs < 0) return NIMG_ERR_LAUNCH;
        if (slabs > 0) {
            finish_reduce2(plan, (const float*)workspace, dw, count, slabs, dbp, db, (long)cout, slabs, accumulate, s);
            NIMG_CHECK_LAUNCH();
            return NIMG_OK;
        }
    }
    if (!dz_idx && ks == 3 && stride == 1 && pad_t == 1 && pad_l == 1 && hout == h && wout == wd && pad_mode == 0 &&
        flags == (NIMG_BF16_IN | NIMG_BF16_DZ)) {
        // the UNet's 3x3 layers with bf16-stored tensors: all 9 taps in one wave, double-buffered tiles (wgrad3.hip)
        const int max_slabs = splits_for(cin, cout, n, hout, wout);
        float* dbp = db ? (float*)workspace + (size_t)max_slabs * count : nullptr;
        const int slabs = nimg_internal_wgrad3_alltaps(in1, c1, in2, c2, dz, cout, (float*)workspace, dbp, n, h, wd, max_slabs, s,
                                                       plan.defer ? nullptr : dw, db, accumulate, owed.e);
        if (slabs != 0) owed.ran_in_kernel();                 // launched: its prologue runs the chained reduction
        if (slabs == -1) return NIMG_ERR_LAUNCH;
        if (slabs < -1) return NIMG_OK;                       // finished in the kernel by the last-arriving workgroups
        if (slabs > 0) {
            finish_reduce2(plan, (const float*)workspace, dw, count, slabs, dbp, db, (long)cout, slabs, accumulate, s);
            NIMG_CHECK_LAUNCH();
            return NIMG_OK;
        }
    }
    // 8 x 8 images (the UNet's bottleneck level): tiles of two images side by side instead of 8 x 16 tiles that are half empty
    static const bool no_pair = getenv("NIMG_NO_WGRAD_PAIR8") != nullptr;
    if (!no_pair && !dz_idx && ks == 3 && stride == 1 && h == 8 && wd == 8 && hout == 8 && wout == 8 && pad_t == 1 && pad_l == 1 &&
        pad_mode == 0 && flags == (NIMG_BF16_IN | NIMG_BF16_DZ) && n >= 2) {
        const long pairs = (n + 1) / 2;
        long sp = p.splits < pairs ? p.splits : pairs;
        const long wps = (pairs + sp - 1) / sp;
        sp = (pairs + wps - 1) / wps;
        p.splits = (int)sp; p.work_per_split = (int)wps; p.tiles_y = p.tiles_x = 1;
        if (db) p.db_partial = p.partial + (size_t)p.splits * count;
        const long pblocks = (long)cdiv(cin, B_CI) * cdiv(cout, B_CO) * p.splits;
        constexpr size_t lds = (size_t)10 * 20 * 64 + (size_t)B_TH * B_TW * B_ZS;
        auto k = conv_wgrad_bf16_kernel<3, 1, 4, true, true, B_TH, false, 2, true>;
        (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        want_tickets(p);
        if (owed.e) p.pre = *owed.e;
        hipLaunchKernelGGL(k, dim3((unsigned)pblocks), dim3(256), lds, s, p);
        NIMG_CHECK_LAUNCH();
        owed.ran_in_kernel();
        if (p.tickets) return NIMG_OK;
        finish_reduce2(plan, (const float*)workspace, dw, count, p.splits, db ? (const float*)p.db_partial : nullptr, db, (long)cout,
                       p.splits, accumulate, s);
        NIMG_CHECK_LAUNCH();
        return NIMG_OK;
    }
    if (db) p.db_partial = p.partial + (size_t)p.splits * count;
    const long blocks = (long)cdiv(cin, B_CI) * cdiv(cout, B_CO) * p.splits;
    want_tickets(p);
    if (owed.e) p.pre = *owed.e;
#define NIMG_WGB1(KS_, ST_, NW_, INB_, DZB_, TH_)                                                               \
    do {                                                                                                      \
        constexpr int THH = (TH_ - 1) * ST_ + KS_, TWH = (B_TW - 1) * ST_ + KS_;                              \
        constexpr size_t lds_t = (size_t)THH * TWH * 64 + (size_t)TH_ * B_TW * B_ZS;                          \
        constexpr size_t lds = lds_t > (size_t)NW_ * 64 * 8 * 4 ? lds_t : (size_t)NW_ * 64 * 8 * 4;          \
        auto k = conv_wgrad_bf16_kernel<KS_, ST_, NW_, INB_, DZB_, TH_>;                                      \
        if constexpr (KS_ == 3 && ST_ == 1) {                  /* narrow outputs: a 32-wide dz tile */            \
            static const bool no_narrow = getenv("NIMG_NO_NARROW_WGRAD") != nullptr;                          \
            if (!no_narrow && p.Cout <= 32 && !p.dz_idx) k = conv_wgrad_bf16_kernel<KS_, ST_, NW_, INB_, DZB_, TH_, false, 1>;  \
        }                                                                                                     \
        if (p.dz_idx) {                                                                                       \
            if constexpr (DZB_ && ST_ == 1 && KS_ == 5) k = conv_wgrad_bf16_kernel<KS_, ST_, NW_, INB_, true, TH_, true>;    \
            else return NIMG_ERR_ARG;                                                                         \
        }                                                                                                     \
        (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);      \
        hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(NW_ * 64), lds, s, p);                             \
    } while (0)
#define NIMG_WGB(KS_, ST_)                                                                                     \
    do {                                                                                                      \
        constexpr int NW = KS_ == 5 ? 8 : 4;                                                                  \
        constexpr int TH_ = (KS_ == 5 && ST_ == 1) ? 16 : B_TH;                                               \
        /* bf16-stored operands: the stride-1 layers and the 2x2 / stride-2 form (UNet Conv2DTranspose weight gradient) */ \
        constexpr bool BFOK = ST_ == 1 || KS_ == 2;                                                           \
        constexpr int S1 = BFOK ? ST_ : 1;                                                                    \
        constexpr int T1 = BFOK ? TH_ : B_TH;                                                                 \
        if (BFOK && (p.flags & NIMG_BF16_IN) && (p.flags & NIMG_BF16_DZ)) NIMG_WGB1(KS_, S1, NW, true, true, T1);    \
        else if (BFOK && (p.flags & NIMG_BF16_IN)) NIMG_WGB1(KS_, S1, NW, true, false, T1);                   \
        else if (BFOK && (p.flags & NIMG_BF16_DZ)) NIMG_WGB1(KS_, S1, NW, false, true, T1);                   \
        else if (p.flags) return NIMG_ERR_ARG;                                                                \
        else NIMG_WGB1(KS_, ST_, NW, false, false, TH_);                                                      \
    } while (0)
    if (stride == 1 && ks == 1) NIMG_WGB(1, 1);
    else if (stride == 1 && ks == 3) NIMG_WGB(3, 1);
    else if (stride == 1 && ks == 5) NIMG_WGB(5, 1);
    else if (stride == 2 && ks == 2) NIMG_WGB(2, 2);
    else if (stride == 2 && ks == 5) NIMG_WGB(5, 2);
    else return NIMG_ERR_ARG;
#undef NIMG_WGB
#undef NIMG_WGB1
    NIMG_CHECK_LAUNCH();
    owed.ran_in_kernel();
    if (p.tickets) return NIMG_OK;
    finish_reduce2(plan, (const float*)workspace, dw, count, p.splits, db ? (const float*)p.db_partial : nullptr, db, (long)cout,
                   p.splits, accumulate, s);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_conv2d_wgrad_bf16(const float* in1, int c1, const float* in2, int c2, const float* dz, int cout, float* dw,
                           float* db, int n, int h, int wd, int ks, int stride, int pad_t, int pad_l, int pad_mode,
                           int hout, int wout, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    return wgrad_bf16_impl(in1, c1, in2, c2, dz, nullptr, cout, dw, db, n, h, wd, ks, stride, pad_t, pad_l, pad_mode, hout,
                           wout, accumulate, workspace, workspace_bytes, 0, stream, ReducePlan{});
}

int nimg_conv2d_wgrad_bf16_ex(const float* in1, int c1, const float* in2, int c2, const float* dz, int cout, float* dw,
                              float* db, int n, int h, int wd, int ks, int stride, int pad_t, int pad_l, int pad_mode,
                              int hout, int wout, int accumulate, void* workspace, size_t workspace_bytes, int flags,
                              void* stream) {
    return wgrad_bf16_impl(in1, c1, in2, c2, dz, nullptr, cout, dw, db, n, h, wd, ks, stride, pad_t, pad_l, pad_mode, hout,
                           wout, accumulate, workspace, workspace_bytes, flags, stream, ReducePlan{});
}

/* Weight (+bias) gradient of a fused conv + pool layer with MANY input channels (the FAN's conv2..4, 5x5, stride 1, SAME) from
 * the POOLED gradient: in (n,h,wd,cin) bf16, g (n,h/2,wd/2,cout) bf16 already multiplied by LeakyReLU', idx its arg-max bytes.
 * The 2x2 un-pooling happens while the gradient tile is staged.  cin % 8 == 0, cout % 8 == 0, h, wd even. */
int nimg_conv2d_wgrad_bf16_unpool(const void* in, int cin, const void* g, const unsigned char* idx, int cout, float* dw, float* db,
                                  int n, int h, int wd, int ks, int accumulate, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    if (!idx || ks != 5 || (h & 1) || (wd & 1)) return NIMG_ERR_ARG;
    return wgrad_bf16_impl((const float*)in, cin, nullptr, 0, (const float*)g, idx, cout, dw, db, n, h, wd, ks, 1, 2, 2, 0, h, wd,
                           accumulate, workspace, workspace_bytes, NIMG_BF16_IN | NIMG_BF16_DZ, stream, ReducePlan{});
}

/* DEFERRED forms of nimg_conv2d_wgrad_bf16_ex / _unpool (idx != null): the split-K partial sums are written to `workspace`, the
 * slab reduction is NOT launched - it is described in *entry (nimg_reduce_entry_bytes() bytes of host memory) for a later
 * nimg_reduce_slabs_batch() on the same stream.  The workspace must stay untouched until then.  accumulate must be 0. */
int nimg_conv2d_wgrad_bf16_deferred(const void* in1, int c1, const void* in2, int c2, const void* dz, const unsigned char* idx,
                                    int cout, float* dw, float* db, int n, int h, int wd, int ks, int stride, int pad_t, int pad_l,
                                    int pad_mode, int hout, int wout, void* workspace, size_t workspace_bytes, int flags,
                                    void* entry, void* stream) {
    if (!entry) return NIMG_ERR_ARG;
    nimg::ReduceEntry* e = reinterpret_cast<nimg::ReduceEntry*>(entry);
    nimg::fill_reduce_entry(e, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, 0, 0);          // n1 == 0: nothing owed (paths that reduce themselves)
    e->blocks1 = 0;
    return wgrad_bf16_impl((const float*)in1, c1, (const float*)in2, c2, (const float*)dz, idx, cout, dw, db, n, h, wd, ks, stride,
                           pad_t, pad_l, pad_mode, hout, wout, 0, workspace, workspace_bytes, flags, stream, ReducePlan{e, nullptr});
}

/* nimg_conv2d_wgrad_bf16_deferred that also runs the reduction a PREVIOUS deferred / chained call on the same stream owes
 * (pre_entry, may be NULL): in the prologue of this call's kernel where that kernel can (the UNet's 3x3 all-taps kernel, the generic
 * bf16 kernel), as a separate launch in front of it otherwise.  Bit-identical sums (common.h reduce_seq). */
int nimg_conv2d_wgrad_bf16_chained(const void* in1, int c1, const void* in2, int c2, const void* dz, const unsigned char* idx,
                                   int cout, float* dw, float* db, int n, int h, int wd, int ks, int stride, int pad_t, int pad_l,
                                   int pad_mode, int hout, int wout, void* workspace, size_t workspace_bytes, int flags,
                                   const void* pre_entry, void* entry, void* stream) {
    if (!entry) return NIMG_ERR_ARG;
    nimg::ReduceEntry pre_copy;
    if (pre_entry) pre_copy = *reinterpret_cast<const nimg::ReduceEntry*>(pre_entry);        // (entry may alias pre_entry)
    nimg::ReduceEntry* e = reinterpret_cast<nimg::ReduceEntry*>(entry);
    *e = nimg::empty_reduce_entry();
    return wgrad_bf16_impl((const float*)in1, c1, (const float*)in2, c2, (const float*)dz, idx, cout, dw, db, n, h, wd, ks, stride,
                           pad_t, pad_l, pad_mode, hout, wout, 0, workspace, workspace_bytes, flags, stream,
                           ReducePlan{e, pre_entry ? &pre_copy : nullptr});
}

size_t nimg_reduce_entry_bytes(void) { return sizeof(nimg::ReduceEntry); }
int nimg_reduce_batch_max(void) { return nimg::REDUCE_BATCH_MAX; }

/* The reductions owed by up to nimg_reduce_batch_max() deferred weight gradients, one launch; entries = n x
 * nimg_reduce_entry_bytes() bytes of HOST memory as the deferred calls filled them (entries that owe nothing are skipped). */
int nimg_reduce_slabs_batch(const void* entries, int n, void* stream) {
    if (n == 0) return NIMG_OK;
    if (!entries || n < 0 || n > nimg::REDUCE_BATCH_MAX) return NIMG_ERR_ARG;
    const nimg::ReduceEntry* src = reinterpret_cast<const nimg::ReduceEntry*>(entries);
    nimg::ReduceBatch b;
    b.n = 0;
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        if (src[i].n1 <= 0 || !src[i].p1 || !src[i].d1) continue;
        b.e[b.n] = src[i];
        b.first_block[b.n] = blocks;
        blocks += src[i].blocks1 + ((src[i].p2 && src[i].d2) ? nimg::reduce_grid(src[i].n2) : 0);
        ++b.n;
    }
    b.first_block[b.n] = blocks;
    if (b.n == 0) return NIMG_OK;
    hipLaunchKernelGGL(nimg::reduce_slabs_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, b);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

/* Weight (+bias) gradient of a fused conv+pool layer (nimg_conv2d_pool_fwd_bf16) with few input channels (cin 3|4):
 * the output gradient arrives POOLED - g (n,h/2,wd/2,cout), already multiplied by LeakyReLU'(pooled) - with the
 * arg-max bytes of the forward pass; the sparse full-resolution gradient is never materialised. */
int nimg_conv2d_wgrad_pooled_bf16(const float* in, int cin, const float* g, const unsigned char* idx, int cout,
                                  float* dw, float* db, int n, int h, int wd, int ks, int accumulate, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    return nimg_conv2d_wgrad_pooled_bf16_ex(in, cin, g, idx, cout, dw, db, n, h, wd, ks, accumulate, workspace,
                                            workspace_bytes, 0, stream);
}

/* flags: NIMG_BF16_DZ = the pooled gradient g is stored as bf16 */
int nimg_conv2d_wgrad_pooled_bf16_ex(const float* in, int cin, const float* g, const unsigned char* idx, int cout,
                                     float* dw, float* db, int n, int h, int wd, int ks, int accumulate, void* workspace,
                                     size_t workspace_bytes, int flags, void* stream) {
    if (!idx || (cin != 3 && cin != 4) || (ks != 3 && ks != 5) || (h & 1) || (wd & 1) || (cout & 3)) return NIMG_ERR_ARG;
    return wgrad_bf16_impl(in, cin, nullptr, 0, g, idx, cout, dw, db, n, h, wd, ks, 1, (ks - 1) / 2, (ks - 1) / 2, 0, h, wd,
                           accumulate, workspace, workspace_bytes, flags & NIMG_BF16_DZ, stream, ReducePlan{});
}

}  // extern "C"
