// Throughput mode of the convolutions: bf16 operands on the CDNA4 matrix cores (v_mfma_f32_32x32x16_bf16, 16x the f32
// MFMA rate), float32 accumulation, float32 master weights and float32 activations in HBM (converted to bf16 while the
// tiles are staged into LDS).  Same im2col-free implicit GEMM as conv_mfma.hip / conv_wgrad.hip; judged on PSNR /
// accuracy parity, not on the 1e-4 contract (that is the f32 mode).
//
//   forward / input gradient: A tile [pixel][16 ci] bf16 (32 B per pixel, one ds_read_b128 per fragment, 1-bit XOR
//       swizzle of the two 16-byte halves => conflict-free), B tile [tap][co][16 ci] bf16 read the same way from weights
//       that nimg_conv_weights_bf16 lays out once per step as [ci chunk][tap][co][16].
//   weight gradient: K = 16 output pixels per MFMA; the f32 NHWC tiles of conv_wgrad.hip are kept and each lane gathers
//       its 8 pixels with ds_read_b32 (conflict-free) and packs them to bf16 in registers (v_cvt_pk_bf16_f32).
//
// The forward / input-gradient kernels are compiled apart from this file, which took five minutes as one unit: templates in
// conv_bf16_tile.h / _ring.h / _dma.h (shared pieces: conv_bf16.h), one conv_bf16_k*.hip per kernel size and input storage.
// Here: the weight-image converters, the forward entry points, the weight gradient and the FAN front end.
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

// ------------------------------------------------------------------------------------------------------------------
struct WgradParamsB {
    const float* in1;
    const float* in2;
    const float* dz;
    const unsigned char* dz_idx;   // optional (packed kernel): dz is the POOLED gradient (Hout/2 x Wout/2) of a fused
                                   // conv+pool layer and dz_idx its arg-max bytes - the 2x2 un-pooling happens while staging
    float* partial;
    float* db_partial;
    int C1, C2, Cout;
    int N, H, W, Hout, Wout, pad_t, pad_l;
    int tiles_y, tiles_x, splits, work_per_split, pad_mode;
    int flags;                     // NIMG_BF16_IN: in1 (and in2) hold bf16; NIMG_BF16_DZ: dz holds bf16
    // in-kernel finish of the split-K sums by the last-arriving workgroup of a dw tile (common.h ticket_finish); null: slabs only
    unsigned* tickets;
    float* dw;
    float* db;
    int group, accumulate;
    nimg::ReduceEntry pre;         // the reduction the PREVIOUS weight gradient of this stream owes (chained mode), or empty
};

constexpr int B_TH = 8, B_TW = 16, B_CI = 32, B_CO = 64;

template <int KS, int CINP, int NI, int ZMODE>
__global__ void conv_wgrad_packed_bf16_kernel(const WgradParamsB p);      // defined with the FAN front-end kernels below

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
                         unsigned char* pool_idx = nullptr) {
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
    if (!in_idx) return NIMG_ERR_ARG;
    return conv2d_fwd_bf16_impl((const float*)in_pooled, c1, nullptr, 0, wb, bias, out1, o1, nullptr, 0, act_mask, n, h, wd, ks, 1,
                                pad_t, pad_l, 0, hout, wout, act, alpha, flags | NIMG_BF16_IN, stream, in_idx);
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

static int packed_splits_b(int cout, int n, int hout, int wout) {
    const long blocks_io = cdiv(cout, cout <= 32 ? 32 : 64);
    const long work = (long)n * cdiv(hout, B_TH) * cdiv(wout, B_TW);
    long splits = (1024 + blocks_io - 1) / blocks_io;
    if (splits > work) splits = work;
    if (splits < 1) splits = 1;
    const long wps = (work + splits - 1) / splits;
    return (int)((work + wps - 1) / wps);
}

size_t nimg_conv2d_wgrad_bf16_workspace_bytes(int cin, int cout, int ks_h, int ks_w, int n, int hout, int wout) {
    if (cin <= 0 || cout <= 0 || n <= 0) return 0;
    const size_t slab = (size_t)ks_h * ks_w * cin * cout * sizeof(float);
    const size_t generic = (slab + cout * sizeof(float)) * splits_for(cin, cout, n, hout, wout);
    const size_t packed = cin <= 4 ? (4 * slab + cout * sizeof(float)) * packed_splits_b(cout, n, hout, wout) : 0;
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
    const bool tiny = c2 == 0 && c1 == 3 && cout == 3 && stride == 1 && (ks == 3 || ks == 5) && hout == h && wout == wd &&
                      pad_t == (ks - 1) / 2 && pad_l == pad_t && !db;            // tiny filter: its own kernels (conv_small.hip)
    const bool packed = c2 == 0 && (c1 == 3 || c1 == 4) && stride == 1 && (ks == 3 || ks == 5);      // (tap, ci)-packed M dimension
    // the FAN's conv2..4: all 25 taps in one wave (wgrad5.hip)
    const bool fan5 = dz_idx && ks == 5 && stride == 1 && c2 == 0 && pad_t == 2 && pad_l == 2 && hout == h && wout == wd && pad_mode == 0;
    // the kernels of these three have no prologue for the owed reduction: it is launched in front of them.  Every path behind
    // them hands it to its kernel.
    if (tiny || packed || fan5) owed.now();
    if (tiny)
        return nimg_internal_conv_wgrad_tiny(in1, dz, dw, c1, cout, n, h, wd, ks, pad_t, pad_mode, accumulate, workspace,
                                             (hipStream_t)stream, true);          // throughput mode: bf16 matrix operands
    if (packed) {
        WgradParamsB q;
        q.pre = nimg::empty_reduce_entry();
        q.in1 = in1; q.in2 = nullptr; q.dz = dz; q.dz_idx = dz_idx; q.partial = (float*)workspace; q.db_partial = nullptr;
        q.flags = flags;
        q.tickets = nullptr; q.dw = nullptr; q.db = nullptr; q.group = 1; q.accumulate = accumulate;
        q.C1 = c1; q.C2 = 0; q.Cout = cout; q.N = n; q.H = h; q.W = wd; q.Hout = hout; q.Wout = wout;
        q.pad_t = pad_t; q.pad_l = pad_l; q.pad_mode = pad_mode;
        q.tiles_y = cdiv(hout, B_TH); q.tiles_x = cdiv(wout, B_TW);
        q.splits = packed_splits_b(cout, n, hout, wout);
        const long work_ = (long)n * q.tiles_y * q.tiles_x;
        q.work_per_split = (int)((work_ + q.splits - 1) / q.splits);
        const long cnt = (long)ks * ks * cin * cout;
        if (db) q.db_partial = q.partial + (size_t)4 * q.splits * cnt;
        const int ni = cout <= 32 ? 1 : 2;
        const long pblocks = (long)cdiv(cout, 32 * ni) * q.splits;
        hipStream_t s_ = (hipStream_t)stream;
        int slabs_per_wg = 4;
#define NIMG_WGPB(KS_, C_, NI_)                                                                                 \
        do {                                                                                                  \
            constexpr size_t lds_t = (size_t)((B_TH + KS_ - 1) * (B_TW + KS_ - 1) * C_ + B_TH * B_TW * 32 * NI_) * \
                                     sizeof(float);                                                           \
            constexpr int MF_ = (KS_ * KS_ + 32 / C_ - 1) / (32 / C_);                                        \
            constexpr bool FOLD_ = MF_ * NI_ <= 2;                  /* as in the kernel */                        \
            constexpr size_t lds_f = FOLD_ ? (size_t)3 * MF_ * NI_ * 16 * 64 * sizeof(float) : 0;             \
            constexpr size_t lds = lds_t > lds_f ? lds_t : lds_f;                                             \
            slabs_per_wg = FOLD_ ? 1 : 4;                                                                     \
            if (!q.dz_idx)                                                                                    \
                hipLaunchKernelGGL((conv_wgrad_packed_bf16_kernel<KS_, C_, NI_, 0>), dim3((unsigned)pblocks),     \
                                   dim3(256), lds, s_, q);                                                    \
            else if (q.flags & NIMG_BF16_DZ)                                                                  \
                hipLaunchKernelGGL((conv_wgrad_packed_bf16_kernel<KS_, C_, NI_, 2>), dim3((unsigned)pblocks),     \
                                   dim3(256), lds, s_, q);                                                    \
            else                                                                                              \
                hipLaunchKernelGGL((conv_wgrad_packed_bf16_kernel<KS_, C_, NI_, 1>), dim3((unsigned)pblocks),     \
                                   dim3(256), lds, s_, q);                                                    \
        } while (0)
        if (ks == 5 && c1 == 3) { if (ni == 1) NIMG_WGPB(5, 3, 1); else NIMG_WGPB(5, 3, 2); }
        else if (ks == 5) { if (ni == 1) NIMG_WGPB(5, 4, 1); else NIMG_WGPB(5, 4, 2); }
        else if (c1 == 3) { if (ni == 1) NIMG_WGPB(3, 3, 1); else NIMG_WGPB(3, 3, 2); }
        else { if (ni == 1) NIMG_WGPB(3, 4, 1); else NIMG_WGPB(3, 4, 2); }
#undef NIMG_WGPB
        NIMG_CHECK_LAUNCH();
        finish_reduce2(plan, (const float*)workspace, dw, cnt, slabs_per_wg * q.splits, db ? (const float*)q.db_partial : nullptr, db,
                       (long)cout, q.splits, accumulate, s_);
        NIMG_CHECK_LAUNCH();
        return NIMG_OK;
    }
    if ((c1 % 4) || (c2 % 4) || (cout % 4) || (c2 > 0 && (c1 % 8))) return NIMG_ERR_ARG;
    WgradParamsB p;
    p.pre = nimg::empty_reduce_entry();
    p.in1 = in1; p.in2 = in2; p.dz = dz; p.dz_idx = dz_idx; p.partial = (float*)workspace; p.db_partial = nullptr;
    p.flags = flags;
    p.tickets = nullptr; p.dw = dw; p.db = db; p.group = 1; p.accumulate = accumulate;
    p.C1 = c1; p.C2 = c2; p.Cout = cout; p.N = n; p.H = h; p.W = wd; p.Hout = hout; p.Wout = wout;
    p.pad_t = pad_t; p.pad_l = pad_l; p.pad_mode = pad_mode;
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
    const long count = (long)ks * ks * cin * cout;
    hipStream_t s = (hipStream_t)stream;
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

// ==================================================================================================================
// FAN front end in throughput mode (the 3-channel side of the first convolution, models/forensics.py:69): the three
// passes that touch the 256x256x32 tensor are HBM-bound (2.7 GB per 320-image batch each), so they must not waste the
// matrix core on channel padding nor the LDS on re-reads.
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
template <int KS, int CINP, int NI, int ZMODE>
__global__ __launch_bounds__(256) void conv_wgrad_packed_bf16_kernel(const WgradParamsB p) {
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
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    if (!in || !pool_out || cin <= 0 || cout <= 0 || (cout & 3) || n < 0 || h <= 0 || wd <= 0) return NIMG_ERR_ARG;
    if ((h & 1) || (wd & 1) || (ks != 3 && ks != 5) || act < 0 || act > 1) return NIMG_ERR_ARG;
    if (n == 0) return NIMG_OK;
    hipStream_t s = (hipStream_t)stream;
    if (cin == 3 || cin == 4) {
        if (!w) return NIMG_ERR_ARG;
        if (flags & NIMG_BF16_IN) return NIMG_ERR_ARG;
        return launch_packed_bf16(in, cin, w, bias, nullptr, pool_out, pool_idx, cout, n, h, wd, ks, 0, act, alpha, s,
                                  (flags & NIMG_BF16_OUT) ? 1 : 0);
    }
    if (!wb || (cin % 8)) return NIMG_ERR_ARG;
    ConvParamsB p;
    p.in1 = in; p.in2 = nullptr; p.wb = (const __bf16*)wb; p.bias = bias; p.out1 = nullptr; p.out2 = nullptr;
    p.act1 = nullptr; p.pool_out = pool_out; p.pool_idx = pool_idx; p.convt = 0; p.flags = flags; p.in_idx = nullptr; p.res = nullptr;
    p.out1b = nullptr;
    p.C1 = cin; p.C2 = 0; p.O1 = cout; p.O2 = 0; p.CinP = (cin + 15) / 16 * 16;
    p.N = n; p.H = h; p.W = wd; p.Hout = h; p.Wout = wd; p.pad_t = p.pad_l = (ks - 1) / 2;
    p.tiles_y = p.tiles_x = 0; p.act = act; p.pad_mode = 0; p.alpha = alpha;
    const bool tn32 = cout <= 32 || (long)cdiv(cout, 64) * cdiv(h, 16) * cdiv(wd, 16) * n < 384;
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
