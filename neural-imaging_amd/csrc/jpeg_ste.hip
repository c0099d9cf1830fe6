// The real JPEG codec as one differentiable-training forward: x (n,h,w,3) float32 -> the image libjpeg decodes
// from the file it would write for x, as float32 byte / 255, plus the clip mask the dJPEG backward kernels (djpeg.hip, djpeg_sub.hip)
// consume.  A straight-through estimator's forward: the backward stays nimg_djpeg_bwd / _bwd_dq / nimg_djpeg_sub_bwd at the same x.
//
// Every integer step is jpegc.h's, shared with the codec's own kernels - byte_of, luma_of / chroma_of and downsample_of (the h2v1 /
// h2v2 rule) of sample(), fdct8, quantise_coef, idct8, limit_byte, fancy_h2v1 / fancy_column / fancy_h2v2 of chroma_at, red_of /
// green_of / blue_of - so y is bit-identical to nimg_jpeg_transform_tables followed by nimg_jpeg_reconstruct_tables wherever every value of x lies in [0, 1].  What differs on purpose: there is NO batch-wide "some value
// exceeds 1" flag.  A value above 1 clamps to 255 here (byte_of with div = false), where the transform would divide the whole batch by
// 255 first; a step of a training loop can neither afford the extra pass over x nor a result that depends on the rest of the batch.
//
// mask (n,h,w) uint8, the layout of nimg_djpeg_fwd: bit c is set iff output channel c (red_of, green_of, blue_of) lies in 0..255
// BEFORE its range limit.  The range limit that ends the inverse DCT (limit_byte of a component sample) is not part of the mask: the float model
// has no clip there, so its adjoint has nowhere to apply one.
//
// Work decomposition, djpeg.hip's and djpeg_sub.hip's: a wave owns a strip of 8 rows x up to 64 samples, lane (b = lane >> 3,
// r = lane & 7) holds row r of block b; 8x8 transposes between the passes go through the wave's private LDS tile.
//   4:4:4            one launch.  x and y move as 16-byte strip loads / stores through the wave's LDS rows (djpeg.h); only x, y and the
//                    mask touch HBM: 12 + 12 + 1 B per pixel.
//   4:2:2 / 4:2:0    chroma pass: lane (b, r) reads the 16 x vs pixels under its 8 reduced samples as 16-byte loads, down-samples them
//                    (chroma_of, downsample_of), runs Cb and Cr through the block path and writes the reconstructed bytes to the
//                    workspace [n][Cb | Cr][h / vs][w / 2], 2 / (hs vs) B per pixel.  luma pass: the strip of the 4:4:4 kernel with
//                    the Y path in registers; the reduced samples under the lane's 8 pixels with their one-sample halo, at indices
//                    clamped at the component's edge, up-sampled (fancy_h2v1 / fancy_h2v2), then colour, limit, y and mask.
// Plain vector stores only, no atomics, no allocation, no synchronisation, nothing read back: the call can be captured.
#include "djpeg.h"
#include "jpegc.h"

namespace {

using namespace nimg;
using namespace nimg::dj;

constexpr int WAVES_PER_BLOCK = 4;
constexpr int TILE_W = 8 * 72;                                    // one channel's transpose tiles of a wave: [block][8][9] words
constexpr int STE_WAVE_W = STAGE_F > 3 * TILE_W ? STAGE_F : 3 * TILE_W;       // 4:4:4: staging rows or three tiles, whichever is larger
constexpr int Q_WORDS = 192;
constexpr size_t kLds444 = ((size_t)WAVES_PER_BLOCK * STE_WAVE_W + Q_WORDS) * 4;
constexpr size_t kLdsLuma = ((size_t)WAVES_PER_BLOCK * STAGE_F + Q_WORDS) * 4;
constexpr size_t kLdsChroma = ((size_t)WAVES_PER_BLOCK * 2 * TILE_W + Q_WORDS) * 4;

// The table set of the call in LDS, transposed to [c][r][k] so that lane (b, r) finds the 8 entries of its column (natural index
// 8 k + r) in two 16-byte reads.  An entry outside 1..255 is clamped, the rule of nimg_jpeg_transform_tables, and the first workgroup
// says so in *err: one thread, a plain read and a plain store.
__device__ __forceinline__ void stage_qtabs(const uint16_t* __restrict__ qtabs, int* qT, int* __restrict__ err) {
    const int tid = threadIdx.x;
    bool bad = false;
    if (tid < Q_WORDS) {
        const int q = qtabs[tid];
        bad = q < 1 || q > 255;
        qT[((tid >> 6) * 8 + (tid & 7)) * 8 + ((tid >> 3) & 7)] = min(max(q, 1), 255);
    }
    const int any = __syncthreads_or(bad ? 1 : 0);
    if (err && any && blockIdx.x == 0 && tid == 0) *err = *err | 1;
}

// NC components of the strip through the codec: lane (b, r) brings row r of its blocks as samples - 128 and leaves with the
// reconstructed samples 0..255 of that row.  comp0 = the table of d[0]; the tables of the others follow it.
template <int NC>
__device__ __forceinline__ void codec_blocks(int (&d)[NC][8], int* tile, const int* qT, int comp0, int b, int r) {
#pragma unroll
    for (int c = 0; c < NC; ++c) fdct8<1, true>(d[c]);
    transpose_tiles<NC>(tile, b, r, d);                             // lane now holds column r
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        fdct8<1, false>(d[c]);
        const int4 q0 = *reinterpret_cast<const int4*>(qT + ((comp0 + c) * 8 + r) * 8);
        const int4 q1 = *reinterpret_cast<const int4*>(qT + ((comp0 + c) * 8 + r) * 8 + 4);
        const int q[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) d[c][k] = (int)(short)quantise_coef(d[c][k], q[k]) * q[k];      // the file's int16, dequantised
        idct8<1>(d[c], 11);
    }
    transpose_tiles<NC>(tile, b, r, d);                             // lane holds row r again
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        idct8<1>(d[c], 18);
#pragma unroll
        for (int j = 0; j < 8; ++j) d[c][j] = limit_byte(d[c][j] + 128);
    }
}

// the 8 pixels of lane (b, r) from their reconstructed components: colour, mask bits, limit, k / 255 into px; returns the mask bytes
__device__ __forceinline__ uint2 finish_row(const int (&yy)[8], const int (&cb)[8], const int (&cr)[8], float (&px)[24]) {
    uint32_t mlo = 0, mhi = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int v[3] = {red_of(yy[j], cr[j] - 128), green_of(yy[j], cb[j] - 128, cr[j] - 128), blue_of(yy[j], cb[j] - 128)};
        uint32_t m = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            m |= (unsigned)v[c] <= 255u ? (1u << c) : 0u;
            px[3 * j + c] = __fdiv_rn((float)limit_byte(v[c]), 255.0f);
        }
        if (j < 4) mlo |= m << (8 * j); else mhi |= m << (8 * (j - 4));
    }
    return make_uint2(mlo, mhi);
}

__global__ __launch_bounds__(256) void jpeg_ste_444_kernel(const float* __restrict__ x, const uint16_t* __restrict__ qtabs,
                                                           float* __restrict__ y, uint8_t* __restrict__ mask, int* __restrict__ err,
                                                           int n, int h, int w) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = lane >> 3, r = lane & 7;
    float* lds = smem + wave * STE_WAVE_W;
    int* qT = reinterpret_cast<int*>(smem + WAVES_PER_BLOCK * STE_WAVE_W);
    const int hb = h / 8, strips = (w + STRIP_PX - 1) / STRIP_PX;
    const Task t = decode_task((long)blockIdx.x * WAVES_PER_BLOCK + wave, (long)n * hb * strips, hb, strips);
    const bool active = t.valid && (t.x0 + b * 8 < w);

    f32x4 pre[6] = {};
    fetch_strip(x, pre, t, h, w, lane);                              // in flight while the tables are staged
    stage_qtabs(qtabs, qT, err);
    commit_strip(lds, pre, lane);
    wave_sync();
    float px[24];
    read_row24(lds, b, r, px);
    wave_sync();
    int d[3][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int R = byte_of(px[3 * j], false), G = byte_of(px[3 * j + 1], false), B = byte_of(px[3 * j + 2], false);
        d[0][j] = luma_of(R, G, B) - 128;
        d[1][j] = chroma_of(1, R, G, B) - 128;
        d[2][j] = chroma_of(2, R, G, B) - 128;
    }
    codec_blocks<3>(d, reinterpret_cast<int*>(lds), qT, 0, b, r);
    const uint2 m = finish_row(d[0], d[1], d[2], px);
    write_row24(lds, b, r, px);
    if (mask && active) *reinterpret_cast<uint2*>(mask + ((long)t.n * h + t.by * 8 + r) * w + t.x0 + b * 8) = m;
    wave_sync();
    store_strip(y, lds, t, h, w, lane);
}

// the reduced planes of image `img` in the workspace: Cb, then Cr, cew bytes a row (whole MCUs: cew = 8 bwC, chroma_at's stride)
__device__ __forceinline__ uint8_t* reduced_plane(uint8_t* planes, const JpegGeo& g, int img, int c) {
    return planes + ((size_t)img * 2 + c) * g.ceh * g.cew;
}

// lane (b, r) of a chroma task: the 16 x VS pixels under its 8 reduced samples as 12 float4 per pixel row (w % 16 == 0 keeps every
// 48-float granule 16-byte aligned), each to bytes, to Cb and Cr, summed over its 2 x VS group and divided by downsample_of
template <int VS>
__device__ __forceinline__ void reduced_chroma(const float* __restrict__ x, const Task& t, const JpegGeo& g, int b, int r, int (&d)[2][8]) {
#pragma unroll
    for (int vv = 0; vv < VS; ++vv) {
        const f32x4* p = reinterpret_cast<const f32x4*>(x + (((long)t.n * g.h + (t.by * 8 + r) * VS + vv) * g.w + (t.x0 + b * 8) * 2) * 3);
        f32x4 raw[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) raw[k] = p[k];
        float px[48];
#pragma unroll
        for (int k = 0; k < 12; ++k) { px[4 * k] = raw[k].x; px[4 * k + 1] = raw[k].y; px[4 * k + 2] = raw[k].z; px[4 * k + 3] = raw[k].w; }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int R = byte_of(px[3 * j], false), G = byte_of(px[3 * j + 1], false), B = byte_of(px[3 * j + 2], false);
            d[0][j >> 1] += chroma_of(1, R, G, B);
            d[1][j >> 1] += chroma_of(2, R, G, B);
        }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) d[c][j] = downsample_of(d[c][j], VS, t.x0 + b * 8 + j) - 128;
}

template <int VS>
__global__ __launch_bounds__(256) void jpeg_ste_chroma_kernel(const float* __restrict__ x, const uint16_t* __restrict__ qtabs,
                                                              uint8_t* __restrict__ planes, JpegGeo g) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = lane >> 3, r = lane & 7;
    int* tile = reinterpret_cast<int*>(smem) + wave * 2 * TILE_W;
    int* qT = reinterpret_cast<int*>(smem) + WAVES_PER_BLOCK * 2 * TILE_W;
    const int cstrips = (g.cew + STRIP_PX - 1) / STRIP_PX;
    const Task t = decode_task((long)blockIdx.x * WAVES_PER_BLOCK + wave, (long)g.n * g.bhC * cstrips, g.bhC, cstrips);
    const bool active = t.valid && (t.x0 + b * 8 < g.cew);

    int d[2][8] = {};
    if (active) reduced_chroma<VS>(x, t, g, b, r, d);
    stage_qtabs(qtabs, qT, nullptr);                                 // the luma pass reports a clamped entry
    codec_blocks<2>(d, tile, qT, 1, b, r);
    if (active) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lo |= (uint32_t)d[c][j] << (8 * j);
                hi |= (uint32_t)d[c][4 + j] << (8 * j);
            }
            *reinterpret_cast<uint2*>(reduced_plane(planes, g, t.n, c) + (size_t)(t.by * 8 + r) * g.cew + t.x0 + b * 8) = make_uint2(lo, hi);
        }
    }
}

// The up-sampled chroma of the 8 pixels of lane (b, r) from one reduced plane: the 4 samples under them and one to either side, at
// indices clamped to the component's extent (chroma_at's edge rule; whole MCUs, so the extent has at least 8 columns), of the row
// under the pixels and - 4:2:0 - of the nearer neighbour row, clamped likewise.  One 4-byte and two 1-byte loads a row; the
// arithmetic is jpegc.h's fancy_h2v1 / fancy_column / fancy_h2v2.
template <int VS>
__device__ __forceinline__ void upsampled_chroma(const uint8_t* __restrict__ plane, const JpegGeo& g, int py, int px0, int (&out)[8]) {
    const int cc0 = px0 >> 1, left = max(cc0 - 1, 0), right = min(cc0 + 4, g.cew - 1);
    const int j = VS == 2 ? py >> 1 : py;
    int s[VS][6];
#pragma unroll
    for (int k = 0; k < VS; ++k) {
        const int row = k == 0 ? j : ((py & 1) ? min(j + 1, g.ceh - 1) : max(j - 1, 0));
        const uint8_t* base = plane + (size_t)row * g.cew;
        const uint32_t m = *reinterpret_cast<const uint32_t*>(base + cc0);
        s[k][0] = base[left];
        s[k][1] = m & 0xffu; s[k][2] = (m >> 8) & 0xffu; s[k][3] = (m >> 16) & 0xffu; s[k][4] = m >> 24;
        s[k][5] = base[right];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = 1 + (k >> 1), nb = (k & 1) ? i + 1 : i - 1;
        if constexpr (VS == 1) out[k] = fancy_h2v1(s[0][i], s[0][nb], px0 + k);
        else out[k] = fancy_h2v2(fancy_column(s[0][i], s[VS - 1][i]), fancy_column(s[0][nb], s[VS - 1][nb]), px0 + k);
    }
}

template <int VS>
__global__ __launch_bounds__(256) void jpeg_ste_luma_kernel(const float* __restrict__ x, const uint16_t* __restrict__ qtabs,
                                                            const uint8_t* __restrict__ planes, float* __restrict__ y,
                                                            uint8_t* __restrict__ mask, int* __restrict__ err, JpegGeo g) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = lane >> 3, r = lane & 7;
    const int h = g.h, w = g.w;
    float* lds = smem + wave * STAGE_F;
    int* qT = reinterpret_cast<int*>(smem + WAVES_PER_BLOCK * STAGE_F);
    const int hb = h / 8, strips = (w + STRIP_PX - 1) / STRIP_PX;
    const Task t = decode_task((long)blockIdx.x * WAVES_PER_BLOCK + wave, (long)g.n * hb * strips, hb, strips);
    const bool active = t.valid && (t.x0 + b * 8 < w);

    f32x4 pre[6] = {};
    fetch_strip(x, pre, t, h, w, lane);
    int cb[8] = {}, cr[8] = {};
    if (active) {                                                    // reads what the chroma pass left
        upsampled_chroma<VS>(reduced_plane(const_cast<uint8_t*>(planes), g, t.n, 0), g, t.by * 8 + r, t.x0 + b * 8, cb);
        upsampled_chroma<VS>(reduced_plane(const_cast<uint8_t*>(planes), g, t.n, 1), g, t.by * 8 + r, t.x0 + b * 8, cr);
    }
    stage_qtabs(qtabs, qT, err);
    commit_strip(lds, pre, lane);
    wave_sync();
    float px[24];
    read_row24(lds, b, r, px);
    wave_sync();
    int d[1][8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
        d[0][j] = luma_of(byte_of(px[3 * j], false), byte_of(px[3 * j + 1], false), byte_of(px[3 * j + 2], false)) - 128;
    codec_blocks<1>(d, reinterpret_cast<int*>(lds), qT, 0, b, r);
    const uint2 m = finish_row(d[0], cb, cr, px);
    write_row24(lds, b, r, px);
    if (mask && active) *reinterpret_cast<uint2*>(mask + ((long)t.n * h + t.by * 8 + r) * w + t.x0 + b * 8) = m;
    wave_sync();
    store_strip(y, lds, t, h, w, lane);
}

// whole MCUs only, within the limits of nimg_jpeg_transform
inline bool ste_geo(JpegGeo* g, int n, int h, int w, int hs, int vs) {
    return make_geo(g, n, h, w, hs, vs) && h % (8 * vs) == 0 && w % (8 * hs) == 0;
}
inline size_t ste_workspace(const JpegGeo& g) { return g.hs == 1 ? 0 : (size_t)g.n * 2 * g.ceh * g.cew; }

}  // namespace

extern "C" {

size_t nimg_jpeg_ste_workspace_bytes(int n, int h, int w, int hs, int vs) {
    JpegGeo g;
    return ste_geo(&g, n, h, w, hs, vs) ? ste_workspace(g) : 0;
}

int nimg_jpeg_ste_fwd(const float* x, const uint16_t* qtabs, int n, int h, int w, int hs, int vs, float* y, uint8_t* mask, int* err,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (n == 0) return NIMG_OK;        /* empty batch: nothing to do (its buffers may be null) */
    JpegGeo g;
    if (!x || !qtabs || !y || !err || !ste_geo(&g, n, h, w, hs, vs)) return NIMG_ERR_ARG;
    const size_t need = ste_workspace(g);
    if (workspace_bytes < need) return NIMG_ERR_WORKSPACE;
    if (need && !workspace) return NIMG_ERR_ARG;
    const long tasks = (long)n * (h / 8) * ((w + STRIP_PX - 1) / STRIP_PX);
    if (!grid_ok(tasks, WAVES_PER_BLOCK)) return NIMG_ERR_ARG;
    const dim3 grid((unsigned)((tasks + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (hs == 1) {
        hipLaunchKernelGGL(jpeg_ste_444_kernel, grid, block, kLds444, s, x, qtabs, y, mask, err, n, h, w);
        NIMG_CHECK_LAUNCH();
        return NIMG_OK;
    }
    const long ctasks = (long)n * g.bhC * ((g.cew + STRIP_PX - 1) / STRIP_PX);
    const dim3 cgrid((unsigned)((ctasks + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK));
    if (vs == 2) hipLaunchKernelGGL(jpeg_ste_chroma_kernel<2>, cgrid, block, kLdsChroma, s, x, qtabs, (uint8_t*)workspace, g);
    else hipLaunchKernelGGL(jpeg_ste_chroma_kernel<1>, cgrid, block, kLdsChroma, s, x, qtabs, (uint8_t*)workspace, g);
    NIMG_CHECK_LAUNCH();
    if (vs == 2) hipLaunchKernelGGL(jpeg_ste_luma_kernel<2>, grid, block, kLdsLuma, s, x, qtabs, (const uint8_t*)workspace, y, mask, err, g);
    else hipLaunchKernelGGL(jpeg_ste_luma_kernel<1>, grid, block, kLdsLuma, s, x, qtabs, (const uint8_t*)workspace, y, mask, err, g);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

}  // extern "C"
