// The item forms of the baseline JPEG codec: one quality per image instead of one per batch, so that a sweep
// over Q qualities or one round of a per-image quality search is one launch.
//   transform_items    item j = source image j % n_src at quality[j] -> the coefficient layout of nimg_jpeg_transform, n_items images
//   reconstruct_items  item j dequantised with the tables of quality[j]; the colour pass is jpegc.hip's own kernel
// The entropy coder needs no item form: nimg_jpeg_encode takes any coefficient tensor.  The tables of all 100 qualities sit in constant
// memory, built at compile time by make_qtabs - the arithmetic of the single-quality entry points.  Sampling, the DCTs and the block
// order are jpegc.h's device functions, shared with jpegc.hip; the two kernels there keep their own few lines around them, because
// folding those into one function with these changed their code objects (tools/codeobj_diff.py: 96 -> 183 VGPRs for the transform).
// tests/test_gpu_ratedist.py holds every item to the bytes of the single-quality path.
#include "jpegc.h"

namespace {

struct QBank { QTabs t[100]; };            // entry quality - 1
constexpr QBank make_qbank() {
    QBank b{};
    for (int q = 1; q <= 100; ++q) b.t[q - 1] = make_qtabs(q);
    return b;
}
__constant__ const QBank c_qbank = make_qbank();

// the tables of item `item`; a quality byte outside 1..100 is clamped into the bank, and the thread with `report` raises *err
__device__ __forceinline__ const QTabs& item_tables(const uint8_t* __restrict__ quality, int item, bool report, int* err) {
    const int q = quality[item];
    if ((q < 1 || q > 100) && report) atomicOr(err, 1);
    return c_qbank.t[min(max(q, 1), 100) - 1];
}

// one thread per real block of an item (jpeg_transform_kernel with the source image and the tables looked up per item)
template <bool U8>
__global__ void __launch_bounds__(256) jpeg_transform_items_kernel(const void* __restrict__ x, int16_t* __restrict__ coef, Geo g, int n_src,
                                                                   const uint8_t* __restrict__ quality,
                                                                   const uint32_t* __restrict__ flag, int* __restrict__ err) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)g.n * g.NB) return;
    int item, comp, br, bc;
    locate(g, t, item, comp, br, bc);
    const bool div = !U8 && *flag != 0;
    const int img = item % n_src;
    const void* base = U8 ? (const void*)((const uint8_t*)x + (long)img * g.h * g.w * 3)
                          : (const void*)((const float*)x + (long)img * g.h * g.w * 3);
    const uint16_t* q = item_tables(quality, item, t == (long)item * g.NB, err).q[comp ? 1 : 0];
    int d[64];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) d[8 * r + c] = sample<U8>(base, g, comp, 8 * br + r, 8 * bc + c, div) - 128;
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct8<1, true>(d + 8 * r);
#pragma unroll
    for (int c = 0; c < 8; ++c) fdct8<8, false>(d + c);
    uint32_t o[32];
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int nat = c_nat_of_zz[k];
        const int v = d[nat], qv = (int)q[nat] << 3;
        const int m = (int)(((unsigned)abs(v) + (unsigned)(qv >> 1)) / (unsigned)qv);
        const uint32_t c16 = (uint32_t)(v < 0 ? -m : m) & 0xffffu;
        if (k & 1) o[k >> 1] |= c16 << 16;
        else o[k >> 1] = c16;
    }
    uint4* dst = reinterpret_cast<uint4*>(coef + t * 64);
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[j] = make_uint4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
}

// one thread per real block of an item (jpeg_idct_kernel with the tables looked up per item)
__global__ void __launch_bounds__(256) jpeg_idct_items_kernel(const int16_t* __restrict__ coef, uint8_t* __restrict__ planes, Geo g,
                                                              const uint8_t* __restrict__ quality, int* __restrict__ err) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)g.n * g.NB) return;
    int item, comp, br, bc;
    locate(g, t, item, comp, br, bc);
    const uint16_t* q = item_tables(quality, item, t == (long)item * g.NB, err).q[comp ? 1 : 0];
    const uint4* src = reinterpret_cast<const uint4*>(coef + t * 64);
    uint32_t wds[32];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint4 v = src[j];
        wds[4 * j] = v.x; wds[4 * j + 1] = v.y; wds[4 * j + 2] = v.z; wds[4 * j + 3] = v.w;
    }
    int d[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int nat = c_nat_of_zz[k];
        d[nat] = (int)(short)(wds[k >> 1] >> (16 * (k & 1))) * (int)q[nat];
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) idct8<8>(d + c, 11);
#pragma unroll
    for (int r = 0; r < 8; ++r) idct8<1>(d + 8 * r, 18);
    const int stride = 8 * (comp ? g.bwC : g.bwY);
    uint8_t* p = plane_of(planes, g, item, comp) + (size_t)(8 * br) * stride + 8 * bc;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            lo |= (uint32_t)min(max(d[8 * r + c] + 128, 0), 255) << (8 * c);
            hi |= (uint32_t)min(max(d[8 * r + 4 + c] + 128, 0), 255) << (8 * c);
        }
        *reinterpret_cast<uint2*>(p + (size_t)r * stride) = make_uint2(lo, hi);
    }
}

}  // namespace

extern "C" {

int nimg_jpeg_transform_items(const void* x, int is_u8, int n_src, int h, int w, int hs, int vs, const uint8_t* quality, int n_items,
                              int16_t* coef, int* err, void* workspace, size_t workspace_bytes, void* stream) {
    Geo g, gs;
    if (!x || !coef || !quality || !err || !workspace || !make_geo(&gs, n_src, h, w, hs, vs) || !make_geo(&g, n_items, h, w, hs, vs))
        return NIMG_ERR_ARG;
    const Workspace ws = carve(g, workspace);
    if (workspace_bytes < ws.bytes) return NIMG_ERR_WORKSPACE;
    const long blocks = (long)n_items * g.NB;
    if (!grid_ok(blocks, 256)) return NIMG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)((blocks + 255) / 256);
    if (is_u8) {
        hipLaunchKernelGGL(jpeg_transform_items_kernel<true>, dim3(grid), dim3(256), 0, st, x, coef, g, n_src, quality,
                           (const uint32_t*)ws.flag, err);
    } else {
        // one flag per call, as in nimg_jpeg_transform: over the source images, whatever qualities they are coded at
        const int rc = nimg_internal_jpeg_above_one((const float*)x, (long)n_src * h * w * 3, ws.flag, st);
        if (rc != NIMG_OK) return rc;
        hipLaunchKernelGGL(jpeg_transform_items_kernel<false>, dim3(grid), dim3(256), 0, st, x, coef, g, n_src, quality,
                           (const uint32_t*)ws.flag, err);
    }
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_jpeg_reconstruct_items(const int16_t* coef, int n_items, int h, int w, int hs, int vs, const uint8_t* quality, float* y, int* err,
                                void* workspace, size_t workspace_bytes, void* stream) {
    Geo g;
    if (!coef || !y || !quality || !err || !workspace || !make_geo(&g, n_items, h, w, hs, vs)) return NIMG_ERR_ARG;
    const Workspace ws = carve(g, workspace);
    if (workspace_bytes < ws.bytes) return NIMG_ERR_WORKSPACE;
    const long blocks = (long)n_items * g.NB;
    if (!grid_ok(blocks, 256)) return NIMG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_idct_items_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, st, coef, ws.planes, g, quality, err);
    NIMG_CHECK_LAUNCH();
    return nimg_internal_jpeg_colour(ws.planes, y, n_items, h, w, hs, vs, st);
}

}  // extern "C"
