// The item forms of the baseline JPEG codec: one quality per image instead of one per batch, so that a sweep
// over Q qualities or one round of a per-image quality search is one launch.
//   transform_items    item j = source image j % n_src at quality[j] -> the coefficient layout of nimg_jpeg_transform, n_items images
//   reconstruct_items  item j dequantised with the tables of quality[j]; the colour pass is jpegc.hip's own kernel
// The entropy coder needs no item form: nimg_jpeg_encode takes any coefficient tensor.  The tables of all 100 qualities sit in constant
// memory, built at compile time by make_qtabs - the arithmetic of the single-quality entry points.  The kernels are jpegc.h's, as in
// jpegc.hip, instantiated with the table source below.  tests/test_gpu_ratedist.py holds every item to the bytes of the single-quality
// path.
#include "jpegc.h"

namespace {

struct QBank { QTabs t[100]; };            // entry quality - 1
constexpr QBank make_qbank() {
    QBank b{};
    for (int q = 1; q <= 100; ++q) b.t[q - 1] = make_qtabs(q);
    return b;
}
__constant__ const QBank c_qbank = make_qbank();

// jpegc.h's table source for one quality per item: item j is source image j % n_src with the tables of quality[j].  A quality byte
// outside 1..100 is clamped into the bank, and the thread of the item's first block raises *err
struct ItemTables {
    const uint8_t* quality;
    int* err;
    int n_src = 1;                     // only the transform asks for source(); the inverse DCT leaves it at 1
    __device__ __forceinline__ const uint16_t* table(const JpegGeo& g, long t, int item, int comp) const {
        const int q = quality[item];
        if ((q < 1 || q > 100) && t == (long)item * g.NB) atomicOr(err, 1);
        return c_qbank.t[min(max(q, 1), 100) - 1].q[comp ? 1 : 0];
    }
    __device__ __forceinline__ int source(int item) const { return item % n_src; }
    __device__ __forceinline__ int divisor(const uint16_t* q, int nat) const { return q[nat]; }
};

}  // namespace

extern "C" {

int nimg_jpeg_transform_items(const void* x, int is_u8, int n_src, int h, int w, int hs, int vs, const uint8_t* quality, int n_items,
                              int16_t* coef, int* err, void* workspace, size_t workspace_bytes, void* stream) {
    JpegGeo g, gs;
    if (!x || !coef || !quality || !err || !workspace || !make_geo(&gs, n_src, h, w, hs, vs) || !make_geo(&g, n_items, h, w, hs, vs))
        return NIMG_ERR_ARG;
    const Workspace ws = carve(g, workspace);
    if (workspace_bytes < ws.bytes) return NIMG_ERR_WORKSPACE;
    const long blocks = (long)n_items * g.NB;
    if (!grid_ok(blocks, 256)) return NIMG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)((blocks + 255) / 256);
    const ItemTables tabs{quality, err, n_src};
    if (is_u8) {
        hipLaunchKernelGGL((jpeg_transform_kernel<true, ItemTables>), dim3(grid), dim3(256), 0, st, x, coef, g, tabs, (const uint32_t*)ws.flag);
    } else {
        // one flag per call, as in nimg_jpeg_transform: over the source images, whatever qualities they are coded at
        const int rc = nimg_internal_jpeg_above_one((const float*)x, (long)n_src * h * w * 3, ws.flag, st);
        if (rc != NIMG_OK) return rc;
        hipLaunchKernelGGL((jpeg_transform_kernel<false, ItemTables>), dim3(grid), dim3(256), 0, st, x, coef, g, tabs, (const uint32_t*)ws.flag);
    }
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_jpeg_reconstruct_items(const int16_t* coef, int n_items, int h, int w, int hs, int vs, const uint8_t* quality, float* y, int* err,
                                void* workspace, size_t workspace_bytes, void* stream) {
    JpegGeo g;
    if (!coef || !y || !quality || !err || !workspace || !make_geo(&g, n_items, h, w, hs, vs)) return NIMG_ERR_ARG;
    const Workspace ws = carve(g, workspace);
    if (workspace_bytes < ws.bytes) return NIMG_ERR_WORKSPACE;
    const long blocks = (long)n_items * g.NB;
    if (!grid_ok(blocks, 256)) return NIMG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_idct_kernel<ItemTables>, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, st, coef, ws.planes, g,
                       ItemTables{quality, err});
    NIMG_CHECK_LAUNCH();
    return nimg_internal_jpeg_colour(ws.planes, y, false, g, st);
}

}  // extern "C"
