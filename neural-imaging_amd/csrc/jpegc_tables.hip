// The table forms of the baseline JPEG writer: the quantisation tables are an input - device memory, one set of
// three per item - instead of a quality the tables are built from, so that a file can be written with any 8-bit tables: the learned
// ones of JPEG(trainable=True), the reference's jpeg_qtable, those of a foreign file.
//   transform_tables    item j = source image j % n_src divided by qtabs[j][component] -> the coefficient layout of nimg_jpeg_transform
//   tables_from_float   float32 tables -> the uint16 layout above by jpeg_qrule.h's rule, with what it had to do per set
// The way back needs nothing new: nimg_jpeg_reconstruct_tables (jpegd.hip) takes this layout, nimg_jpeg_encode any coefficient tensor.
// The transform is jpegc.h's kernel, as in jpegc.hip and jpegc_items.hip, instantiated with the table source below.  Each thread reads
// the 64 divisors of its block from global memory: the addresses are compile-time offsets from one base that all threads of an item
// and component share, so a wave's loads are wide, mostly one cache line broadcast to its lanes, and hit L2 after the item's first
// wave; a staging of the tables through LDS would add a barrier to a kernel that has none and whose workgroups straddle items.
// tests/test_gpu_jpegq.py holds it to the bytes of the quality path and of libjpeg.
#include "jpeg_qrule.h"
#include "jpegc.h"

namespace {

// jpegc.h's table source for the caller's tables: qtabs[item][component][64], natural order, in global memory.  An entry outside
// 1..255 is clamped where it is used, so no thread divides by zero, and the thread of the item's first block, which looks at all
// entries of the item - 192, or the 64 of a grey-scale file's one table (NC = 1) -, raises *err.
template <int NC>
struct DeviceTables {
    const uint16_t* qtabs;
    int* err;
    int n_src;
    __device__ __forceinline__ const uint16_t* table(const JpegGeo& g, long t, int item, int comp) const {
        constexpr int entries = 64 * NC;
        const uint16_t* q = qtabs + (size_t)item * entries;
        if (t == (long)item * g.NB) {
            bool bad = false;
            for (int k = 0; k < entries; ++k) bad |= q[k] < 1 || q[k] > 255;
            if (bad) atomicOr(err, 1);
        }
        return q + comp * 64;
    }
    __device__ __forceinline__ int source(int item) const { return item % n_src; }
    __device__ __forceinline__ int divisor(const uint16_t* q, int nat) const { return min(max((int)q[nat], 1), 255); }
};

// one thread per entry of the output: set s, component c, entry k <- t[s][min(c, n_tabs - 1)][k]
__global__ void __launch_bounds__(256) jpeg_tables_from_float_kernel(const float* __restrict__ t, int n_sets, int n_tabs,
                                                                     uint16_t* __restrict__ qtabs, uint32_t* __restrict__ status) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n_sets * 192) return;
    const int s = (int)(i / 192), c = (int)(i % 192) / 64, k = (int)(i & 63);
    uint32_t st = 0;
    qtabs[i] = jpegq_entry(t[((size_t)s * n_tabs + min(c, n_tabs - 1)) * 64 + k], &st);
    if (st) atomicOr(status + s, st);
}

// the launcher of the transform with the caller's tables, for three components (nc = 3) and for one (nc = 1, section 4p)
int transform_tables_launch(const void* x, int is_u8, int n_src, int h, int w, int hs, int vs, int nc, const uint16_t* qtabs, int n_items,
                            int16_t* coef, int* err, void* workspace, size_t workspace_bytes, void* stream) {
    JpegGeo g, gs;
    if (!x || !coef || !qtabs || !err || !workspace || !make_geo(&gs, n_src, h, w, hs, vs, nc) || !make_geo(&g, n_items, h, w, hs, vs, nc))
        return NIMG_ERR_ARG;
    const Workspace ws = carve(g, workspace);
    if (workspace_bytes < ws.bytes) return NIMG_ERR_WORKSPACE;
    const long blocks = (long)n_items * g.NB;
    if (!grid_ok(blocks, 256)) return NIMG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)((blocks + 255) / 256);
    const uint32_t* flag = ws.flag;
    if (!is_u8) {
        // one flag per call, as in nimg_jpeg_transform: over the source images, whatever tables they are coded with
        const int rc = nimg_internal_jpeg_above_one((const float*)x, (long)n_src * h * w * nc, ws.flag, st);
        if (rc != NIMG_OK) return rc;
    }
    if (nc == 1) {
        const DeviceTables<1> tabs{qtabs, err, n_src};
        if (is_u8) hipLaunchKernelGGL((jpeg_transform_kernel<true, DeviceTables<1>, true>), dim3(grid), dim3(256), 0, st, x, coef, g, tabs, flag);
        else hipLaunchKernelGGL((jpeg_transform_kernel<false, DeviceTables<1>, true>), dim3(grid), dim3(256), 0, st, x, coef, g, tabs, flag);
    } else {
        const DeviceTables<3> tabs{qtabs, err, n_src};
        if (is_u8) hipLaunchKernelGGL((jpeg_transform_kernel<true, DeviceTables<3>>), dim3(grid), dim3(256), 0, st, x, coef, g, tabs, flag);
        else hipLaunchKernelGGL((jpeg_transform_kernel<false, DeviceTables<3>>), dim3(grid), dim3(256), 0, st, x, coef, g, tabs, flag);
    }
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

}  // namespace

extern "C" {

int nimg_jpeg_transform_tables(const void* x, int is_u8, int n_src, int h, int w, int hs, int vs, const uint16_t* qtabs, int n_items,
                               int16_t* coef, int* err, void* workspace, size_t workspace_bytes, void* stream) {
    return transform_tables_launch(x, is_u8, n_src, h, w, hs, vs, 3, qtabs, n_items, coef, err, workspace, workspace_bytes, stream);
}

int nimg_jpeg_grey_transform_tables(const void* x, int is_u8, int n_src, int h, int w, const uint16_t* qtabs, int n_items, int16_t* coef,
                                    int* err, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_src == 0 && n_items == 0) return NIMG_OK;
    return transform_tables_launch(x, is_u8, n_src, h, w, 1, 1, 1, qtabs, n_items, coef, err, workspace, workspace_bytes, stream);
}

int nimg_jpeg_tables_from_float(const float* t, int n_sets, int n_tabs, uint16_t* qtabs, uint32_t* status, void* stream) {
    if (!t || !qtabs || !status || n_sets < 1 || n_sets > 65535 || (n_tabs != 2 && n_tabs != 3)) return NIMG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, (size_t)n_sets * 4, st) != hipSuccess) return NIMG_ERR_LAUNCH;
    hipLaunchKernelGGL(jpeg_tables_from_float_kernel, dim3((unsigned)(((long)n_sets * 192 + 255) / 256)), dim3(256), 0, st, t, n_sets,
                       n_tabs, qtabs, status);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

}  // extern "C"
