// MS-SSIM as a metric: tf.image.ssim_multiscale per image, for the msssim / msssim_db columns of the
// rate-distortion tables.  The five scales are the entry points the MS-SSIM loss is built from - nimg_ssim_planes (losses.hip) on
// each, nimg_avgpool_fwd (manip.hip) between them - followed by the per-image combination below.  Every sum on the way has one fixed
// order and stays inside one image (nimg_ssim_planes reduces per (image, channel) plane), so an image's value is the same alone and
// in any batch.
#include "common.h"

namespace {

constexpr int WIN = 11;                    // the Gaussian window of nimg_ssim_planes
constexpr int SCALES = 5;

// out[i] = mean_c prod_k relu(v[k][i][c]) ^ w[k], the weights and the arithmetic of msssim_combine_kernel (losses.hip); one thread
// per image, its channels added in order.  The result stays a double: the tables need 1 - value, and a float32 next to 1 would
// leave 255 (1 - value) with an error of 7.6e-6, more than the whole bound the MS-SSIM loss is held to
__global__ __launch_bounds__(64) void msssim_images_kernel(const float* __restrict__ v, int n, int c, double* __restrict__ out) {
    const float wts[SCALES] = {0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f};
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int planes = n * c;
    double acc = 0.0;
    for (int ch = 0; ch < c; ++ch) {
        double ms = 1.0;
        for (int k = 0; k < SCALES; ++k) ms *= pow((double)fmaxf(v[k * planes + i * c + ch], 0.f), (double)wts[k]);
        acc += ms;
    }
    out[i] = acc / c;
}

using nimg::align256;

inline bool size_ok(int n, int h, int w, int c) {
    const int div = 1 << (SCALES - 1);
    return n > 0 && c > 0 && h > 0 && w > 0 && h % div == 0 && w % div == 0 && h / div >= WIN && w / div >= WIN &&
           (long)n * c * SCALES <= 0x7fffffffL && (long)n * h * w * c <= 0x7fffffffL;
}

}  // namespace

extern "C" {

size_t nimg_msssim_workspace_bytes(int n, int h, int w, int c) {
    if (!size_ok(n, h, w, c)) return 0;
    size_t bytes = align256((size_t)SCALES * n * c * sizeof(float)) + align256(nimg_ssim_planes_workspace_bytes(n, c));
    for (int k = 1; k < SCALES; ++k) bytes += 2 * align256((size_t)n * (h >> k) * (w >> k) * c * sizeof(float));
    return bytes;
}

int nimg_msssim(const float* a, const float* b, int n, int h, int w, int c, float max_val, const float* gauss_win, double* out,
                void* workspace, size_t workspace_bytes, void* stream) {
    if (!a || !b || !gauss_win || !out || !workspace || !size_ok(n, h, w, c) || !(max_val > 0.f)) return NIMG_ERR_ARG;
    if (workspace_bytes < nimg_msssim_workspace_bytes(n, h, w, c)) return NIMG_ERR_WORKSPACE;
    uint8_t* p = (uint8_t*)workspace;
    float* values = (float*)p; p += align256((size_t)SCALES * n * c * sizeof(float));
    void* planes_ws = p; p += align256(nimg_ssim_planes_workspace_bytes(n, c));
    const float *ak = a, *bk = b;
    for (int k = 0; k < SCALES; ++k) {
        const int hk = h >> k, wk = w >> k;
        if (k > 0) {                                           // scale k = the 2x2 average of scale k - 1
            const size_t level = align256((size_t)n * hk * wk * c * sizeof(float));
            float* an = (float*)p; p += level;
            float* bn = (float*)p; p += level;
            int rc = nimg_avgpool_fwd(ak, an, n, 2 * hk, 2 * wk, c, 2, stream);
            if (rc == NIMG_OK) rc = nimg_avgpool_fwd(bk, bn, n, 2 * hk, 2 * wk, c, 2, stream);
            if (rc != NIMG_OK) return rc;
            ak = an; bk = bn;
        }
        const bool last = k == SCALES - 1;                     // contrast-structure means of scales 0..3, the SSIM mean of scale 4
        float* vk = values + (size_t)k * n * c;
        const int rc = nimg_ssim_planes(ak, bk, n, hk, wk, c, max_val, gauss_win, last ? vk : nullptr, last ? nullptr : vk, nullptr, 0,
                                        planes_ws, nimg_ssim_planes_workspace_bytes(n, c), stream);
        if (rc != NIMG_OK) return rc;
    }
    hipLaunchKernelGGL(msssim_images_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const float*)values, n, c, out);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

}  // extern "C"
