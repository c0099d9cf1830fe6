// Scaled reconstruction: the coefficients of a batch of files -> the images libjpeg decodes at 1/2, 1/4 or 1/8
// of their size (scale_num / scale_denom), with the tables of each file.
//   idct     one thread per real block of the components that share a block size N: dequantise what the N x N transform uses, the
//            reduced inverse DCT of jpegscale.h (N = 4, 2, 1) or jpegc.h's idct8 (N = 8: the chroma of a 4:2:0 file at 1/2), + 128,
//            clamp -> the component's scaled sample plane.  Luma and chroma of a 4:2:0 file differ in N and take a launch each.
//   colour   one thread per output pixel: the luma sample, the chroma samples - as wide as the output, or for 4:2:2 half as wide and
//            brought up by jpegc.h's h2v1 triangle filter or by replication, as libjpeg chooses at that scale - colour, clamp,
//            the byte or k / 255
// The geometry and the transforms are jpegscale.h, shared with a host program.  Scale 1 is jpegd.hip's launcher behind nimg_jpeg_reconstruct_tables.
#include "jpegc.h"
#include "jpegscale.h"

namespace {

enum { PART_ALL = 0, PART_LUMA = 1, PART_CHROMA = 2 };        // the blocks of an image one launch covers

__device__ __forceinline__ int part_blocks(const JpegGeo& g, int part) {
    return part == PART_ALL ? g.NB : part == PART_LUMA ? g.nbY : 2 * g.nbC;
}

// the coefficients of one block held in registers, two to a word as they lie in memory
struct BlockWords {
    uint32_t w[32];
    __device__ __forceinline__ int operator()(int k) const { return (int)(short)(w[k >> 1] >> (16 * (k & 1))); }
};
// the DC alone, for the 1 x 1 transform
struct BlockDc {
    int dc;
    __device__ __forceinline__ int operator()(int) const { return dc; }
};

template <int N>
__device__ __forceinline__ void store_row(uint8_t* p, const int* v) {
    if constexpr (N == 1) {
        p[0] = (uint8_t)v[0];
    } else if constexpr (N == 2) {
        *reinterpret_cast<uint16_t*>(p) = (uint16_t)(v[0] | v[1] << 8);
    } else {
        const uint32_t lo = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
        if constexpr (N == 4) {
            *reinterpret_cast<uint32_t*>(p) = lo;
        } else {
            const uint32_t hi = (uint32_t)v[4] | (uint32_t)v[5] << 8 | (uint32_t)v[6] << 16 | (uint32_t)v[7] << 24;
            *reinterpret_cast<uint2*>(p) = make_uint2(lo, hi);
        }
    }
}

// one thread per real block of `part`, all of block size N.  A plane begins at a multiple of 16 bytes and its stride and a block's
// first column are multiples of N, so a row of N samples is stored whole.
template <int N, class Tables>
__global__ void __launch_bounds__(256) jpeg_idct_scaled_kernel(const int16_t* __restrict__ coef, uint8_t* __restrict__ planes, JpegGeo g,
                                                               JpegScaleGeo sg, Tables tabs, int part) {
    const long u = (long)blockIdx.x * 256 + threadIdx.x;
    const int count = part_blocks(g, part);
    if (u >= (long)g.n * count) return;
    const long image = u / count;
    const long t = image * g.NB + (u - image * count) + (part == PART_CHROMA ? g.nbY : 0);        // the block in the batch
    int img, comp, br, bc;
    locate(g, t, img, comp, br, bc);
    const uint16_t* q = tabs.table(g, t, img, comp);
    int d[N == 8 ? 64 : N * N];
    if constexpr (N == 1) {
        jpegscale_idct<1>(BlockDc{(int)coef[t * 64]}, q, d);
    } else {
        const uint4* src = reinterpret_cast<const uint4*>(coef + t * 64);
        BlockWords b;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint4 v = src[j];
            b.w[4 * j] = v.x; b.w[4 * j + 1] = v.y; b.w[4 * j + 2] = v.z; b.w[4 * j + 3] = v.w;
        }
        if constexpr (N == 8) {
#pragma unroll
            for (int k = 0; k < 64; ++k) {
                const int nat = c_nat_of_zz[k];
                d[nat] = b(k) * (int)q[nat];
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) idct8<8>(d + c, 11);
#pragma unroll
            for (int r = 0; r < 8; ++r) idct8<1>(d + 8 * r, 18);
#pragma unroll
            for (int k = 0; k < 64; ++k) d[k] = limit_byte(d[k] + 128);
        } else {
            jpegscale_idct<N>(b, q, d);
        }
    }
    const int stride = comp ? sg.strideC : sg.strideY;
    uint8_t* p = planes + jpegscale_plane_offset(sg, img, comp) + (size_t)(N * br) * stride + N * bc;
#pragma unroll
    for (int r = 0; r < N; ++r) store_row<N>(p + (size_t)r * stride, d + N * r);
}

// one thread per output pixel.  ANY: the up-sampler of any sampling (jpegscale_chroma_at, section 4r) in place of the 4:2:2 form - a
// compile-time choice, so that the instantiation of the three samplings of section 4q stays the code it was
template <bool U8, bool ANY = false>
__global__ void __launch_bounds__(256) jpeg_colour_scaled_kernel(const uint8_t* __restrict__ planes, void* __restrict__ out, JpegGeo g,
                                                                 JpegScaleGeo sg) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long area = (long)sg.oh * sg.ow;
    if (t >= (long)g.n * area) return;
    const int img = (int)(t / area), r = (int)(t - (long)img * area), y = r / sg.ow, x = r - y * sg.ow;
    const int yy = planes[jpegscale_plane_offset(sg, img, 0) + (size_t)y * sg.strideY + x];
    if (g.nc == 1) {                                     // grey-scale: the range-limited sample is the pixel
        if (U8) ((uint8_t*)out)[t] = (uint8_t)yy;
        else ((float*)out)[t] = __fdiv_rn((float)yy, 255.0f);
        return;
    }
    const uint8_t* pb = planes + jpegscale_plane_offset(sg, img, 1) + (size_t)y * sg.strideC;
    const uint8_t* pr = pb + sg.planeC;
    int cb, cr;
    if (ANY) {
        const uint8_t* plane = planes + jpegscale_plane_offset(sg, img, 1);
        cb = jpegscale_chroma_at(plane, sg, y, x); cr = jpegscale_chroma_at(plane + sg.planeC, sg, y, x);
    } else if (sg.up == JPEGSCALE_UP_NONE) {
        cb = pb[x]; cr = pr[x];
    } else {
        int near, nb;
        jpegscale_chroma_columns(sg, x, near, nb);
        if (sg.up == JPEGSCALE_UP_FANCY) {
            cb = fancy_h2v1(pb[near], pb[nb], x); cr = fancy_h2v1(pr[near], pr[nb], x);
        } else {
            cb = pb[near]; cr = pr[near];
        }
    }
    cb -= 128; cr -= 128;
    const int R = limit_byte(red_of(yy, cr)), G = limit_byte(green_of(yy, cb, cr)), B = limit_byte(blue_of(yy, cb));
    if (U8) {
        uint8_t* o = (uint8_t*)out + t * 3;
        o[0] = (uint8_t)R; o[1] = (uint8_t)G; o[2] = (uint8_t)B;
    } else {
        float* o = (float*)out + t * 3;
        o[0] = __fdiv_rn((float)R, 255.0f);
        o[1] = __fdiv_rn((float)G, 255.0f);
        o[2] = __fdiv_rn((float)B, 255.0f);
    }
}

template <int N>
void launch_idct(const int16_t* coef, uint8_t* planes, const JpegGeo& g, const JpegScaleGeo& sg, const uint16_t* qtabs, int part,
                 hipStream_t st) {
    const long blocks = (long)g.n * (part == PART_ALL ? g.NB : part == PART_LUMA ? g.nbY : 2 * g.nbC);
    hipLaunchKernelGGL((jpeg_idct_scaled_kernel<N, FileTables>), dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, st, coef, planes, g, sg,
                       FileTables{qtabs}, part);
}

// the launch of the blocks of `part`, whose block size is N = 1, 2, 4 or 8
void launch_idct_of(int N, const int16_t* coef, uint8_t* planes, const JpegGeo& g, const JpegScaleGeo& sg, const uint16_t* qtabs, int part,
                    hipStream_t st) {
    if (N == 1) launch_idct<1>(coef, planes, g, sg, qtabs, part, st);
    else if (N == 2) launch_idct<2>(coef, planes, g, sg, qtabs, part, st);
    else if (N == 4) launch_idct<4>(coef, planes, g, sg, qtabs, part, st);
    else launch_idct<8>(coef, planes, g, sg, qtabs, part, st);
}

size_t scaled_workspace_size(int n, int h, int w, int hs, int vs, int nc, int scale, int factors = JPEG_FACTORS_THREE) {
    JpegGeo g;
    JpegScaleGeo sg;
    if (!jpegscale_ok(scale) || !make_geo(&g, n, h, w, hs, vs, nc, factors)) return 0;
    if (scale == 1) return carve(g, nullptr).bytes;        // what nimg_jpeg_workspace_bytes counts
    return make_scale_geo(&sg, g, scale) ? align256((size_t)n * sg.per) : 0;
}

int reconstruct_scaled_launch(const int16_t* coef, int n, int h, int w, int hs, int vs, int nc, const uint16_t* qtabs, int scale, void* y,
                              int out_u8, void* workspace, size_t workspace_bytes, void* stream, int factors = JPEG_FACTORS_THREE) {
    JpegGeo g;
    JpegScaleGeo sg;
    if (!coef || !y || !qtabs || !workspace || !jpegscale_ok(scale) || !make_geo(&g, n, h, w, hs, vs, nc, factors)) return NIMG_ERR_ARG;
    if (scale == 1)
        return nimg_internal_jpeg_reconstruct_tables(coef, n, h, w, hs, vs, nc, qtabs, y, out_u8, workspace, workspace_bytes, stream, factors);
    if (!make_scale_geo(&sg, g, scale)) return NIMG_ERR_ARG;
    if (workspace_bytes < align256((size_t)n * sg.per)) return NIMG_ERR_WORKSPACE;
    const long blocks = (long)n * g.NB, pixels = (long)n * sg.oh * sg.ow;
    if (!grid_ok(blocks, 256) || !grid_ok(pixels, 256)) return NIMG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* planes = (uint8_t*)workspace;
    if (nc == 1 || sg.nC == sg.nY) {
        launch_idct_of(sg.nY, coef, planes, g, sg, qtabs, PART_ALL, st);
        NIMG_CHECK_LAUNCH();
    } else {
        launch_idct_of(sg.nY, coef, planes, g, sg, qtabs, PART_LUMA, st);
        NIMG_CHECK_LAUNCH();
        launch_idct_of(sg.nC, coef, planes, g, sg, qtabs, PART_CHROMA, st);
        NIMG_CHECK_LAUNCH();
    }
    const dim3 grid((unsigned)((pixels + 255) / 256));
    if (nc == 3 && !jpeg_factors_ok(hs, vs, JPEG_FACTORS_THREE)) {        // the samplings of section 4r
        if (out_u8) hipLaunchKernelGGL((jpeg_colour_scaled_kernel<true, true>), grid, dim3(256), 0, st, (const uint8_t*)planes, y, g, sg);
        else hipLaunchKernelGGL((jpeg_colour_scaled_kernel<false, true>), grid, dim3(256), 0, st, (const uint8_t*)planes, y, g, sg);
    } else if (out_u8) hipLaunchKernelGGL(jpeg_colour_scaled_kernel<true>, grid, dim3(256), 0, st, (const uint8_t*)planes, y, g, sg);
    else hipLaunchKernelGGL(jpeg_colour_scaled_kernel<false>, grid, dim3(256), 0, st, (const uint8_t*)planes, y, g, sg);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

}  // namespace

extern "C" {

size_t nimg_jpeg_reconstruct_scaled_workspace_bytes(int n, int h, int w, int hs, int vs, int scale) {
    return scaled_workspace_size(n, h, w, hs, vs, 3, scale);
}

int nimg_jpeg_reconstruct_scaled(const int16_t* coef, int n, int h, int w, int hs, int vs, const uint16_t* qtabs, int scale, void* y,
                                 int out_u8, void* workspace, size_t workspace_bytes, void* stream) {
    return reconstruct_scaled_launch(coef, n, h, w, hs, vs, 3, qtabs, scale, y, out_u8, workspace, workspace_bytes, stream);
}

// the same launcher with the wide set of sampling factors; scale 1 is nimg_jpeg_sampling_reconstruct_tables
size_t nimg_jpeg_sampling_reconstruct_scaled_workspace_bytes(int n, int h, int w, int hs, int vs, int scale) {
    return scaled_workspace_size(n, h, w, hs, vs, 3, scale, JPEG_FACTORS_WIDE);
}

int nimg_jpeg_sampling_reconstruct_scaled(const int16_t* coef, int n, int h, int w, int hs, int vs, const uint16_t* qtabs, int scale, void* y,
                                          int out_u8, void* workspace, size_t workspace_bytes, void* stream) {
    return reconstruct_scaled_launch(coef, n, h, w, hs, vs, 3, qtabs, scale, y, out_u8, workspace, workspace_bytes, stream,
                                     JPEG_FACTORS_WIDE);
}

size_t nimg_jpeg_reconstruct_scaled_grey_workspace_bytes(int n, int h, int w, int scale) {
    return scaled_workspace_size(n, h, w, 1, 1, 1, scale);
}

int nimg_jpeg_reconstruct_scaled_grey(const int16_t* coef, int n, int h, int w, const uint16_t* qtabs, int scale, void* y, int out_u8,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    if (n == 0) return jpegscale_ok(scale) ? NIMG_OK : NIMG_ERR_ARG;
    return reconstruct_scaled_launch(coef, n, h, w, 1, 1, 1, qtabs, scale, y, out_u8, workspace, workspace_bytes, stream);
}

}  // extern "C"
