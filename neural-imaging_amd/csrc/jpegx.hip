// Lossless transforms: the coefficients of a batch of files of one geometry -> the coefficients of the files
// jpegtran makes of them by a flip, a transposition, a rotation or an aligned crop - a permutation of the blocks and of the 64
// coefficients of a block, with sign changes.  Pure data movement: a block is 128 bytes, one cache line, read once and written once.
//   lossless   eight lanes per output block, all components in one launch: the lanes find the block's source (jpegxform.h, shared with
//              a host program), load its 128 bytes as eight contiguous 16-byte pieces and store the output block the same way.  A
//              mirroring negates the coefficients of odd u or v in the words the lane already holds; a transposition moves the 64
//              coefficients between the eight lanes through LDS - 128 bytes per block, never through global memory.
// No atomics, no workspace, no switch.
#include "common.h"
#include "jpegxform.h"

namespace {

constexpr int XF_THREADS = 256, XF_LANES = 8, XF_BLOCKS = XF_THREADS / XF_LANES;        // 32 blocks, 4 KiB, per workgroup

// the source positions of the eight coefficients lane j writes of a transposed block (jpegxform_transposed_octet): compile-time
// constants behind a select, no table in memory
__device__ __forceinline__ uint64_t transposed_octet_of(int j) {
    constexpr uint64_t o0 = jpegxform_transposed_octet(0), o1 = jpegxform_transposed_octet(1), o2 = jpegxform_transposed_octet(2),
                       o3 = jpegxform_transposed_octet(3), o4 = jpegxform_transposed_octet(4), o5 = jpegxform_transposed_octet(5),
                       o6 = jpegxform_transposed_octet(6), o7 = jpegxform_transposed_octet(7);
    return j == 0 ? o0 : j == 1 ? o1 : j == 2 ? o2 : j == 3 ? o3 : j == 4 ? o4 : j == 5 ? o5 : j == 6 ? o6 : o7;
}

// two coefficients in a word, each negated (two's complement on its 16 bits) where its bit of `neg` is set
__device__ __forceinline__ uint32_t negate_pair(uint32_t v, unsigned neg) {
    const uint32_t lo = (neg & 1) ? (0u - v) & 0xffffu : v & 0xffffu;
    const uint32_t hi = (neg & 2) ? (0u - (v >> 16)) << 16 : v & 0xffff0000u;
    return lo | hi;
}

// FLAGS: jpegxform_flags of the operation.  Thread t serves piece t % 8 of output block t / 8 of the batch.
template <int FLAGS>
__global__ void __launch_bounds__(XF_THREADS) jpeg_lossless_kernel(const int16_t* __restrict__ coef, int16_t* __restrict__ out, JpegXform x,
                                                                   long blocks) {
    constexpr uint64_t NEG = jpegxform_negated(FLAGS);
    const long b = (long)blockIdx.x * XF_BLOCKS + threadIdx.x / XF_LANES;
    const int j = threadIdx.x % XF_LANES;
    const bool live = b < blocks;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (live) {
        const long img = b / x.NB;
        int comp, r, c;
        jpegxform_locate(x, (int)(b - img * x.NB), comp, r, c);
        const long src = img * x.sNB + jpegxform_source_block(x, comp, r, c);
        v = reinterpret_cast<const uint4*>(coef + src * 64)[j];
    }
    if constexpr (FLAGS & JPEGXFORM_T) {
        __shared__ uint4 tile[XF_THREADS];
        tile[threadIdx.x] = v;
        __syncthreads();
        const uint16_t* blk = reinterpret_cast<const uint16_t*>(tile + (threadIdx.x - j));        // the 64 coefficients of this block
        const uint64_t from = transposed_octet_of(j);
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t lo = blk[(from >> (16 * i)) & 63], hi = blk[(from >> (16 * i + 8)) & 63];
            w[i] = lo | hi << 16;
        }
        v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if constexpr (NEG != 0) {
        const unsigned neg = (unsigned)(NEG >> (8 * j)) & 0xffu;                                  // the eight positions this lane holds
        v.x = negate_pair(v.x, neg); v.y = negate_pair(v.y, neg >> 2); v.z = negate_pair(v.z, neg >> 4); v.w = negate_pair(v.w, neg >> 6);
    }
    if (live) reinterpret_cast<uint4*>(out + b * 64)[j] = v;
}

template <int FLAGS>
void launch(const int16_t* coef, int16_t* out, const JpegXform& x, long blocks, hipStream_t st) {
    hipLaunchKernelGGL(jpeg_lossless_kernel<FLAGS>, dim3((unsigned)((blocks + XF_BLOCKS - 1) / XF_BLOCKS)), dim3(XF_THREADS), 0, st, coef, out,
                       x, blocks);
}

int geometry(JpegXform* x, int h, int w, int hs, int vs, int nc, int op, int crop_x, int crop_y, int crop_w, int crop_h, int trim) {
    return jpegxform_make(x, h, w, hs, vs, nc, op, crop_x, crop_y, crop_w, crop_h, trim) == JPEGXFORM_OK ? NIMG_OK : NIMG_ERR_ARG;
}

}  // namespace

extern "C" {

int nimg_jpeg_lossless_geometry(int h, int w, int hs, int vs, int nc, int op, int crop_x, int crop_y, int crop_w, int crop_h, int trim,
                                int* out_h, int* out_w, int* out_hs, int* out_vs) {
    JpegXform x;
    if (!out_h || !out_w || !out_hs || !out_vs || geometry(&x, h, w, hs, vs, nc, op, crop_x, crop_y, crop_w, crop_h, trim) != NIMG_OK)
        return NIMG_ERR_ARG;
    *out_h = x.h; *out_w = x.w; *out_hs = x.hs; *out_vs = x.vs;
    return NIMG_OK;
}

int nimg_jpeg_lossless(const int16_t* coef, int n, int h, int w, int hs, int vs, int nc, int op, int crop_x, int crop_y, int crop_w,
                       int crop_h, int trim, int16_t* out, int* out_h, int* out_w, int* out_hs, int* out_vs, void* stream) {
    JpegXform x;
    if (geometry(&x, h, w, hs, vs, nc, op, crop_x, crop_y, crop_w, crop_h, trim) != NIMG_OK) return NIMG_ERR_ARG;
    if (nc == 1 && n == 0) return NIMG_OK;                          // a grey-scale batch of no images, as the nimg_jpeg_grey_* entries take it
    if (!coef || !out || !out_h || !out_w || !out_hs || !out_vs || n < 1 || n > 65535) return NIMG_ERR_ARG;
    const long blocks = (long)n * x.NB;
    if ((blocks + XF_BLOCKS - 1) / XF_BLOCKS > 0x7fffffffL) return NIMG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    switch (x.flags) {
        case 0: launch<0>(coef, out, x, blocks, st); break;
        case 1: launch<1>(coef, out, x, blocks, st); break;
        case 2: launch<2>(coef, out, x, blocks, st); break;
        case 3: launch<3>(coef, out, x, blocks, st); break;
        case 4: launch<4>(coef, out, x, blocks, st); break;
        case 5: launch<5>(coef, out, x, blocks, st); break;
        case 6: launch<6>(coef, out, x, blocks, st); break;
        default: launch<7>(coef, out, x, blocks, st); break;
    }
    NIMG_CHECK_LAUNCH();
    *out_h = x.h; *out_w = x.w; *out_hs = x.hs; *out_vs = x.vs;
    return NIMG_OK;
}

}  // extern "C"
