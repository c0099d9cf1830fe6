// Baseline JPEG codec: the files libjpeg writes with default settings - one interleaved scan, Annex K
// Huffman tables, no restart markers - and the images it decodes from them, as integer kernels over a whole batch per launch.
//   transform    RGB (float32 | uint8, NHWC) -> quantised coefficients, int16 [image][component][block row][block col][64 zig-zag],
//                real blocks only (colour, edge replication, chroma down-sampling, jfdctint forward DCT, quantisation)
//   encode       coefficients -> the entropy-coded segments of all images back to back + lengths[n]:
//                  bit length of every block in scan order (dummy blocks included) | exclusive scan per image | zero the words
//                  that will be OR-ed into | every block places its bits at its offset (last block: the 1-padding) |
//                  count the FF bytes per image | scan the segment lengths | scatter the bytes with their 00 stuffing
//                with a restart interval (nimg_jpeg_encode_restart, section 4i) the same passes: the predictors restart in the
//                block walk, the scan rounds an interval's end up to a byte and leaves 16 bits free, the emitter of the interval's
//                last block pads, and the scatter writes FF D0 .. D7 where those 16 bits stand
//   reconstruct  coefficients -> float32 NHWC (dequantise, jidctint inverse DCT, fancy chroma up-sampling, colour, k / 255)
// Nothing here loops over images or blocks on the host, and nothing is read back: the caller synchronises once for `lengths`.
// The transform and inverse-DCT kernels and the bit sink are jpegc.h's, instantiated here for one quality per batch; the scan-order
// block walk is csrc/jpegopt.h's, the one tests/jpegopt_host.cpp runs on the host.
#include "jpegc.h"
#include "jpegopt.h"

namespace {

// Annex K: codes per length 1..16 and the symbols in code order (as in the DHT segments of every file)
constexpr int DC_LUMA_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr int DC_CHROMA_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr int AC_LUMA_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
constexpr int AC_CHROMA_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
constexpr char DC_VALS[] = "000102030405060708090a0b";
constexpr char AC_LUMA_VALS[] =
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738"
    "393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5"
    "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa";
constexpr char AC_CHROMA_VALS[] =
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3"
    "a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa";

struct HuffTabs {
    uint32_t dc[2][16];        // [luma | chroma][category]: code << 5 | length
    uint32_t ac[2][256];       // [luma | chroma][run << 4 | category]
};
constexpr int hexv(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }
constexpr void fill_codes(uint32_t* tab, const int* bits, const char* vals) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int j = 0; j < bits[len - 1]; ++j, ++k, ++code) tab[hexv(vals[2 * k]) * 16 + hexv(vals[2 * k + 1])] = code << 5 | len;
        code <<= 1;
    }
}
constexpr HuffTabs make_tabs() {
    HuffTabs t{};
    fill_codes(t.dc[0], DC_LUMA_BITS, DC_VALS);
    fill_codes(t.dc[1], DC_CHROMA_BITS, DC_VALS);
    fill_codes(t.ac[0], AC_LUMA_BITS, AC_LUMA_VALS);
    fill_codes(t.ac[1], AC_CHROMA_BITS, AC_CHROMA_VALS);
    return t;
}
__constant__ const HuffTabs c_huff = make_tabs();

// ---- transform --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) jpeg_above_one_kernel(const float* __restrict__ x, long count, uint32_t* flag) {
    bool any = false;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) any |= x[i] > 1.0f;
    if (__ballot(any) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// ---- entropy coding -----------------------------------------------------------------------------------------------------
// the shared bit sink behind the Annex K codes in constant memory; table = 0 Y DC, 1 Y AC, 2 chroma DC, 3 chroma AC
template <bool EMIT>
struct HuffSink : BitSink<EMIT> {
    __device__ __forceinline__ void symbol(int table, int sym, uint32_t value, int nbits) {
        const uint32_t e = (table & 1) ? c_huff.ac[table >> 1][sym] : c_huff.dc[table >> 1][sym];
        this->put(((e >> 5) << nbits) | value, (int)(e & 31u) + nbits);
    }
};

// one thread per scan-order block, dummy blocks included; the walk is jpegopt.h's, which clamps what baseline coding cannot carry, so
// a block never exceeds BLOCK_BITS_MAX bits
__global__ void __launch_bounds__(256) jpeg_bitlen_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ len, JpegGeo g) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)g.n * g.SB) return;
    const int img = (int)(t / g.SB), s = (int)(t - (long)img * g.SB);
    HuffSink<false> sink;
    sink.init(nullptr, 0, 0);
    jpegopt_walk_block(coef + (long)img * g.NB * 64, g, s, sink);
    len[t] = sink.count;
}

// one workgroup per image: lengths -> offsets in place, total[image] = the bits before the last padding.  T = uint32_t: a plain sum;
// T = BitFn (g.ri > 0): a block that a restart marker follows also fills its byte up and leaves 16 bits free
template <typename T>
__device__ __forceinline__ T scan_item(uint32_t len, const JpegGeo& g, int s);
template <>
__device__ __forceinline__ uint32_t scan_item<uint32_t>(uint32_t len, const JpegGeo&, int) { return len; }
template <>
__device__ __forceinline__ BitFn scan_item<BitFn>(uint32_t len, const JpegGeo& g, int s) { return jpegrst_block_fn(len, g, s); }
__device__ __forceinline__ uint32_t scan_value(uint32_t v) { return v; }
__device__ __forceinline__ uint32_t scan_value(const BitFn& f) { return f.at(0u); }

template <typename T>
__global__ void __launch_bounds__(SCAN_THREADS) jpeg_bitscan_kernel(uint32_t* __restrict__ off, uint32_t* __restrict__ total, JpegGeo g) {
    __shared__ T wtot[SCAN_THREADS / 64];
    const int SB = g.SB;
    uint32_t* o = off + (long)blockIdx.x * SB;
    T carry{};
    for (int b = 0; b < SB; b += SCAN_THREADS) {
        const int j = b + threadIdx.x;
        const T v = j < SB ? scan_item<T>(o[j], g, j) : T{};
        T sum;
        const T ex = block_excl_scan(v, wtot, sum);
        if (j < SB) o[j] = scan_value(carry + ex);
        carry = carry + sum;
    }
    if (threadIdx.x == 0) total[blockIdx.x] = scan_value(carry);
}

// zeroes the words the bits of an image will be OR-ed into (nothing beyond them, and never beyond the image's slot)
__global__ void __launch_bounds__(256) jpeg_zero_kernel(uint32_t* __restrict__ raw, const uint32_t* __restrict__ total, unsigned raw_words) {
    const unsigned img = blockIdx.y;
    const unsigned need = min(raw_words, ((total[img] + 7u) / 8u + 3u) / 4u);
    const unsigned i = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (i >= need) return;                               // raw_words is a multiple of 4 and the slot 16-byte aligned
    *reinterpret_cast<uint4*>(raw + (size_t)img * raw_words + i) = make_uint4(0u, 0u, 0u, 0u);
}

__global__ void __launch_bounds__(256) jpeg_emit_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ off,
                                                        uint32_t* __restrict__ raw, JpegGeo g, unsigned raw_words) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)g.n * g.SB) return;
    const int img = (int)(t / g.SB), s = (int)(t - (long)img * g.SB);
    HuffSink<true> sink;
    sink.init(raw + (size_t)img * raw_words, raw_words, off[t]);
    jpegopt_walk_block(coef + (long)img * g.NB * 64, g, s, sink);
    pad_interval(sink, g, s, off[t]);
    sink.finish();
}

__device__ __forceinline__ unsigned ff_bytes(uint32_t word) {
    return (unsigned)((word >> 24) == 0xffu) + (unsigned)(((word >> 16) & 0xffu) == 0xffu) +
           (unsigned)(((word >> 8) & 0xffu) == 0xffu) + (unsigned)((word & 0xffu) == 0xffu);
}

// one workgroup per image: lengths[image] = its bytes + its FF bytes.  The bytes past the end of the last word are zero.
__global__ void __launch_bounds__(SCAN_THREADS) jpeg_count_kernel(const uint32_t* __restrict__ raw, const uint32_t* __restrict__ total,
                                                                  uint32_t* __restrict__ lengths, unsigned raw_words) {
    __shared__ uint32_t wtot[SCAN_THREADS / 64];
    const unsigned img = blockIdx.x, nbytes = (total[img] + 7u) / 8u, nwords = min(raw_words, (nbytes + 3u) / 4u);
    const uint32_t* r = raw + (size_t)img * raw_words;
    uint32_t cnt = 0;
    for (unsigned j = threadIdx.x; j < nwords; j += SCAN_THREADS) cnt += ff_bytes(r[j]);
    uint32_t sum;
    block_excl_scan(cnt, wtot, sum);
    if (threadIdx.x == 0) lengths[img] = nbytes + sum;
}

// one workgroup: dst[image] = sum of the lengths before it
__global__ void __launch_bounds__(SCAN_THREADS) jpeg_imgscan_kernel(const uint32_t* __restrict__ lengths, unsigned long long* __restrict__ dst,
                                                                    int n) {
    __shared__ unsigned long long wtot[SCAN_THREADS / 64];
    const int per = (n + SCAN_THREADS - 1) / SCAN_THREADS, j0 = min(n, (int)threadIdx.x * per), j1 = min(n, j0 + per);
    unsigned long long loc = 0, sum;
    for (int j = j0; j < j1; ++j) loc += lengths[j];
    unsigned long long run = block_excl_scan(loc, wtot, sum);
    for (int j = j0; j < j1; ++j) {
        dst[j] = run;
        run += lengths[j];
    }
}

// one workgroup per image: its bytes to dst[image] + position + FF bytes before it, every FF followed by 00.  RST: the bytes left
// free for the restart markers are zero in raw - counted and placed like data, never stuffed - and go out as the markers
template <bool RST>
__global__ void __launch_bounds__(SCAN_THREADS) jpeg_stuff_kernel(const uint32_t* __restrict__ raw, const uint32_t* __restrict__ total,
                                                                  const uint32_t* __restrict__ off,
                                                                  const unsigned long long* __restrict__ dst, uint8_t* __restrict__ out,
                                                                  unsigned long long capacity, JpegGeo g, unsigned raw_words) {
    __shared__ uint32_t wtot[SCAN_THREADS / 64];
    const unsigned img = blockIdx.x, nbytes = (total[img] + 7u) / 8u, nwords = min(raw_words, (nbytes + 3u) / 4u);
    const uint32_t* r = raw + (size_t)img * raw_words;
    const uint32_t* o = off + (size_t)img * g.SB;
    const unsigned long long d0 = dst[img];
    uint32_t carry = 0;
    for (unsigned b = 0; b < nwords; b += SCAN_THREADS) {
        const unsigned j = b + threadIdx.x;
        const uint32_t word = j < nwords ? r[j] : 0u;
        uint32_t sum;
        uint32_t before = carry + block_excl_scan((uint32_t)ff_bytes(word), wtot, sum);
        carry += sum;
        if (j < nwords) {
            const int k0 = RST ? jpegrst_first_marker(o, g, 4u * j) : 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned pos = 4u * j + (unsigned)q;
                const uint32_t byte = (word >> (24 - 8 * q)) & 0xffu;
                if (pos < nbytes) {
                    const unsigned long long at = d0 + pos + before;
                    const uint32_t mark = RST ? jpegrst_marker_byte(o, g, k0, pos) : 0u;
                    if (at < capacity) out[at] = (uint8_t)(mark ? mark : byte);
                    if (byte == 0xffu) {
                        if (at + 1 < capacity) out[at + 1] = 0;
                        ++before;
                    }
                }
            }
        }
    }
}

// ---- reconstruct --------------------------------------------------------------------------------------------------------
// one thread per pixel: clamp, then k / 255 in float32 or the byte itself.  UP: jpegc.h's up-sampler of the chroma, CHROMA_FANCY for
// every geometry but those of section 4r
template <bool U8, int UP = CHROMA_FANCY>
__global__ void __launch_bounds__(256) jpeg_colour_kernel(uint8_t* __restrict__ planes, void* __restrict__ out, JpegGeo g) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)g.n * g.h * g.w) return;
    const int img = (int)(t / ((long)g.h * g.w)), r = (int)(t - (long)img * g.h * g.w), y = r / g.w, x = r - y * g.w;
    const int yy = plane_of(planes, g, img, 0)[(size_t)y * 8 * g.bwY + x];
    if (g.nc == 1) {                                     // grey-scale: the range-limited sample is the pixel
        if (U8) ((uint8_t*)out)[t] = (uint8_t)yy;
        else ((float*)out)[t] = __fdiv_rn((float)yy, 255.0f);
        return;
    }
    const int cb = chroma_sample<UP>(plane_of(planes, g, img, 1), g, y, x) - 128;
    const int cr = chroma_sample<UP>(plane_of(planes, g, img, 2), g, y, x) - 128;
    const int R = min(max(red_of(yy, cr), 0), 255);
    const int G = min(max(green_of(yy, cb, cr), 0), 255);
    const int B = min(max(blue_of(yy, cb), 0), 255);
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

// ---- the launchers: one per operation, for files of three components (nc = 3) and of one (nc = 1, section 4p) -------------------
int transform_launch(const void* x, int is_u8, int n, int h, int w, int hs, int vs, int nc, int quality, int16_t* coef, void* workspace,
                     size_t workspace_bytes, void* stream) {
    JpegGeo g;
    if (!x || !coef || !workspace || quality < 1 || quality > 100 || !make_geo(&g, n, h, w, hs, vs, nc)) return NIMG_ERR_ARG;
    const Workspace ws = carve(g, workspace);
    if (workspace_bytes < ws.bytes) return NIMG_ERR_WORKSPACE;
    const long blocks = (long)n * g.NB;
    if (!grid_ok(blocks, 256)) return NIMG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const BatchTables tabs{make_qtabs(quality)};
    const unsigned grid = (unsigned)((blocks + 255) / 256);
    const uint32_t* flag = ws.flag;
    if (!is_u8) {
        const int rc = nimg_internal_jpeg_above_one((const float*)x, (long)n * h * w * nc, ws.flag, st);
        if (rc != NIMG_OK) return rc;
    }
    if (nc == 1) {
        if (is_u8) hipLaunchKernelGGL((jpeg_transform_kernel<true, BatchTables, true>), dim3(grid), dim3(256), 0, st, x, coef, g, tabs, flag);
        else hipLaunchKernelGGL((jpeg_transform_kernel<false, BatchTables, true>), dim3(grid), dim3(256), 0, st, x, coef, g, tabs, flag);
    } else {
        if (is_u8) hipLaunchKernelGGL((jpeg_transform_kernel<true, BatchTables>), dim3(grid), dim3(256), 0, st, x, coef, g, tabs, flag);
        else hipLaunchKernelGGL((jpeg_transform_kernel<false, BatchTables>), dim3(grid), dim3(256), 0, st, x, coef, g, tabs, flag);
    }
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

size_t workspace_size(int n, int h, int w, int hs, int vs, int nc, int restart_interval) {
    JpegGeo g;
    if (!make_geo(&g, n, h, w, hs, vs, nc) || !set_restart(&g, restart_interval)) return 0;
    return carve(g, nullptr).bytes;
}

int encode_launch(const int16_t* coef, int n, int h, int w, int hs, int vs, int nc, int restart_interval, uint8_t* out,
                  size_t out_capacity, uint32_t* lengths, void* workspace, size_t workspace_bytes, void* stream) {
    JpegGeo g;
    if (!coef || !out || !lengths || !workspace || !make_geo(&g, n, h, w, hs, vs, nc) || !set_restart(&g, restart_interval))
        return NIMG_ERR_ARG;
    const Workspace ws = carve(g, workspace);
    if (workspace_bytes < ws.bytes) return NIMG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long blocks = (long)n * g.SB;
    const unsigned grid = (unsigned)((blocks + 255) / 256);
    hipLaunchKernelGGL(jpeg_bitlen_kernel, dim3(grid), dim3(256), 0, st, coef, ws.off, g);
    NIMG_CHECK_LAUNCH();
    const int rc = nimg_internal_jpeg_offsets(ws.off, ws.total, ws.raw, g, ws.raw_words, st);
    if (rc != NIMG_OK) return rc;
    hipLaunchKernelGGL(jpeg_emit_kernel, dim3(grid), dim3(256), 0, st, coef, (const uint32_t*)ws.off, ws.raw, g, ws.raw_words);
    NIMG_CHECK_LAUNCH();
    return nimg_internal_jpeg_pack(ws.raw, ws.total, ws.off, lengths, ws.dst, out, out_capacity, g, ws.raw_words, st);
}

}  // namespace

extern "C" {

size_t nimg_jpeg_workspace_bytes(int n, int h, int w, int hs, int vs) { return workspace_size(n, h, w, hs, vs, 3, 0); }

int nimg_jpeg_transform(const void* x, int is_u8, int n, int h, int w, int hs, int vs, int quality, int16_t* coef, void* workspace,
                        size_t workspace_bytes, void* stream) {
    return transform_launch(x, is_u8, n, h, w, hs, vs, 3, quality, coef, workspace, workspace_bytes, stream);
}

size_t nimg_jpeg_encode_restart_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval) {
    return workspace_size(n, h, w, hs, vs, 3, restart_interval);
}

int nimg_jpeg_encode_restart(const int16_t* coef, int n, int h, int w, int hs, int vs, int restart_interval, uint8_t* out,
                             size_t out_capacity, uint32_t* lengths, void* workspace, size_t workspace_bytes, void* stream) {
    return encode_launch(coef, n, h, w, hs, vs, 3, restart_interval, out, out_capacity, lengths, workspace, workspace_bytes, stream);
}

size_t nimg_jpeg_grey_workspace_bytes(int n, int h, int w, int restart_interval) {
    return workspace_size(n, h, w, 1, 1, 1, restart_interval);
}

int nimg_jpeg_grey_transform(const void* x, int is_u8, int n, int h, int w, int quality, int16_t* coef, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (n == 0) return NIMG_OK;
    return transform_launch(x, is_u8, n, h, w, 1, 1, 1, quality, coef, workspace, workspace_bytes, stream);
}

int nimg_jpeg_grey_encode(const int16_t* coef, int n, int h, int w, int restart_interval, uint8_t* out, size_t out_capacity,
                          uint32_t* lengths, void* workspace, size_t workspace_bytes, void* stream) {
    if (n == 0) return NIMG_OK;
    return encode_launch(coef, n, h, w, 1, 1, 1, restart_interval, out, out_capacity, lengths, workspace, workspace_bytes, stream);
}

int nimg_jpeg_encode(const int16_t* coef, int n, int h, int w, int hs, int vs, uint8_t* out, size_t out_capacity, uint32_t* lengths,
                     void* workspace, size_t workspace_bytes, void* stream) {
    return nimg_jpeg_encode_restart(coef, n, h, w, hs, vs, 0, out, out_capacity, lengths, workspace, workspace_bytes, stream);
}

int nimg_jpeg_reconstruct(const int16_t* coef, int n, int h, int w, int hs, int vs, int quality, float* y, void* workspace,
                          size_t workspace_bytes, void* stream) {
    JpegGeo g;
    if (!coef || !y || !workspace || quality < 1 || quality > 100 || !make_geo(&g, n, h, w, hs, vs)) return NIMG_ERR_ARG;
    const Workspace ws = carve(g, workspace);
    if (workspace_bytes < ws.bytes) return NIMG_ERR_WORKSPACE;
    const long blocks = (long)n * g.NB, pixels = (long)n * h * w;
    if (!grid_ok(blocks, 256) || !grid_ok(pixels, 256)) return NIMG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_idct_kernel<BatchTables>, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, st, coef, ws.planes, g,
                       BatchTables{make_qtabs(quality)});
    NIMG_CHECK_LAUNCH();
    return nimg_internal_jpeg_colour(ws.planes, y, false, g, st);
}

}  // extern "C"

int nimg_internal_jpeg_above_one(const float* x, long count, uint32_t* flag, hipStream_t stream) {
    if (hipMemsetAsync(flag, 0, 4, stream) != hipSuccess) return NIMG_ERR_LAUNCH;
    hipLaunchKernelGGL(jpeg_above_one_kernel, dim3((unsigned)((count + 255) / 256 < 4096 ? (count + 255) / 256 : 4096)), dim3(256), 0, stream, x,
                       count, flag);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_internal_jpeg_colour(uint8_t* planes, void* y, bool u8, const JpegGeo& g, hipStream_t stream) {
    const long pixels = (long)g.n * g.h * g.w;
    if (!grid_ok(pixels, 256)) return NIMG_ERR_ARG;
    const dim3 grid((unsigned)((pixels + 255) / 256));
    const int up = g.nc == 1 ? CHROMA_FANCY : jpeg_chroma_mode(g);
    if (up == CHROMA_H1V2) {
        if (u8) hipLaunchKernelGGL((jpeg_colour_kernel<true, CHROMA_H1V2>), grid, dim3(256), 0, stream, planes, y, g);
        else hipLaunchKernelGGL((jpeg_colour_kernel<false, CHROMA_H1V2>), grid, dim3(256), 0, stream, planes, y, g);
    } else if (up == CHROMA_REPLICATE) {
        if (u8) hipLaunchKernelGGL((jpeg_colour_kernel<true, CHROMA_REPLICATE>), grid, dim3(256), 0, stream, planes, y, g);
        else hipLaunchKernelGGL((jpeg_colour_kernel<false, CHROMA_REPLICATE>), grid, dim3(256), 0, stream, planes, y, g);
    } else if (u8) hipLaunchKernelGGL(jpeg_colour_kernel<true>, grid, dim3(256), 0, stream, planes, y, g);
    else hipLaunchKernelGGL(jpeg_colour_kernel<false>, grid, dim3(256), 0, stream, planes, y, g);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_internal_jpeg_offsets(uint32_t* off, uint32_t* total, uint32_t* raw, const JpegGeo& g, unsigned raw_words, hipStream_t stream) {
    if (g.ri) hipLaunchKernelGGL(jpeg_bitscan_kernel<BitFn>, dim3((unsigned)g.n), dim3(SCAN_THREADS), 0, stream, off, total, g);
    else hipLaunchKernelGGL(jpeg_bitscan_kernel<uint32_t>, dim3((unsigned)g.n), dim3(SCAN_THREADS), 0, stream, off, total, g);
    NIMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_zero_kernel, dim3((raw_words / 4 + 255) / 256, (unsigned)g.n), dim3(256), 0, stream, raw, (const uint32_t*)total,
                       raw_words);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_internal_jpeg_pack(const uint32_t* raw, const uint32_t* total, const uint32_t* off, uint32_t* lengths, unsigned long long* dst,
                            uint8_t* out, size_t capacity, const JpegGeo& g, unsigned raw_words, hipStream_t stream) {
    const int n = g.n;
    hipLaunchKernelGGL(jpeg_count_kernel, dim3((unsigned)n), dim3(SCAN_THREADS), 0, stream, raw, total, lengths, raw_words);
    NIMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_imgscan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, (const uint32_t*)lengths, dst, n);
    NIMG_CHECK_LAUNCH();
    if (g.ri)
        hipLaunchKernelGGL(jpeg_stuff_kernel<true>, dim3((unsigned)n), dim3(SCAN_THREADS), 0, stream, raw, total, off,
                           (const unsigned long long*)dst, out, (unsigned long long)capacity, g, raw_words);
    else
        hipLaunchKernelGGL(jpeg_stuff_kernel<false>, dim3((unsigned)n), dim3(SCAN_THREADS), 0, stream, raw, total, off,
                           (const unsigned long long*)dst, out, (unsigned long long)capacity, g, raw_words);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}
