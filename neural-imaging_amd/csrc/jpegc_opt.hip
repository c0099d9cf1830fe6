// Writing JPEG files with optimised Huffman tables (libjpeg's optimize_coding): per image the symbol statistics,
// libjpeg's optimal tables from them, and the entropy coder of section 4c with the tables of each image read from memory.
//   histogram       coefficients -> hist[image][00 | 10 | 01 | 11][257]: one thread per scan block, a workgroup belongs to one image and
//                   counts in LDS, then one integer atomicAdd per non-zero bin
//   optimal_tables  histograms -> tables as a DHT segment has them (16 counts, 256 symbols): one wave per table, the 257 frequencies in
//                   registers (5 per lane), every merge two wave-wide arg-min reductions, the tree update parallel over the lanes;
//                   the sizes are counted and the symbols ranked with ballots, one lane folds the counts back to 16 bits
//   encode_tables   derive the code words of every image into the workspace | bit length of every block | jpegc.hip's scan and zero
//                   passes | emit | jpegc.hip's count, image scan and stuff passes.  The bit-length and the emit kernel keep their
//                   image's 544 code words in LDS, so a workgroup never spans two images.
// The block walk, the length limiting and the derive step are csrc/jpegopt.h's, which tests/jpegopt_host.cpp runs on the host; the bit
// sink and the workspace layout are jpegc.h's, shared with jpegc.hip.
#include "jpegc.h"
#include "jpegopt.h"

namespace {

// ---- histogram ----------------------------------------------------------------------------------------------------------
struct HistSink {
    uint32_t* hist;                    // LDS, [4][257]
    __device__ __forceinline__ void symbol(int table, int sym, uint32_t, int) { atomicAdd(hist + table * JPEGOPT_HIST + sym, 1u); }
};

// grid (ceil(SB / 256), n)
__global__ void __launch_bounds__(256) jpeg_histogram_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ hist, JpegGeo g) {
    __shared__ uint32_t s_hist[4 * JPEGOPT_HIST];
    for (int i = threadIdx.x; i < 4 * JPEGOPT_HIST; i += 256) s_hist[i] = 0;
    __syncthreads();
    const int img = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x;
    if (s < g.SB) {
        HistSink sink{s_hist};
        jpegopt_walk_block(coef + (long)img * g.NB * 64, g, s, sink);
    }
    __syncthreads();
    const int bins = jpegopt_tables(g) * JPEGOPT_HIST;   // a grey-scale file has the two luma histograms alone
    uint32_t* dst = hist + (size_t)img * bins;
    for (int i = threadIdx.x; i < bins; i += 256) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(dst + i, v);
    }
}

// ---- optimal tables -------------------------------------------------------------------------------------------------------
constexpr unsigned long long NO_KEY = ~0ull;

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// 4 tables per workgroup, one wave each.  Lane l holds the entries l, l + 64, l + 128, l + 192 and (lane 0 only) the pseudo-symbol 256.
// The smallest non-zero frequency with the largest index is the smallest key (frequency << 9) | (256 - index).
__global__ void __launch_bounds__(256) jpeg_optimal_tables_kernel(const uint32_t* __restrict__ hist, int n_tables,
                                                                  uint8_t* __restrict__ tables, uint32_t* __restrict__ status) {
    __shared__ uint32_t s_bits[4][33];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, tab = blockIdx.x * 4 + wv;
    const bool active = tab < n_tables;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t f[5];
    int tree[5], size[5];
    unsigned long long total = 0;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int idx = r * 64 + lane;
        f[r] = !active || idx > 256 ? 0u : (idx == 256 ? 1u : hist[(size_t)tab * JPEGOPT_HIST + idx]);
        tree[r] = idx;
        size[r] = 0;
        total += f[r];
    }
    total = wave_sum(total);
    uint32_t st = total >= (1ull << 32) ? JPEGOPT_ST_TOTAL : 0u;
    if (st) {
#pragma unroll
        for (int r = 0; r < 5; ++r) f[r] = 0;
    }
    for (int it = 0; it < 256; ++it) {                       // 257 entries merge at most 256 times
        unsigned long long k1 = NO_KEY, k2 = NO_KEY;
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const unsigned long long k = f[r] ? ((unsigned long long)f[r] << 9) | (unsigned)(256 - (r * 64 + lane)) : NO_KEY;
            k1 = k < k1 ? k : k1;
        }
        k1 = wave_min(k1);
        if (k1 == NO_KEY) break;
        const int c1 = 256 - (int)(k1 & 511u);
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const int idx = r * 64 + lane;
            const unsigned long long k = f[r] && idx != c1 ? ((unsigned long long)f[r] << 9) | (unsigned)(256 - idx) : NO_KEY;
            k2 = k < k2 ? k : k2;
        }
        k2 = wave_min(k2);
        if (k2 == NO_KEY) break;
        const int c2 = 256 - (int)(k2 & 511u);
        const uint32_t sum = (uint32_t)(k1 >> 9) + (uint32_t)(k2 >> 9);         // below 2^32: the total was checked
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const int idx = r * 64 + lane;
            if (idx == c1) f[r] = sum;
            if (idx == c2) f[r] = 0;
            if (tree[r] == c1 || tree[r] == c2) {
                ++size[r];
                tree[r] = c1;
            }
        }
    }
    bool big = false;
#pragma unroll
    for (int r = 0; r < 5; ++r) big |= size[r] > 32;
    if (__ballot(big) != 0) st |= JPEGOPT_ST_OVERFLOW;
    // the number of codes of every size, the pseudo-symbol included
    for (int l = 0; l <= 32; ++l) {
        unsigned n = 0;
#pragma unroll
        for (int r = 0; r < 5; ++r) n += (unsigned)__popcll(__ballot(l > 0 && size[r] == l));
        if (lane == 0) s_bits[wv][l] = n;
    }
    __syncthreads();
    if (lane == 0 && st == 0) jpegopt_limit_bits(s_bits[wv]);        // (the counts of a refused histogram are no code: not folded)
    __syncthreads();
    if (!active) return;
    uint8_t* row = tables + (size_t)tab * JPEGOPT_TABLE_BYTES;
    if (lane == 0) status[tab] = st;
    if (st) {
        for (int i = lane; i < JPEGOPT_TABLE_BYTES; i += 64) row[i] = 0;
        return;
    }
    if (lane < 16) row[lane] = (uint8_t)s_bits[wv][lane + 1];
    // the symbols by unlimited code size, then by value: entry r * 64 + lane ranks behind the entries of lower r and lower lanes
    unsigned base = 0;
    for (int l = 1; l <= 32; ++l) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned long long mask = __ballot(size[r] == l);
            if (size[r] == l) row[16 + base + (unsigned)__popcll(mask & below)] = (uint8_t)(r * 64 + lane);
            base += (unsigned)__popcll(mask);
        }
    }
    for (unsigned i = base + lane; i < 256; i += 64) row[16 + i] = 0;
}

// ---- entropy coding with the tables of each image ----------------------------------------------------------------------------
// one thread per image: status[image] = JPEGOPT_ST_TABLE or 0 (the call's only plain store to it; the bit-length pass ORs into it)
__global__ void __launch_bounds__(64) jpeg_derive_kernel(const uint8_t* __restrict__ tables, uint32_t* __restrict__ codes,
                                                         uint32_t* __restrict__ status, int n, int n_tables) {
    const int img = blockIdx.x * 64 + threadIdx.x;
    if (img >= n) return;
    const bool ok = jpegopt_derive_image(tables + (size_t)img * n_tables * JPEGOPT_TABLE_BYTES, codes + (size_t)img * JPEGOPT_CODE_WORDS,
                                         n_tables);
    status[img] = ok ? 0u : JPEGOPT_ST_TABLE;
}

// jpegc.h's bit sink behind the code words of one image; a symbol without a code puts nothing and sets `missing`
template <bool EMIT>
struct CodeSink : BitSink<EMIT> {
    const uint32_t* codes;             // LDS
    bool missing = false;
    __device__ __forceinline__ void symbol(int table, int sym, uint32_t value, int nbits) {
        const uint32_t e = codes[jpegopt_code_index(table, sym)];
        if (e == 0) { missing = true; return; }
        this->put(((e >> 5) << nbits) | value, (int)(e & 31u) + nbits);
    }
};

__device__ __forceinline__ void load_codes(uint32_t* s_codes, const uint32_t* __restrict__ codes, int img) {
    for (int i = threadIdx.x; i < JPEGOPT_CODE_WORDS; i += 256) s_codes[i] = codes[(size_t)img * JPEGOPT_CODE_WORDS + i];
    __syncthreads();
}

// grid (ceil(SB / 256), n).  An image whose tables were refused gets length 0 for every block.
__global__ void __launch_bounds__(256) jpeg_bitlen_tables_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ codes,
                                                                 uint32_t* __restrict__ len, uint32_t* __restrict__ status, JpegGeo g) {
    __shared__ uint32_t s_codes[JPEGOPT_CODE_WORDS];
    const int img = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x;
    load_codes(s_codes, codes, img);
    if (s >= g.SB) return;
    CodeSink<false> sink;
    sink.codes = s_codes;
    sink.init(nullptr, 0, 0);
    const bool refused = (status[img] & JPEGOPT_ST_TABLE) != 0;          // written by the derive pass, before this kernel began
    if (!refused) jpegopt_walk_block(coef + (long)img * g.NB * 64, g, s, sink);
    len[(size_t)img * g.SB + s] = sink.count;
    if (sink.missing) atomicOr(status + img, JPEGOPT_ST_SYMBOL);
}

__global__ void __launch_bounds__(256) jpeg_emit_tables_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ codes,
                                                               const uint32_t* __restrict__ off,
                                                               const uint32_t* __restrict__ status, uint32_t* __restrict__ raw,
                                                               JpegGeo g, unsigned raw_words) {
    __shared__ uint32_t s_codes[JPEGOPT_CODE_WORDS];
    const int img = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x;
    load_codes(s_codes, codes, img);
    if (s >= g.SB || (status[img] & JPEGOPT_ST_TABLE) != 0) return;
    CodeSink<true> sink;
    sink.codes = s_codes;
    sink.init(raw + (size_t)img * raw_words, raw_words, off[(size_t)img * g.SB + s]);
    jpegopt_walk_block(coef + (long)img * g.NB * 64, g, s, sink);
    pad_interval(sink, g, s, off[(size_t)img * g.SB + s]);
    sink.finish();
}

// ---- the launchers, for files of three components (nc = 3) and of one (nc = 1, section 4p) ----------------------------------------
int histogram_launch(const int16_t* coef, int n, int h, int w, int hs, int vs, int nc, int restart_interval, uint32_t* hist, void* stream,
                     int factors = JPEG_FACTORS_THREE) {
    JpegGeo g;
    if (!coef || !hist || !make_geo(&g, n, h, w, hs, vs, nc, factors) || !set_restart(&g, restart_interval)) return NIMG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (size_t)n * jpegopt_tables(g) * JPEGOPT_HIST * 4, st) != hipSuccess) return NIMG_ERR_LAUNCH;
    hipLaunchKernelGGL(jpeg_histogram_kernel, dim3((unsigned)((g.SB + 255) / 256), (unsigned)n), dim3(256), 0, st, coef, hist, g);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

size_t tables_workspace_size(int n, int h, int w, int hs, int vs, int nc, int restart_interval, int factors = JPEG_FACTORS_THREE) {
    JpegGeo g;
    if (!make_geo(&g, n, h, w, hs, vs, nc, factors) || !set_restart(&g, restart_interval)) return 0;
    return carve(g, nullptr, JPEGOPT_BLOCK_BITS_MAX, JPEGOPT_CODE_WORDS).bytes;
}

int encode_tables_launch(const int16_t* coef, int n, int h, int w, int hs, int vs, int nc, int restart_interval, const uint8_t* tables,
                         uint8_t* out, size_t out_capacity, uint32_t* lengths, uint32_t* status, void* workspace, size_t workspace_bytes,
                         void* stream, int factors = JPEG_FACTORS_THREE) {
    JpegGeo g;
    if (!coef || !tables || !out || !lengths || !status || !workspace || !make_geo(&g, n, h, w, hs, vs, nc, factors) ||
        !set_restart(&g, restart_interval))
        return NIMG_ERR_ARG;
    const Workspace ws = carve(g, workspace, JPEGOPT_BLOCK_BITS_MAX, JPEGOPT_CODE_WORDS);
    if (workspace_bytes < ws.bytes) return NIMG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((g.SB + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(jpeg_derive_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, tables, ws.codes, status, n, jpegopt_tables(g));
    NIMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_bitlen_tables_kernel, grid, dim3(256), 0, st, coef, (const uint32_t*)ws.codes, ws.off, status, g);
    NIMG_CHECK_LAUNCH();
    int rc = nimg_internal_jpeg_offsets(ws.off, ws.total, ws.raw, g, ws.raw_words, st);
    if (rc != NIMG_OK) return rc;
    hipLaunchKernelGGL(jpeg_emit_tables_kernel, grid, dim3(256), 0, st, coef, (const uint32_t*)ws.codes, (const uint32_t*)ws.off,
                       (const uint32_t*)status, ws.raw, g, ws.raw_words);
    NIMG_CHECK_LAUNCH();
    return nimg_internal_jpeg_pack(ws.raw, ws.total, ws.off, lengths, ws.dst, out, out_capacity, g, ws.raw_words, st);
}

}  // namespace

extern "C" {

int nimg_jpeg_histogram_restart(const int16_t* coef, int n, int h, int w, int hs, int vs, int restart_interval, uint32_t* hist,
                                void* stream) {
    return histogram_launch(coef, n, h, w, hs, vs, 3, restart_interval, hist, stream);
}

int nimg_jpeg_grey_histogram(const int16_t* coef, int n, int h, int w, int restart_interval, uint32_t* hist, void* stream) {
    if (n == 0) return NIMG_OK;
    return histogram_launch(coef, n, h, w, 1, 1, 1, restart_interval, hist, stream);
}

size_t nimg_jpeg_grey_encode_tables_workspace_bytes(int n, int h, int w, int restart_interval) {
    return tables_workspace_size(n, h, w, 1, 1, 1, restart_interval);
}

int nimg_jpeg_grey_encode_tables(const int16_t* coef, int n, int h, int w, int restart_interval, const uint8_t* tables, uint8_t* out,
                                 size_t out_capacity, uint32_t* lengths, uint32_t* status, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    if (n == 0) return NIMG_OK;
    return encode_tables_launch(coef, n, h, w, 1, 1, 1, restart_interval, tables, out, out_capacity, lengths, status, workspace,
                                workspace_bytes, stream);
}

// the same launchers with the wide set of sampling factors
int nimg_jpeg_sampling_histogram(const int16_t* coef, int n, int h, int w, int hs, int vs, int restart_interval, uint32_t* hist,
                                 void* stream) {
    return histogram_launch(coef, n, h, w, hs, vs, 3, restart_interval, hist, stream, JPEG_FACTORS_WIDE);
}

size_t nimg_jpeg_sampling_encode_tables_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval) {
    return tables_workspace_size(n, h, w, hs, vs, 3, restart_interval, JPEG_FACTORS_WIDE);
}

int nimg_jpeg_sampling_encode_tables(const int16_t* coef, int n, int h, int w, int hs, int vs, int restart_interval, const uint8_t* tables,
                                     uint8_t* out, size_t out_capacity, uint32_t* lengths, uint32_t* status, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    return encode_tables_launch(coef, n, h, w, hs, vs, 3, restart_interval, tables, out, out_capacity, lengths, status, workspace,
                                workspace_bytes, stream, JPEG_FACTORS_WIDE);
}

int nimg_jpeg_histogram(const int16_t* coef, int n, int h, int w, int hs, int vs, uint32_t* hist, void* stream) {
    return nimg_jpeg_histogram_restart(coef, n, h, w, hs, vs, 0, hist, stream);
}

int nimg_jpeg_optimal_tables(const uint32_t* hist, int n_tables, uint8_t* tables, uint32_t* status, void* stream) {
    if (!hist || !tables || !status || n_tables < 1 || n_tables > 4 * 65535) return NIMG_ERR_ARG;
    hipLaunchKernelGGL(jpeg_optimal_tables_kernel, dim3((unsigned)((n_tables + 3) / 4)), dim3(256), 0, (hipStream_t)stream, hist, n_tables,
                       tables, status);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

size_t nimg_jpeg_encode_tables_restart_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval) {
    return tables_workspace_size(n, h, w, hs, vs, 3, restart_interval);
}

size_t nimg_jpeg_encode_tables_workspace_bytes(int n, int h, int w, int hs, int vs) {
    return nimg_jpeg_encode_tables_restart_workspace_bytes(n, h, w, hs, vs, 0);
}

int nimg_jpeg_encode_tables_restart(const int16_t* coef, int n, int h, int w, int hs, int vs, int restart_interval, const uint8_t* tables,
                                    uint8_t* out, size_t out_capacity, uint32_t* lengths, uint32_t* status, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return encode_tables_launch(coef, n, h, w, hs, vs, 3, restart_interval, tables, out, out_capacity, lengths, status, workspace,
                                workspace_bytes, stream);
}

int nimg_jpeg_encode_tables(const int16_t* coef, int n, int h, int w, int hs, int vs, const uint8_t* tables, uint8_t* out,
                            size_t out_capacity, uint32_t* lengths, uint32_t* status, void* workspace, size_t workspace_bytes,
                            void* stream) {
    return nimg_jpeg_encode_tables_restart(coef, n, h, w, hs, vs, 0, tables, out, out_capacity, lengths, status, workspace, workspace_bytes,
                                           stream);
}

}  // extern "C"
