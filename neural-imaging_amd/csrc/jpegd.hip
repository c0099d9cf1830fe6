// Decoder of baseline JPEG files: the entropy-coded segments of a batch -> the coefficient tensor of
// jpegc.hip, by the self-synchronisation of Huffman codes (Weissenberger and Schmidt), and the coefficients -> images with the
// tables of each file.
//   prepare    one workgroup per image: the six Huffman tables from the DHT counts; the segment without its stuffing (FF 00 -> FF),
//              MSB first in 32-bit words, by a block scan with a carry; the number of subsequences
//   speculate  one thread per subsequence of subseq_bits bits: decode from the guess (m, z) = (0, 0), store exit state and blocks begun
//   sync       one workgroup per image: the rounds of jpegd_sync.h - which also says why their number is the host program's for every
//              chunking - then the exclusive scan of the block counts
//   write      one thread per subsequence: decode from the true state; AC values into coef, DC differences into a scan-order array
//   dc         one workgroup per (image, component): prefix sum of the differences, dummy blocks included, into position 0
// The sequential core - tables, block placement, the decode of one subsequence - is jpegd.h, shared with a host program.
// Files with a restart interval (nimg_jpeg_decode_restart) go through the same kernels, instantiated with
// RST: prepare also takes the markers FF D0 .. D7 out, checks their sequence and records where every interval begins; the
// subsequences are cut per interval, the first of each starts from the known state (interval start, m 0, z 0) and is never decoded
// again, a run ends with its interval's blocks, and the DC sums restart with every interval.
#include "jpegc.h"
#include "jpegd.h"
#include "jpegd_prepare.h"
#include "jpegd_sync.h"

namespace {

constexpr int DEC_THREADS = 256;
constexpr int SYNC_THREADS = 256;        // the workgroup that synchronises one image; longer images are walked in chunks of it
constexpr uint32_t SUBSEQ_DEFAULT = 2048;        // the fastest setting measured

struct DLayout {
    uint32_t* total_bits;        // [n] bits of an image's un-stuffed stream
    uint32_t* nsub;              // [n] its subsequences (0: the image is not decoded)
    JpegdTable* tabs;            // [n][2 nc]: six, or the two of a grey-scale file
    int32_t* dcdiff;             // [n][SB] DC differences in scan order
    uint32_t* raw;               // un-stuffed streams; image i from word (ecd_off[i] >> 2) + 2 i, (len + 3) / 4 + 1 words
    JpegdState* exit;            // exit states; image i from slot 8 ecd_off[i] / subseq_bits + i
    uint32_t* cnt;               // blocks begun, then (in place) the index of the first block begun; slots as `exit`
    uint32_t* ibit;              // restart intervals only: [n][K + 1] the bit every interval begins at (jpegd.h)
    uint32_t* sub0;              // restart intervals only: [n][K + 1] the first subsequence of every interval
    uint32_t* maxsub;            // restart intervals only: [n] the subsequences of the image's longest interval
    size_t raw_words, slots, bytes;
};

// slots an image has beyond 8 * its bytes / subseq_bits: one for the partial subsequence at its end - with restart intervals one
// per interval, and one more because an interval has at least one
inline uint32_t slot_extra(const JpegGeo& g) { return g.ri ? jpegd_intervals(g) + 1u : 1u; }

DLayout carve_d(const JpegGeo& g, uint64_t ecd_bytes, uint32_t sb, void* base) {
    DLayout d;
    uint8_t* p = (uint8_t*)base;
    d.total_bits = (uint32_t*)p; p += align256((size_t)g.n * 4);
    d.nsub = (uint32_t*)p; p += align256((size_t)g.n * 4);
    d.tabs = (JpegdTable*)p; p += align256((size_t)g.n * 2 * g.nc * sizeof(JpegdTable));
    d.dcdiff = (int32_t*)p; p += align256((size_t)g.n * g.SB * 4);
    d.raw_words = (size_t)(ecd_bytes / 4) + 2 * (size_t)g.n + 2;
    d.raw = (uint32_t*)p; p += align256(d.raw_words * 4);
    d.slots = (size_t)(8 * ecd_bytes / sb) + (size_t)g.n * slot_extra(g) + 1;
    d.exit = (JpegdState*)p; p += align256(d.slots * sizeof(JpegdState));
    d.cnt = (uint32_t*)p; p += align256(d.slots * 4);
    d.ibit = d.sub0 = d.maxsub = nullptr;
    if (g.ri) {
        const size_t table = align256((size_t)g.n * (jpegd_intervals(g) + 1u) * 4);
        d.ibit = (uint32_t*)p; p += table;
        d.sub0 = (uint32_t*)p; p += table;
        d.maxsub = (uint32_t*)p; p += align256((size_t)g.n * 4);
    }
    d.bytes = (size_t)(p - (uint8_t*)base);
    return d;
}

struct DArgs {
    const uint8_t* ecd;
    const uint64_t* off;
    const uint8_t* huffman;
    uint64_t ecd_cap;            // the segment bytes the workspace was sized for
    uint32_t sb;
    uint32_t K;                  // restart intervals of an image (1 without a restart interval)
    uint32_t extra;              // slot_extra
    JpegGeo g;
    int16_t* coef;
    uint32_t* status;
    uint32_t* rounds;
};

__device__ __forceinline__ size_t raw_start(uint64_t off, int img) { return (size_t)(off >> 2) + 2 * (size_t)img; }
__device__ __forceinline__ size_t slot_start(const DArgs& a, uint64_t off, int img) {
    return (size_t)(8 * off / a.sb) + (size_t)img * a.extra;
}

// ---- prepare ------------------------------------------------------------------------------------------------------------
template <bool RST>
__global__ void __launch_bounds__(SCAN_THREADS) jpegd_prepare_kernel(DArgs a, DLayout d) {
    const int img = blockIdx.x, tid = threadIdx.x;
    const uint64_t o0 = a.off[img], o1 = a.off[img + 1];
    uint32_t* ibit = RST ? d.ibit + (size_t)img * (a.K + 1u) : nullptr;
    uint32_t* sub0 = RST ? d.sub0 + (size_t)img * (a.K + 1u) : nullptr;
    if (o1 < o0 || o1 > a.ecd_cap || o1 - o0 > JPEGD_ECD_MAX) {               // uniform
        if (tid == 0) {
            atomicOr(a.status + img, JPEGD_ST_OFFSETS);
            d.total_bits[img] = 0; d.nsub[img] = 0;
        }
        return;
    }
    const int nt = 2 * a.g.nc;
    if (tid < nt && !jpegd_build_table(a.huffman + ((size_t)img * nt + tid) * JPEGD_DHT_BYTES, d.tabs + (size_t)img * nt + tid))
        atomicOr(a.status + img, JPEGD_ST_TABLE);
    jpegd_prepare_segment<RST>(a.ecd + o0, (uint32_t)(o1 - o0), (uint8_t*)(d.raw + raw_start(o0, img)), a.K, a.sb, ibit, sub0, a.status + img,
                               d.total_bits + img, d.nsub + img, RST ? d.maxsub + img : nullptr);
}

// ---- speculate / write: one thread per subsequence ------------------------------------------------------------------------
template <bool WRITE, bool RST>
__global__ void __launch_bounds__(DEC_THREADS) jpegd_decode_kernel(DArgs a, DLayout d) {
    __shared__ JpegdTable tabs[6];
    const int img = blockIdx.y;
    const uint32_t S = d.nsub[img];
    if (blockIdx.x * DEC_THREADS >= S) return;           // uniform
    jpegd_load_tables(tabs, d.tabs + (size_t)img * 2 * a.g.nc, 2 * a.g.nc, DEC_THREADS);
    const uint64_t o0 = a.off[img];
    const uint32_t nwords = ((uint32_t)(a.off[img + 1] - o0) + 3u) / 4u + 1u, total = d.total_bits[img];
    const uint32_t* bits = d.raw + raw_start(o0, img);
    JpegdState* ex = d.exit + slot_start(a, o0, img);
    uint32_t* cnt = d.cnt + slot_start(a, o0, img);
    const uint32_t* ibit = RST ? d.ibit + (size_t)img * (a.K + 1u) : nullptr;
    const uint32_t* sub0 = RST ? d.sub0 + (size_t)img * (a.K + 1u) : nullptr;
    int16_t* coef = a.coef + (size_t)img * a.g.NB * 64;
    int32_t* dcdiff = d.dcdiff + (size_t)img * a.g.SB;
    uint32_t status = 0;
    for (uint32_t i = blockIdx.x * DEC_THREADS + threadIdx.x; i < S; i += gridDim.x * DEC_THREADS) {
        JpegdState s;
        uint32_t begun;
        if (RST) {
            const JpegdSpan sp = jpegd_span(a.g, ibit, sub0, a.K, a.sb, i);
            if (WRITE && sp.j) s = ex[i - 1];
            else { s.p = sp.start; s.mz = 0; }
            // the first block begun here: the interval's first and the blocks begun in the interval before this subsequence
            const uint32_t block = WRITE ? sp.block_begin + (cnt[i] - cnt[sub0[sp.k]]) : 0u;
            jpegd_run_interval<WRITE>(bits, nwords, sp.end, sp.limit, tabs, a.g, s, begun, block, sp.block_begin, sp.block_end, coef,
                                      dcdiff, status);
        } else {
            if (WRITE && i) s = ex[i - 1];
            else { s.p = i * a.sb; s.mz = 0; }
            const uint32_t limit = min((i + 1u) * a.sb, total);
            jpegd_run<WRITE>(bits, nwords, total, limit, tabs, a.g, s, begun, WRITE ? cnt[i] : 0u, coef, dcdiff, status);
        }
        if (!WRITE) { ex[i] = s; cnt[i] = begun; }
    }
    if (WRITE && status) atomicOr(a.status + img, status);
}

// ---- synchronise and place: one workgroup per image -------------------------------------------------------------------------
template <bool RST>
__global__ void __launch_bounds__(SYNC_THREADS) jpegd_sync_kernel(DArgs a, DLayout d) {
    __shared__ JpegdTable tabs[6];
    __shared__ uint32_t wtot[SYNC_THREADS / 64];
    const int img = blockIdx.x, tid = threadIdx.x;
    const uint32_t S = d.nsub[img];
    if (S == 0) {
        if (tid == 0 && a.rounds) a.rounds[img] = 0;
        return;
    }
    jpegd_load_tables(tabs, d.tabs + (size_t)img * 2 * a.g.nc, 2 * a.g.nc, SYNC_THREADS);
    const uint64_t o0 = a.off[img];
    const uint32_t nwords = ((uint32_t)(a.off[img + 1] - o0) + 3u) / 4u + 1u, total = d.total_bits[img];
    const uint32_t* bits = d.raw + raw_start(o0, img);
    JpegdState* ex = d.exit + slot_start(a, o0, img);
    uint32_t* cnt = d.cnt + slot_start(a, o0, img);
    const uint32_t* ibit = RST ? d.ibit + (size_t)img * (a.K + 1u) : nullptr;
    const uint32_t* sub0 = RST ? d.sub0 + (size_t)img * (a.K + 1u) : nullptr;
    // without restart intervals (a separate instantiation for its instruction count) the scan is the one interval, and sp is not used
    const auto active = [&](uint32_t i, uint32_t r, JpegdSpan& sp) {
        if (!RST) return i >= r;
        sp = jpegd_span(a.g, ibit, sub0, a.K, a.sb, i);
        return sp.j >= r;
    };
    uint32_t unused = 0;                                   // the status of runs that do not write
    const auto run = [&](uint32_t i, const JpegdSpan& sp, JpegdState& s, uint32_t& begun) {
        if (RST) jpegd_run_interval<false>(bits, nwords, sp.end, sp.limit, tabs, a.g, s, begun, 0u, 0u, 0u, nullptr, nullptr, unused);
        else jpegd_run<false>(bits, nwords, total, min((i + 1u) * a.sb, total), tabs, a.g, s, begun, 0u, nullptr, nullptr, unused);
    };
    const uint32_t rounds = jpegd_sync_rounds<SYNC_THREADS>(S, RST ? d.maxsub[img] : S, ex, cnt, active, run);
    const uint32_t begun = jpegd_place_blocks<SYNC_THREADS>(S, cnt, wtot);
    // every interval must have begun its own blocks
    const bool few = RST ? jpegd_intervals_short(cnt, sub0, a.K, begun, (uint32_t)a.g.ri * (uint32_t)a.g.per, (uint32_t)a.g.SB, tid, SYNC_THREADS)
                         : tid == 0 && begun < (uint32_t)a.g.SB;
    if (few) atomicOr(a.status + img, JPEGD_ST_BLOCKS);
    if (tid == 0 && a.rounds) a.rounds[img] = rounds;
}

// ---- DC: one workgroup per (component, image) --------------------------------------------------------------------------------
// a sum that starts again where `first` is set: (a, then b) = b if b.first, else their sum - the prediction of a restart interval
struct DcSum {
    int v, first;
};
__device__ __forceinline__ DcSum operator+(const DcSum& a, const DcSum& b) { return b.first ? b : DcSum{a.v + b.v, a.first}; }
__device__ __forceinline__ DcSum lane_up(const DcSum& s, int o) { return DcSum{__shfl_up(s.v, o, 64), __shfl_up(s.first, o, 64)}; }
__device__ __forceinline__ DcSum wave_excl_of(const DcSum& incl, const DcSum&, int lane) {
    const DcSum u = lane_up(incl, 1);
    return lane ? u : DcSum{};
}
__device__ __forceinline__ int dc_value(int s) { return s; }
__device__ __forceinline__ int dc_value(const DcSum& s) { return s.v; }
template <typename T>
__device__ __forceinline__ T dc_item(int v, bool first);
template <>
__device__ __forceinline__ int dc_item<int>(int v, bool) { return v; }
template <>
__device__ __forceinline__ DcSum dc_item<DcSum>(int v, bool first) { return DcSum{v, first ? 1 : 0}; }

// T = int: one sum over the component; T = DcSum (a.g.ri > 0): one per restart interval
template <typename T>
__global__ void __launch_bounds__(SCAN_THREADS) jpegd_dc_kernel(DArgs a, DLayout d) {
    __shared__ T wtot[SCAN_THREADS / 64];
    const int comp = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
    if (d.nsub[img] == 0) return;
    const int ny = a.g.ny, mcus = a.g.SB / a.g.per, count = comp ? mcus : mcus * ny;
    const int span = a.g.ri ? (comp ? a.g.ri : a.g.ri * ny) : count;        // the component's blocks in one interval
    const int32_t* diff = d.dcdiff + (size_t)img * a.g.SB;
    int16_t* coef = a.coef + (size_t)img * a.g.NB * 64;
    T carry{};
    bool bad = false;
    for (int base = 0; base < count; base += SCAN_THREADS) {
        const int j = base + tid;
        const uint32_t b = jpegd_dc_block(ny, a.g.per, comp, j);
        const T v = dc_item<T>(j < count ? diff[b] : 0, j % span == 0);
        T sum;
        const int dc = dc_value(carry + block_excl_scan(v, wtot, sum) + v);
        carry = carry + sum;
        if (j < count) {
            int c2;
            const long at = jpegd_place(a.g, b, c2);
            if (dc < -32768 || dc > 32767) bad = true;
            if (at >= 0) coef[at * 64] = (int16_t)dc;
        }
    }
    if (bad) atomicOr(a.status + img, JPEGD_ST_DC);
}

// ---- the launchers, for files of three components (nc = 3) and of one (nc = 1, section 4p) ----------------------------------------
size_t decode_workspace_size(int n, int h, int w, int hs, int vs, int nc, int restart_interval, size_t ecd_bytes, int subseq_bits,
                             int factors = JPEG_FACTORS_THREE) {
    JpegGeo g;
    uint32_t sb;
    if (!make_geo(&g, n, h, w, hs, vs, nc, factors) || !set_restart(&g, restart_interval) || !jpegd_subseq_ok(subseq_bits, SUBSEQ_DEFAULT, &sb) ||
        ecd_bytes > (size_t)n * JPEGD_ECD_MAX)
        return 0;
    return carve_d(g, ecd_bytes, sb, nullptr).bytes;
}

int decode_launch(const uint8_t* ecd, const uint64_t* ecd_off, const uint8_t* huffman, int n, int h, int w, int hs, int vs, int nc,
                  int restart_interval, int subseq_bits, int16_t* coef, uint32_t* status, uint32_t* rounds, void* workspace,
                  size_t workspace_bytes, void* stream, int factors = JPEG_FACTORS_THREE) {
    JpegGeo g;
    uint32_t sb;
    if (!ecd || !ecd_off || !huffman || !coef || !status || !workspace || !make_geo(&g, n, h, w, hs, vs, nc, factors) ||
        !set_restart(&g, restart_interval) || !jpegd_subseq_ok(subseq_bits, SUBSEQ_DEFAULT, &sb))
        return NIMG_ERR_ARG;
    const auto bytes_for = [&](uint64_t ecd_bytes) { return carve_d(g, ecd_bytes, sb, workspace).bytes; };
    if (bytes_for(0) > workspace_bytes) return NIMG_ERR_WORKSPACE;
    const uint64_t lo = jpegd_ecd_capacity(bytes_for, (uint64_t)n * JPEGD_ECD_MAX, workspace_bytes);
    const DLayout d = carve_d(g, lo, sb, workspace);
    DArgs a;
    a.ecd = ecd; a.off = ecd_off; a.huffman = huffman; a.ecd_cap = lo; a.sb = sb; a.K = jpegd_intervals(g); a.extra = slot_extra(g); a.g = g;
    a.coef = coef; a.status = status; a.rounds = rounds;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, (size_t)n * 4, st) != hipSuccess || hipMemsetAsync(coef, 0, (size_t)n * g.NB * 128, st) != hipSuccess ||
        hipMemsetAsync(d.dcdiff, 0, (size_t)n * g.SB * 4, st) != hipSuccess || hipMemsetAsync(d.raw, 0, d.raw_words * 4, st) != hipSuccess)
        return NIMG_ERR_LAUNCH;
    const bool rst = g.ri != 0;
    if (rst) hipLaunchKernelGGL(jpegd_prepare_kernel<true>, dim3((unsigned)n), dim3(SCAN_THREADS), 0, st, a, d);
    else hipLaunchKernelGGL(jpegd_prepare_kernel<false>, dim3((unsigned)n), dim3(SCAN_THREADS), 0, st, a, d);
    NIMG_CHECK_LAUNCH();
    // no valid stream is longer than SB blocks of JPEGD_BLOCK_BITS_MAX bits; a longer (damaged) one is covered by the threads' stride
    const uint64_t bits_max = min((uint64_t)g.SB * JPEGD_BLOCK_BITS_MAX, 8 * min(lo, JPEGD_ECD_MAX));
    const uint64_t subs_max = bits_max / sb + (rst ? a.K : 0u);
    const unsigned gx = (unsigned)min((uint64_t)4096, max((uint64_t)1, (subs_max + DEC_THREADS) / DEC_THREADS));
    if (rst) hipLaunchKernelGGL((jpegd_decode_kernel<false, true>), dim3(gx, (unsigned)n), dim3(DEC_THREADS), 0, st, a, d);
    else hipLaunchKernelGGL((jpegd_decode_kernel<false, false>), dim3(gx, (unsigned)n), dim3(DEC_THREADS), 0, st, a, d);
    NIMG_CHECK_LAUNCH();
    if (rst) hipLaunchKernelGGL(jpegd_sync_kernel<true>, dim3((unsigned)n), dim3(SYNC_THREADS), 0, st, a, d);
    else hipLaunchKernelGGL(jpegd_sync_kernel<false>, dim3((unsigned)n), dim3(SYNC_THREADS), 0, st, a, d);
    NIMG_CHECK_LAUNCH();
    if (rst) hipLaunchKernelGGL((jpegd_decode_kernel<true, true>), dim3(gx, (unsigned)n), dim3(DEC_THREADS), 0, st, a, d);
    else hipLaunchKernelGGL((jpegd_decode_kernel<true, false>), dim3(gx, (unsigned)n), dim3(DEC_THREADS), 0, st, a, d);
    NIMG_CHECK_LAUNCH();
    if (rst) hipLaunchKernelGGL(jpegd_dc_kernel<DcSum>, dim3((unsigned)nc, (unsigned)n), dim3(SCAN_THREADS), 0, st, a, d);
    else hipLaunchKernelGGL(jpegd_dc_kernel<int>, dim3((unsigned)nc, (unsigned)n), dim3(SCAN_THREADS), 0, st, a, d);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

}  // namespace

// declared in jpegc.h: jpegd_scaled.hip calls it for scale 1
int nimg_internal_jpeg_reconstruct_tables(const int16_t* coef, int n, int h, int w, int hs, int vs, int nc, const uint16_t* qtabs, void* y,
                                          int out_u8, void* workspace, size_t workspace_bytes, void* stream, int factors) {
    JpegGeo g;
    if (!coef || !y || !qtabs || !workspace || !make_geo(&g, n, h, w, hs, vs, nc, factors)) return NIMG_ERR_ARG;
    const Workspace ws = carve(g, workspace);
    if (workspace_bytes < ws.bytes) return NIMG_ERR_WORKSPACE;
    const long blocks = (long)n * g.NB, pixels = (long)n * h * w;
    if (!grid_ok(blocks, 256) || !grid_ok(pixels, 256)) return NIMG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_idct_kernel<FileTables>, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, st, coef, ws.planes, g,
                       FileTables{qtabs});
    NIMG_CHECK_LAUNCH();
    return nimg_internal_jpeg_colour(ws.planes, y, out_u8 != 0, g, st);
}

extern "C" {

size_t nimg_jpeg_decode_restart_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval, size_t ecd_bytes,
                                                int subseq_bits) {
    return decode_workspace_size(n, h, w, hs, vs, 3, restart_interval, ecd_bytes, subseq_bits);
}

size_t nimg_jpeg_decode_workspace_bytes(int n, int h, int w, int hs, int vs, size_t ecd_bytes, int subseq_bits) {
    return decode_workspace_size(n, h, w, hs, vs, 3, 0, ecd_bytes, subseq_bits);
}

int nimg_jpeg_decode_restart(const uint8_t* ecd, const uint64_t* ecd_off, const uint8_t* huffman, int n, int h, int w, int hs, int vs,
                             int restart_interval, int subseq_bits, int16_t* coef, uint32_t* status, uint32_t* rounds, void* workspace,
                             size_t workspace_bytes, void* stream) {
    return decode_launch(ecd, ecd_off, huffman, n, h, w, hs, vs, 3, restart_interval, subseq_bits, coef, status, rounds, workspace,
                         workspace_bytes, stream);
}

size_t nimg_jpeg_grey_decode_workspace_bytes(int n, int h, int w, int restart_interval, size_t ecd_bytes, int subseq_bits) {
    return decode_workspace_size(n, h, w, 1, 1, 1, restart_interval, ecd_bytes, subseq_bits);
}

int nimg_jpeg_grey_decode(const uint8_t* ecd, const uint64_t* ecd_off, const uint8_t* huffman, int n, int h, int w, int restart_interval,
                          int subseq_bits, int16_t* coef, uint32_t* status, uint32_t* rounds, void* workspace, size_t workspace_bytes,
                          void* stream) {
    if (n == 0) return NIMG_OK;
    return decode_launch(ecd, ecd_off, huffman, n, h, w, 1, 1, 1, restart_interval, subseq_bits, coef, status, rounds, workspace,
                         workspace_bytes, stream);
}

int nimg_jpeg_grey_reconstruct_tables(const int16_t* coef, int n, int h, int w, const uint16_t* qtabs, void* y, int out_u8, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    if (n == 0) return NIMG_OK;
    return nimg_internal_jpeg_reconstruct_tables(coef, n, h, w, 1, 1, 1, qtabs, y, out_u8, workspace, workspace_bytes, stream);
}

int nimg_jpeg_decode(const uint8_t* ecd, const uint64_t* ecd_off, const uint8_t* huffman, int n, int h, int w, int hs, int vs,
                     int subseq_bits, int16_t* coef, uint32_t* status, uint32_t* rounds, void* workspace, size_t workspace_bytes,
                     void* stream) {
    return nimg_jpeg_decode_restart(ecd, ecd_off, huffman, n, h, w, hs, vs, 0, subseq_bits, coef, status, rounds, workspace,
                                    workspace_bytes, stream);
}

int nimg_jpeg_reconstruct_tables(const int16_t* coef, int n, int h, int w, int hs, int vs, const uint16_t* qtabs, void* y, int out_u8,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    return nimg_internal_jpeg_reconstruct_tables(coef, n, h, w, hs, vs, 3, qtabs, y, out_u8, workspace, workspace_bytes, stream);
}

// ---- the same launchers with the wide set of sampling factors -----------------------------------------------
size_t nimg_jpeg_sampling_decode_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval, size_t ecd_bytes,
                                                 int subseq_bits) {
    return decode_workspace_size(n, h, w, hs, vs, 3, restart_interval, ecd_bytes, subseq_bits, JPEG_FACTORS_WIDE);
}

int nimg_jpeg_sampling_decode(const uint8_t* ecd, const uint64_t* ecd_off, const uint8_t* huffman, int n, int h, int w, int hs, int vs,
                              int restart_interval, int subseq_bits, int16_t* coef, uint32_t* status, uint32_t* rounds, void* workspace,
                              size_t workspace_bytes, void* stream) {
    return decode_launch(ecd, ecd_off, huffman, n, h, w, hs, vs, 3, restart_interval, subseq_bits, coef, status, rounds, workspace,
                         workspace_bytes, stream, JPEG_FACTORS_WIDE);
}

int nimg_jpeg_sampling_reconstruct_tables(const int16_t* coef, int n, int h, int w, int hs, int vs, const uint16_t* qtabs, void* y,
                                          int out_u8, void* workspace, size_t workspace_bytes, void* stream) {
    return nimg_internal_jpeg_reconstruct_tables(coef, n, h, w, hs, vs, 3, qtabs, y, out_u8, workspace, workspace_bytes, stream,
                                                 JPEG_FACTORS_WIDE);
}

}  // extern "C"
