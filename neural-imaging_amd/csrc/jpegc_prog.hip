// Writing progressive JPEG files (libjpeg's jpeg_simple_progression): the ten scans of one set of quantised
// coefficients, each coded with a Huffman table made for it.  The block walks, the scan script and the run resolution are
// csrc/jpegprog.h's, which tests/jpegprog_host.cpp runs on the host; the bit sink and the scans over a workgroup are jpegc.h's.
//   pass<HIST>    one workgroup per (image, scan), 256 blocks of the scan at a time, one thread per block: the block's symbols into
//                 the scan's histogram in LDS - or its bit length with the image's tables - and its summary word into LDS; thread 0
//                 then walks the 256 summaries (never a coefficient) and resolves the end-of-band runs, whose forced ends at 0x7fff
//                 blocks and at more than 937 waiting correction bits make them depend on what came before.  A run's EOBn symbol is
//                 counted - or its bits added to the length of the run's first block, and the run's length stored for the emitter.
//   emit          one thread per (image, scan, block): the walk again behind the bit sink, the EOBn symbol of the run that starts
//                 with the block, the correction bits it leaves, the padding in front of a restart marker and at the end of the scan.
//   layout/gather the segments of the three scan classes (jpegc.hip's count, scan and stuff passes run once per class: the scans of
//                 a class share a block grid) -> the ten segments of each image back to back, lengths[n][10].
// A scan of an image is a segment of its own to jpegc.hip's hidden launchers: they see a class as a batch of n * 2 or n * 4 images
// whose MCUs are the blocks of the scan (jpegprog_class_geo).
#include "jpegc.h"
#include "jpegprog.h"

namespace {

struct ProgClass {
    JpegGeo g;                         // jpegprog_class_geo
    uint32_t* off;                     // [segments][g.SB] bit lengths, then offsets
    uint32_t* run;                     // [segments][g.SB] AC classes: the length of the run that starts with the block, else 0
    uint32_t* total;                   // [segments]
    unsigned long long* dst;           // [segments]
    uint32_t* raw;                     // [segments][raw_words]
    unsigned raw_words;
    uint32_t* lengths;                 // [segments] stuffed bytes
    uint8_t* bytes;                    // the stuffed segments of the class back to back
    size_t bytes_capacity;
};

struct ProgWorkspace {
    uint32_t* codes;                   // [n][JPEGPROG_CODE_WORDS]
    unsigned long long* base;          // [n] first byte of an image in `out`
    ProgClass c[3];
    size_t bytes;
};

inline bool prog_geo(JpegGeo* g, int n, int h, int w, int hs, int vs, int restart_interval) {
    if (n > 16383 || !make_geo(g, n, h, w, hs, vs) || !set_restart(g, restart_interval)) return false;     // 4 n segments are a grid's y
    return (long)n * 4 * g->SB < 0x7fffffffL;                      // no class has more blocks than 4 n scans of SB
}

inline ProgWorkspace prog_carve(const JpegGeo& g, void* base) {
    ProgWorkspace ws{};
    uint8_t* p = (uint8_t*)base;
    ws.codes = (uint32_t*)p; p += align256((size_t)g.n * JPEGPROG_CODE_WORDS * 4);
    ws.base = (unsigned long long*)p; p += align256((size_t)g.n * 8);
    for (int k = 0; k < 3; ++k) {
        ProgClass& c = ws.c[k];
        c.g = jpegprog_class_geo(g, k);
        const size_t seg = (size_t)c.g.n;
        c.raw_words = jpegprog_raw_words(c.g, k);
        c.off = (uint32_t*)p; p += align256(seg * c.g.SB * 4);
        c.run = (uint32_t*)p; p += k ? align256(seg * c.g.SB * 4) : 0;
        c.total = (uint32_t*)p; p += align256(seg * 4);
        c.dst = (unsigned long long*)p; p += align256(seg * 8);
        c.lengths = (uint32_t*)p; p += align256(seg * 4);
        c.raw = (uint32_t*)p; p += align256(seg * c.raw_words * 4);
        c.bytes_capacity = seg * c.raw_words * 8;          // every byte stuffed
        c.bytes = p; p += align256(c.bytes_capacity);
    }
    ws.bytes = (size_t)(p - (uint8_t*)base);
    return ws;
}

// what the kernels need of the three classes
struct ProgView {
    JpegGeo g[3];
    uint32_t* off[3];
    uint32_t* run[3];
    uint32_t* raw[3];
    unsigned raw_words[3];
};

inline ProgView prog_view(const ProgWorkspace& ws) {
    ProgView v{};
    for (int k = 0; k < 3; ++k) {
        v.g[k] = ws.c[k].g; v.off[k] = ws.c[k].off; v.run[k] = ws.c[k].run; v.raw[k] = ws.c[k].raw; v.raw_words[k] = ws.c[k].raw_words;
    }
    return v;
}

// ---- sinks ------------------------------------------------------------------------------------------------------------------
struct ProgHistSink {
    uint32_t* hist;                    // LDS: the scan's table, or the two DC tables
    int first;                         // the table hist[0] belongs to
    __device__ __forceinline__ void symbol(int table, int sym, uint32_t, int) { atomicAdd(hist + (table - first) * JPEGOPT_HIST + sym, 1u); }
    __device__ __forceinline__ void raw(uint64_t, int) {}
};

// jpegc.h's bit sink behind the code words of one scan; a symbol without a code puts nothing and sets `missing`
template <bool EMIT>
struct ProgCodeSink : BitSink<EMIT> {
    const uint32_t* codes;             // LDS: the scan's table [256], or the two DC tables [2][16]
    int first;
    bool missing = false;
    __device__ __forceinline__ void symbol(int table, int sym, uint32_t value, int nbits) {
        const uint32_t e = codes[(table - first) * 16 + sym];
        if (e == 0) { missing = true; return; }
        this->put(((e >> 5) << nbits) | value, (int)(e & 31u) + nbits);
    }
    __device__ __forceinline__ void raw(uint64_t bits, int nbits) {
        while (nbits > 16) {
            nbits -= 16;
            this->put((uint32_t)(bits >> nbits) & 0xffffu, 16);
        }
        if (nbits > 0) this->put((uint32_t)bits & ((1u << nbits) - 1u), nbits);
    }
};

// the code words of scan sc of image img -> LDS (the DC first scan: both DC tables; the DC refine scan: none)
__device__ __forceinline__ void prog_load_codes(uint32_t* s_codes, const uint32_t* __restrict__ codes, int img, const JpegProgScan& sc) {
    const int count = sc.table < 0 ? 0 : (sc.table == 0 ? 32 : 256);
    const uint32_t* src = codes + (size_t)img * JPEGPROG_CODE_WORDS + jpegprog_code_base(sc.table < 0 ? 0 : sc.table);
    for (int i = threadIdx.x; i < count; i += 256) s_codes[i] = src[i];
    __syncthreads();
}

// ---- histogram / bit length and the runs ------------------------------------------------------------------------------------------
// what thread 0 does with a resolved run
struct ProgHistRec {
    uint32_t* hist;
    __device__ __forceinline__ void run(int, int length) { atomicAdd(hist + (jpegprog_run_category(length) << 4), 1u); }
};
struct ProgLenRec {
    const uint32_t* codes;             // LDS, the scan's table
    uint32_t *len, *runs;              // the scan's rows
    bool missing;
    __device__ __forceinline__ void run(int first, int length) {
        const int n = jpegprog_run_category(length);
        const uint32_t e = codes[n << 4];
        if (e == 0) { missing = true; return; }           // the emitter leaves the symbol and its run bits out as well
        len[first] += (e & 31u) + (uint32_t)n;
        runs[first] = (uint32_t)length;
    }
};

// grid (10, n).  HIST: hist[image][table][257] += (zeroed by the caller).  Otherwise off / run of the view and status |=; an image whose
// tables were refused gets length 0 for every block.
template <bool HIST>
__global__ void __launch_bounds__(256) jpeg_prog_pass_kernel(const int16_t* __restrict__ coef, uint32_t* __restrict__ hist,
                                                             const uint32_t* __restrict__ codes, uint32_t* __restrict__ status, JpegGeo g,
                                                             ProgView v) {
    __shared__ uint32_t s_tab[HIST ? 2 * JPEGOPT_HIST : 256];
    __shared__ uint32_t s_sum[256];
    const int scan = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
    const JpegProgScan sc = jpegprog_scan(scan);
    const int16_t* ci = coef + (long)img * g.NB * 64;
    const int nblk = jpegprog_class_blocks(g, sc.cls), first = sc.table < 0 ? 0 : sc.table;
    bool refused = false;
    if (HIST) {
        for (int i = tid; i < 2 * JPEGOPT_HIST; i += 256) s_tab[i] = 0;
        __syncthreads();
    } else {
        prog_load_codes(s_tab, codes, img, sc);
        refused = (status[img] & JPEGOPT_ST_TABLE) != 0;           // written by the derive pass, before this kernel began
    }
    const size_t row = ((size_t)img * jpegprog_class_scans(sc.cls) + sc.idx) * nblk;
    uint32_t* len = HIST ? nullptr : v.off[sc.cls] + row;
    uint32_t* runs = HIST || sc.cls == 0 ? nullptr : v.run[sc.cls] + row;
    JpegProgRun state;                                              // thread 0's
    bool missing = false;
    for (int b0 = 0; b0 < nblk; b0 += 256) {
        const int b = b0 + tid;
        uint32_t sum = 0;
        if (b < nblk && !refused) {
            if (HIST) {
                ProgHistSink sink{s_tab, first};
                if (sc.cls == 0) jpegprog_walk_dc(ci, g, b, sc.ah != 0, sc.al, sink);
                else sum = jpegprog_walk_ac(ci, g, sc, b, sink).summary;
            } else {
                ProgCodeSink<false> sink;
                sink.codes = s_tab;
                sink.first = first;
                sink.init(nullptr, 0, 0);
                if (sc.cls == 0) jpegprog_walk_dc(ci, g, b, sc.ah != 0, sc.al, sink);
                else sum = jpegprog_walk_ac(ci, g, sc, b, sink).summary;
                len[b] = sink.count + ((sum & JPEGPROG_SUM_RUN) ? sum >> JPEGPROG_SUM_BITS_SHIFT : 0u);
                if (runs) runs[b] = 0;
                missing |= sink.missing;
            }
        } else if (b < nblk && !HIST) {
            len[b] = 0;
            if (runs) runs[b] = 0;
        }
        if (sc.cls == 0) continue;                                  // a DC scan has no runs (uniform: no barrier is skipped by some)
        s_sum[tid] = sum;
        __syncthreads();                                            // the summaries, and the lengths in memory, are the workgroup's
        if (tid == 0 && !refused) {
            const int cnt = min(256, nblk - b0);
            if (HIST) {
                ProgHistRec rec{s_tab};
                for (int j = 0; j < cnt; ++j) jpegprog_run_block(state, b0 + j, g.ri, s_sum[j], rec);
                if (b0 + cnt == nblk) jpegprog_run_end(state, rec);
            } else {
                ProgLenRec rec{s_tab, len, runs, false};
                for (int j = 0; j < cnt; ++j) jpegprog_run_block(state, b0 + j, g.ri, s_sum[j], rec);
                if (b0 + cnt == nblk) jpegprog_run_end(state, rec);
                missing |= rec.missing;
            }
        }
        __syncthreads();
    }
    if (HIST) {
        __syncthreads();
        const int tables = sc.table < 0 ? 0 : (sc.table == 0 ? 2 : 1);
        uint32_t* dst = hist + ((size_t)img * JPEGPROG_TABLES + first) * JPEGOPT_HIST;
        for (int i = tid; i < tables * JPEGOPT_HIST; i += 256) {
            const uint32_t c = s_tab[i];
            if (c) atomicAdd(dst + i, c);
        }
    } else if (missing) {
        atomicOr(status + img, JPEGOPT_ST_SYMBOL);
    }
}

// one thread per image: status[image] = JPEGOPT_ST_TABLE or 0 (the call's only plain store to it)
__global__ void __launch_bounds__(64) jpeg_prog_derive_kernel(const uint8_t* __restrict__ tables, uint32_t* __restrict__ codes,
                                                              uint32_t* __restrict__ status, int n) {
    const int img = blockIdx.x * 64 + threadIdx.x;
    if (img >= n) return;
    const bool ok = jpegprog_derive_image(tables + (size_t)img * JPEGPROG_TABLES * JPEGOPT_TABLE_BYTES, codes + (size_t)img * JPEGPROG_CODE_WORDS);
    status[img] = ok ? 0u : JPEGOPT_ST_TABLE;
}

// ---- emit -------------------------------------------------------------------------------------------------------------------
// grid (ceil(g.SB / 256), 10, n): g.SB is the largest block count of a scan
__global__ void __launch_bounds__(256) jpeg_prog_emit_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ codes,
                                                             const uint32_t* __restrict__ status, JpegGeo g, ProgView v) {
    __shared__ uint32_t s_codes[256];
    const int scan = blockIdx.y, img = blockIdx.z, b = blockIdx.x * 256 + threadIdx.x;
    const JpegProgScan sc = jpegprog_scan(scan);
    const int nblk = jpegprog_class_blocks(g, sc.cls);
    if (blockIdx.x * 256 >= nblk) return;                           // the whole workgroup
    prog_load_codes(s_codes, codes, img, sc);
    if (b >= nblk || (status[img] & JPEGOPT_ST_TABLE) != 0) return;
    const size_t seg = (size_t)img * jpegprog_class_scans(sc.cls) + sc.idx;
    const uint32_t begin = v.off[sc.cls][seg * nblk + b];
    const unsigned raw_words = v.raw_words[sc.cls];
    ProgCodeSink<true> sink;
    sink.codes = s_codes;
    sink.first = sc.table < 0 ? 0 : sc.table;
    sink.init(v.raw[sc.cls] + seg * raw_words, raw_words, begin);
    const int16_t* ci = coef + (long)img * g.NB * 64;
    if (sc.cls == 0) {
        jpegprog_walk_dc(ci, g, b, sc.ah != 0, sc.al, sink);
    } else {
        const JpegProgTail tail = jpegprog_walk_ac(ci, g, sc, b, sink);
        jpegprog_block_end(tail, sc.table, (int)v.run[sc.cls][seg * nblk + b], sink);
    }
    pad_interval(sink, v.g[sc.cls], b, begin);
    sink.finish();
}

// ---- the segments of the classes -> the caller's order --------------------------------------------------------------------------------
struct ProgSegments {
    const uint32_t* lengths[3];
    const unsigned long long* dst[3];
    const uint8_t* bytes[3];
};

// one workgroup: base[image] = the bytes of the images before it, lengths[image][scan]
__global__ void __launch_bounds__(SCAN_THREADS) jpeg_prog_layout_kernel(ProgSegments s, uint32_t* __restrict__ lengths,
                                                                        unsigned long long* __restrict__ base, int n) {
    __shared__ unsigned long long wtot[SCAN_THREADS / 64];
    const int per = (n + SCAN_THREADS - 1) / SCAN_THREADS, j0 = min(n, (int)threadIdx.x * per), j1 = min(n, j0 + per);
    unsigned long long loc = 0, sum;
    for (int j = j0; j < j1; ++j)
        for (int scan = 0; scan < JPEGPROG_SCANS; ++scan) {
            const JpegProgScan sc = jpegprog_scan(scan);
            const uint32_t l = s.lengths[sc.cls][(size_t)j * jpegprog_class_scans(sc.cls) + sc.idx];
            lengths[(size_t)j * JPEGPROG_SCANS + scan] = l;
            loc += l;
        }
    unsigned long long at = block_excl_scan(loc, wtot, sum);
    for (int j = j0; j < j1; ++j) {
        base[j] = at;
        for (int scan = 0; scan < JPEGPROG_SCANS; ++scan) at += lengths[(size_t)j * JPEGPROG_SCANS + scan];
    }
}

// grid (8, 10, n): the bytes of one segment to where the caller wants them, none at or beyond capacity
__global__ void __launch_bounds__(256) jpeg_prog_gather_kernel(ProgSegments s, const uint32_t* __restrict__ lengths,
                                                               const unsigned long long* __restrict__ base, uint8_t* __restrict__ out,
                                                               unsigned long long capacity) {
    const int scan = blockIdx.y, img = blockIdx.z;
    const JpegProgScan sc = jpegprog_scan(scan);
    const size_t seg = (size_t)img * jpegprog_class_scans(sc.cls) + sc.idx;
    unsigned long long at = base[img];
    for (int k = 0; k < scan; ++k) at += lengths[(size_t)img * JPEGPROG_SCANS + k];
    const uint32_t count = lengths[(size_t)img * JPEGPROG_SCANS + scan];
    const uint8_t* src = s.bytes[sc.cls] + s.dst[sc.cls][seg];
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256)
        if (at + i < capacity) out[at + i] = src[i];
}

}  // namespace

extern "C" {

size_t nimg_jpeg_progressive_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval) {
    JpegGeo g;
    if (!prog_geo(&g, n, h, w, hs, vs, restart_interval)) return 0;
    return prog_carve(g, nullptr).bytes;
}

int nimg_jpeg_progressive_histogram(const int16_t* coef, int n, int h, int w, int hs, int vs, int restart_interval, uint32_t* hist,
                                    void* stream) {
    if (n == 0) return NIMG_OK;
    JpegGeo g;
    if (!coef || !hist || !prog_geo(&g, n, h, w, hs, vs, restart_interval)) return NIMG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (size_t)n * JPEGPROG_TABLES * JPEGOPT_HIST * 4, st) != hipSuccess) return NIMG_ERR_LAUNCH;
    hipLaunchKernelGGL(jpeg_prog_pass_kernel<true>, dim3(JPEGPROG_SCANS, (unsigned)n), dim3(256), 0, st, coef, hist, (const uint32_t*)nullptr,
                       (uint32_t*)nullptr, g, ProgView{});
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_jpeg_encode_progressive(const int16_t* coef, int n, int h, int w, int hs, int vs, int restart_interval, const uint8_t* tables,
                                 uint8_t* out, size_t out_capacity, uint32_t* lengths, uint32_t* status, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (n == 0) return NIMG_OK;
    JpegGeo g;
    if (!coef || !tables || !out || !lengths || !status || !workspace || !prog_geo(&g, n, h, w, hs, vs, restart_interval)) return NIMG_ERR_ARG;
    const ProgWorkspace ws = prog_carve(g, workspace);
    if (workspace_bytes < ws.bytes) return NIMG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const ProgView v = prog_view(ws);
    hipLaunchKernelGGL(jpeg_prog_derive_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, tables, ws.codes, status, n);
    NIMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_prog_pass_kernel<false>, dim3(JPEGPROG_SCANS, (unsigned)n), dim3(256), 0, st, coef, (uint32_t*)nullptr,
                       (const uint32_t*)ws.codes, status, g, v);
    NIMG_CHECK_LAUNCH();
    for (int k = 0; k < 3; ++k) {
        const ProgClass& c = ws.c[k];
        const int rc = nimg_internal_jpeg_offsets(c.off, c.total, c.raw, c.g, c.raw_words, st);
        if (rc != NIMG_OK) return rc;
    }
    hipLaunchKernelGGL(jpeg_prog_emit_kernel, dim3((unsigned)((g.SB + 255) / 256), JPEGPROG_SCANS, (unsigned)n), dim3(256), 0, st, coef,
                       (const uint32_t*)ws.codes, (const uint32_t*)status, g, v);
    NIMG_CHECK_LAUNCH();
    ProgSegments s{};
    for (int k = 0; k < 3; ++k) {
        const ProgClass& c = ws.c[k];
        const int rc = nimg_internal_jpeg_pack(c.raw, c.total, c.off, c.lengths, c.dst, c.bytes, c.bytes_capacity, c.g, c.raw_words, st);
        if (rc != NIMG_OK) return rc;
        s.lengths[k] = c.lengths; s.dst[k] = c.dst; s.bytes[k] = c.bytes;
    }
    hipLaunchKernelGGL(jpeg_prog_layout_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, s, lengths, ws.base, n);
    NIMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_prog_gather_kernel, dim3(8, JPEGPROG_SCANS, (unsigned)n), dim3(256), 0, st, s, (const uint32_t*)lengths,
                       (const unsigned long long*)ws.base, out, (unsigned long long)out_capacity);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

}  // extern "C"
