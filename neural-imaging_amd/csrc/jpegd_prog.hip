// Decoder of progressive JPEG files: the entropy-coded segments of every scan of a batch -> the coefficient
// tensor of jpegc.hip.  The scans of a script are ordered in levels (jpegdprog.h): a scan reads only what scans of lower levels wrote,
// the scans of one level write disjoint int16 elements and run side by side.
//   prepare    one workgroup per (image, scan): the scan's Huffman tables; the segment without its stuffing and restart markers and
//              the bit every restart interval begins at (jpegd_prepare.h, the baseline decoder's un-stuffing)
//   first      DC and AC first scans of a level, one workgroup per (image, scan): speculate, synchronise, place and write as section
//              4e orders them, all four inside the workgroup, the rounds and the placement by jpegd_sync.h - the baseline decoder's
//              code; then, in a DC scan, the sums of the differences per component and restart interval
//   dc refine  one thread per block: its bit is at a known place
//   ac refine  one wave per (image, scan, restart interval), its blocks in order: which bits a block consumes depends on which of its
//              coefficients are non-zero already, so nothing can be decoded ahead of its block.  The lanes hold the block's 64
//              coefficients and share out the walk inside it
// A call launches prepare once and then, per level, one kernel per kind of scan the level holds: the number of launches depends on the
// script alone.  The sequential core is jpegdprog.h, shared with a host program (tests/jpegdprog_host.cpp).
#include "jpegc.h"
#include "jpegd.h"
#include "jpegd_prepare.h"
#include "jpegd_sync.h"
#include "jpegdprog.h"

namespace {

constexpr int FIRST_THREADS = 256;
constexpr int REFINE_THREADS = 256;
constexpr uint32_t PROG_SUBSEQ_DEFAULT = 512;         // the fastest setting measured

struct PScript {
    int n_scans;
    JpegdProgScan sc[JPEGDPROG_SCANS_MAX];
};

// segment q = image * n_scans + scan
struct PLayout {
    uint32_t* total_bits;        // [nq] bits of a segment's un-stuffed stream
    uint32_t* nsub;              // [nq] its subsequences (0: bad offsets, the scan is not decoded)
    uint32_t* maxsub;            // [nq] the subsequences of its longest restart interval
    JpegdTable* tabs;            // [nq][3]
    int32_t* dcdiff;             // [n][SB] DC differences (jpegdprog_dc_slot), then their running sums
    uint32_t* raw;               // un-stuffed streams; segment q from word (ecd_off[q] >> 2) + 2 q, (len + 3) / 4 + 1 words
    JpegdState* exit;            // exit states; segment q from slot 8 ecd_off[q] / subseq_bits + q * extra
    uint32_t* cnt;               // blocks completed, then (in place) the index of the first block completed; slots as `exit`
    uint32_t* ibit;              // [nq][Kmax + 1] the bit every restart interval begins at
    uint32_t* sub0;              // [nq][Kmax + 1] the first subsequence of every interval
    size_t raw_words, slots, bytes;
};

// the most restart intervals a scan of the frame has: those of the luma scans, an interval of which is ri blocks
inline uint32_t intervals_max(const JpegGeo& g) { return g.ri ? (uint32_t)((g.nbY + g.ri - 1) / g.ri) : 1u; }

PLayout carve_p(const JpegGeo& g, int n_scans, uint64_t ecd_bytes, uint32_t sb, void* base) {
    PLayout d;
    const size_t nq = (size_t)g.n * n_scans, table = align256(nq * (intervals_max(g) + 1u) * 4);
    uint8_t* p = (uint8_t*)base;
    d.total_bits = (uint32_t*)p; p += align256(nq * 4);
    d.nsub = (uint32_t*)p; p += align256(nq * 4);
    d.maxsub = (uint32_t*)p; p += align256(nq * 4);
    d.tabs = (JpegdTable*)p; p += align256(nq * 3 * sizeof(JpegdTable));
    d.dcdiff = (int32_t*)p; p += align256((size_t)g.n * g.SB * 4);
    d.raw_words = (size_t)(ecd_bytes / 4) + 2 * nq + 2;
    d.raw = (uint32_t*)p; p += align256(d.raw_words * 4);
    d.slots = (size_t)(8 * ecd_bytes / sb) + nq * (intervals_max(g) + 1u) + 1;
    d.exit = (JpegdState*)p; p += align256(d.slots * sizeof(JpegdState));
    d.cnt = (uint32_t*)p; p += align256(d.slots * 4);
    d.ibit = (uint32_t*)p; p += table;
    d.sub0 = (uint32_t*)p; p += table;
    d.bytes = (size_t)(p - (uint8_t*)base);
    return d;
}

struct PArgs {
    const uint8_t* ecd;
    const uint64_t* off;
    const uint8_t* huffman;
    uint64_t ecd_cap;            // the segment bytes the workspace was sized for
    uint32_t sb;
    uint32_t Kmax;               // intervals_max
    JpegGeo g;
    int16_t* coef;
    uint32_t* status;
    uint32_t* rounds;
    PScript script;
};

// what every kernel needs of segment q
struct PSeg {
    const uint32_t* bits;
    uint32_t nwords;
    uint32_t* ibit;
    uint32_t* sub0;
    size_t slot;
};
__device__ __forceinline__ PSeg segment(const PArgs& a, const PLayout& d, size_t q) {
    const uint64_t o0 = a.off[q];
    PSeg s;
    s.bits = d.raw + (size_t)(o0 >> 2) + 2 * q;
    s.nwords = ((uint32_t)(a.off[q + 1] - o0) + 3u) / 4u + 1u;
    s.ibit = d.ibit + q * (a.Kmax + 1u);
    s.sub0 = d.sub0 + q * (a.Kmax + 1u);
    s.slot = (size_t)(8 * o0 / a.sb) + q * (a.Kmax + 1u);
    return s;
}

// ---- prepare: one workgroup per (image, scan) -----------------------------------------------------------------------------------
template <bool RST>
__global__ void __launch_bounds__(SCAN_THREADS) jpegd_prog_prepare_kernel(PArgs a, PLayout d) {
    const int scan = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
    const size_t q = (size_t)img * a.script.n_scans + scan;
    const uint64_t o0 = a.off[q], o1 = a.off[q + 1];
    if (tid == 0) a.rounds[q] = 0;
    if (o1 < o0 || o1 > a.ecd_cap || o1 - o0 > JPEGD_ECD_MAX) {          // uniform
        if (tid == 0) {
            atomicOr(a.status + img, JPEGD_ST_OFFSETS);
            d.total_bits[q] = 0; d.nsub[q] = 0; d.maxsub[q] = 0;
        }
        return;
    }
    if (tid < 3 && !jpegd_build_table(a.huffman + (q * 3 + tid) * JPEGD_DHT_BYTES, d.tabs + q * 3 + tid)) atomicOr(a.status + img, JPEGD_ST_TABLE);
    const JpegGeo cg = jpegdprog_geo(a.g, a.script.sc[scan]);
    uint32_t* ibit = d.ibit + q * (a.Kmax + 1u);
    uint32_t* sub0 = d.sub0 + q * (a.Kmax + 1u);
    jpegd_prepare_segment<RST>(a.ecd + o0, (uint32_t)(o1 - o0), (uint8_t*)(d.raw + (size_t)(o0 >> 2) + 2 * q), jpegd_intervals(cg), a.sb, ibit,
                               sub0, a.status + img, d.total_bits + q, d.nsub + q, d.maxsub + q);
    if (!RST && tid == 0) {                              // one interval: the tables every other kernel reads
        ibit[0] = 0; ibit[1] = d.total_bits[q];
        sub0[0] = 0; sub0[1] = d.nsub[q];
        d.maxsub[q] = d.nsub[q];
    }
}

// ---- first scans of a level: one workgroup per (image, scan) ---------------------------------------------------------------------
__global__ void __launch_bounds__(FIRST_THREADS) jpegd_prog_first_kernel(PArgs a, PLayout d, int level) {
    __shared__ JpegdTable tabs[3];
    __shared__ uint32_t wtot[FIRST_THREADS / 64];
    const int scan = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
    const JpegdProgScan sc = a.script.sc[scan];
    if (sc.level != level || !jpegdprog_first(sc)) return;              // uniform
    const size_t q = (size_t)img * a.script.n_scans + scan;
    const uint32_t S = d.nsub[q];
    if (S == 0) return;
    jpegd_load_tables(tabs, d.tabs + q * 3, 3, FIRST_THREADS);
    const JpegGeo cg = jpegdprog_geo(a.g, sc);
    const uint32_t K = jpegd_intervals(cg);
    const PSeg sg = segment(a, d, q);
    JpegdState* ex = d.exit + sg.slot;
    uint32_t* cnt = d.cnt + sg.slot;
    int16_t* coef = a.coef + (size_t)img * a.g.NB * 64;
    int32_t* dcdiff = d.dcdiff + (size_t)img * a.g.SB;
    const uint32_t chunks = (S + FIRST_THREADS - 1) / FIRST_THREADS;
    uint32_t unused = 0;
    // speculate: every subsequence from the guess "a block starts here"; the first of an interval from its true state
    for (uint32_t c = 0; c < chunks; ++c) {
        const uint32_t i = c * FIRST_THREADS + tid;
        if (i >= S) continue;
        const JpegdSpan sp = jpegd_span(cg, sg.ibit, sg.sub0, K, a.sb, i);
        JpegdState s = jpegdprog_start(sc, sp.start);
        uint32_t done;
        jpegdprog_run_first<false>(sg.bits, sg.nwords, sp.end, sp.limit, tabs, a.g, sc, cg.per, s, done, 0u, 0u, 0u, nullptr, nullptr, unused);
        ex[i] = s; cnt[i] = done;
    }
    __syncthreads();
    // synchronise (jpegd_sync.h), then place: the first block every subsequence completes
    const auto active = [&](uint32_t i, uint32_t r, JpegdSpan& sp) {
        sp = jpegd_span(cg, sg.ibit, sg.sub0, K, a.sb, i);
        return sp.j >= r;
    };
    const auto run = [&](uint32_t, const JpegdSpan& sp, JpegdState& s, uint32_t& done) {
        jpegdprog_run_first<false>(sg.bits, sg.nwords, sp.end, sp.limit, tabs, a.g, sc, cg.per, s, done, 0u, 0u, 0u, nullptr, nullptr, unused);
    };
    const uint32_t rounds = jpegd_sync_rounds<FIRST_THREADS>(S, d.maxsub[q], ex, cnt, active, run);
    const uint32_t completed = jpegd_place_blocks<FIRST_THREADS>(S, cnt, wtot);
    const uint32_t per = jpegdprog_interval_blocks(cg);        // every interval must have completed its own blocks
    uint32_t status = jpegd_intervals_short(cnt, sg.sub0, K, completed, per, (uint32_t)cg.SB, tid, FIRST_THREADS) ? JPEGD_ST_BLOCKS : 0u;
    // write
    for (uint32_t c = 0; c < chunks; ++c) {
        const uint32_t i = c * FIRST_THREADS + tid;
        if (i >= S) continue;
        const JpegdSpan sp = jpegd_span(cg, sg.ibit, sg.sub0, K, a.sb, i);
        JpegdState s = sp.j ? ex[i - 1] : jpegdprog_start(sc, sp.start);
        uint32_t done;
        jpegdprog_run_first<true>(sg.bits, sg.nwords, sp.end, sp.limit, tabs, a.g, sc, cg.per, s, done, sp.block_begin + (cnt[i] - cnt[sg.sub0[sp.k]]),
                                  sp.block_begin, sp.block_end, coef, dcdiff, status);
    }
    if (tid == 0) a.rounds[q] = rounds;
    if (sc.ss == 0) {
        // DC: per component the running sum of its differences in scan order, then every block's sum since its interval began
        __syncthreads();
        const int ny = cg.ny, mcus = cg.SB / cg.per;
        for (int comp = 0; comp < 3; ++comp) {
            if (!(sc.mask >> comp & 1)) continue;
            const int count = sc.mask != 7 ? cg.SB : (comp ? mcus : mcus * ny);
            const int span = !cg.ri ? count : (sc.mask != 7 ? cg.ri : (comp ? cg.ri : cg.ri * ny));
            int sums = 0;
            for (int base = 0; base < count; base += FIRST_THREADS) {
                const int j = base + tid;
                const uint32_t b = sc.mask != 7 ? (uint32_t)j : jpegd_dc_block(ny, cg.per, comp, j);
                const int v = j < count ? dcdiff[jpegdprog_dc_slot(a.g, sc, b)] : 0;
                int sum;
                const int incl = sums + block_excl_scan<int, FIRST_THREADS>(v, (int*)wtot, sum) + v;
                sums += sum;
                if (j < count) dcdiff[jpegdprog_dc_slot(a.g, sc, b)] = incl;
            }
            __syncthreads();
            for (int j = tid; j < count; j += FIRST_THREADS) {
                const int first = j / span * span;
                const uint32_t b = sc.mask != 7 ? (uint32_t)j : jpegd_dc_block(ny, cg.per, comp, j);
                const uint32_t bf = sc.mask != 7 ? (uint32_t)(first - 1) : jpegd_dc_block(ny, cg.per, comp, first - 1);
                const int sum = dcdiff[jpegdprog_dc_slot(a.g, sc, b)] - (first ? dcdiff[jpegdprog_dc_slot(a.g, sc, bf)] : 0);
                status |= jpegdprog_dc_store(coef, jpegdprog_place(a.g, sc, b), sum, sc.al);
            }
        }
    }
    if (status) atomicOr(a.status + img, status);
}

// ---- DC refine scans of a level: one thread per block ---------------------------------------------------------------------------
__global__ void __launch_bounds__(REFINE_THREADS) jpegd_prog_dc_refine_kernel(PArgs a, PLayout d, int level) {
    const int scan = blockIdx.y, img = blockIdx.z;
    const JpegdProgScan sc = a.script.sc[scan];
    if (sc.level != level || jpegdprog_first(sc) || sc.ss != 0) return;
    const size_t q = (size_t)img * a.script.n_scans + scan;
    if (d.nsub[q] == 0) return;
    const JpegGeo cg = jpegdprog_geo(a.g, sc);
    const uint32_t b = blockIdx.x * REFINE_THREADS + threadIdx.x;
    if (b >= (uint32_t)cg.SB) return;
    const PSeg sg = segment(a, d, q);
    const uint32_t st = jpegdprog_dc_refine_block(sg.bits, sg.nwords, sg.ibit, a.g, cg, sc, b, a.coef + (size_t)img * a.g.NB * 64);
    if (st) atomicOr(a.status + img, st);
}

// ---- AC refine scans of a level: one wave per (image, scan, restart interval) ------------------------------------------------------
// jpegdprog_ac_refine_interval with the 64 lanes holding the 64 coefficients of the block in progress.  The blocks are still walked in
// order and every symbol is parsed by the whole wave on uniform values; what the lanes share out is the inner walk: the non-zero history
// of a block is one ballot, the place a zero run ends is its (r + 1)-th clear bit, the correction bits of the coefficients passed are
// consecutive in the stream, and each such lane takes the bit of its rank.  A block of an end-of-band run is one load, one ballot and
// one store.  The stores of a failing symbol are those of the sequential walk - the corrections whose bits the stream still has - so
// that later scans see the same history on the device and in the host program.
__global__ void __launch_bounds__(64) jpegd_prog_ac_refine_kernel(PArgs a, PLayout d, int level) {
    __shared__ JpegdTable tab;
    const int scan = blockIdx.y, img = blockIdx.z, lane = threadIdx.x;
    const JpegdProgScan sc = a.script.sc[scan];
    if (sc.level != level || jpegdprog_first(sc) || sc.ss == 0) return;
    const size_t q = (size_t)img * a.script.n_scans + scan;
    if (d.nsub[q] == 0) return;
    const JpegGeo cg = jpegdprog_geo(a.g, sc);
    const uint32_t k = blockIdx.x, per = jpegdprog_interval_blocks(cg);
    if (k >= jpegd_intervals(cg)) return;
    jpegd_load_tables(&tab, d.tabs + q * 3, 1, 64);
    const PSeg sg = segment(a, d, q);
    const uint32_t b0 = k * per, nb = min(b0 + per, (uint32_t)cg.SB) - b0, end = sg.ibit[k + 1u];
    int16_t* blk = a.coef + ((size_t)img * a.g.NB + (size_t)jpegdprog_place(a.g, sc, b0)) * 64;
    const unsigned long long band = (sc.se == 63 ? ~0ull : (1ull << (sc.se + 1)) - 1ull) & ~((1ull << sc.ss) - 1ull);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int p1 = 1 << sc.al;
    uint32_t p = sg.ibit[k], eobrun = 0, st = 0;
    for (uint32_t b = 0; b < nb && !st; ++b, blk += 64) {
        const int c0 = blk[lane];
        int c = c0, kk = sc.ss;
        const unsigned long long nz = __ballot(c0 != 0) & band;
        // the corrections of the non-zero coefficients in m, in zig-zag order from bit p on; false = the stream ends before the last
        auto correct = [&](unsigned long long m) {
            const uint32_t count = (uint32_t)__popcll(m), at = p + (uint32_t)__popcll(m & below);
            if ((m >> lane & 1ull) && at < end) c = jpegdprog_correct(c, jpegd_peek(sg.bits, sg.nwords, at) >> 31, p1);
            if (p + count > end) return false;
            p += count;
            return true;
        };
        if (eobrun == 0) {
            while (kk <= sc.se) {
                const uint32_t window = jpegd_peek(sg.bits, sg.nwords, p);
                int len;
                const int sym = jpegd_symbol(tab, window, len);
                if (sym < 0) { st = JPEGD_ST_CODE; break; }
                const int sz = sym & 15, r = sym >> 4;
                int fresh = 0;
                if (sz) {
                    if (sz != 1) { st = JPEGD_ST_CATEGORY; break; }
                    if (p + (uint32_t)len + 1u > end) { st = JPEGD_ST_END; break; }
                    fresh = ((window << len) >> 31) ? p1 : -p1;
                    p += (uint32_t)len + 1u;
                } else if (r != 15) {
                    if (p + (uint32_t)(len + r) > end) { st = JPEGD_ST_END; break; }
                    const uint32_t run = (1u << r) + (r ? (window << len) >> (32 - r) : 0u);
                    if (run > nb - b) { st = JPEGD_ST_RUN; break; }
                    p += (uint32_t)(len + r);
                    eobrun = run;
                    break;
                } else {
                    if (p + (uint32_t)len > end) { st = JPEGD_ST_END; break; }
                    p += (uint32_t)len;
                }
                const unsigned long long from = ~0ull << kk;
                unsigned long long zeros = ~nz & band & from;
                for (int z = 0; z < r && zeros; ++z) zeros &= zeros - 1ull;           // the (r + 1)-th zero ends the walk
                const int pos = zeros ? __builtin_ctzll(zeros) : sc.se + 1;
                if (!correct(nz & from & (pos > 63 ? ~0ull : (1ull << pos) - 1ull))) { st = JPEGD_ST_END; break; }
                kk = pos;
                if (fresh) {
                    if (kk > sc.se) { st = JPEGD_ST_ZIGZAG; break; }
                    if (lane == kk) c = fresh;
                }
                ++kk;
            }
        }
        if (!st && eobrun > 0) {                       // inside a run: the rest of the band takes correction bits only
            if (!correct(kk > 63 ? 0ull : nz & (~0ull << kk))) st = JPEGD_ST_END;
            --eobrun;
        }
        if (c != c0) blk[lane] = (int16_t)c;
    }
    if (st && lane == 0) atomicOr(a.status + img, st);
}

// the script of a call, checked: the rules of jpegdprog.h, and the levels the caller passes are the ones they give
bool take_script(const int32_t* script, int n_scans, int nc, PScript* out, int* top) {
    int32_t levels[JPEGDPROG_SCANS_MAX];
    if (!script || !jpegdprog_check_script(script, n_scans, levels, nc)) return false;
    out->n_scans = n_scans;
    *top = 0;
    for (int s = 0; s < n_scans; ++s) {
        const int32_t* e = script + 6 * s;
        if (e[5] != levels[s]) return false;
        out->sc[s] = JpegdProgScan{e[0], e[1], e[2], e[3], e[4], e[5]};
        *top = levels[s] > *top ? levels[s] : *top;
    }
    return true;
}

// ---- the launchers, for frames of three components (nc = 3) and of one (nc = 1, section 4p) ---------------------------------------
size_t progressive_workspace_size(int n, int h, int w, int hs, int vs, int nc, int restart_interval, int n_scans, size_t ecd_bytes,
                                  int subseq_bits, int factors = JPEG_FACTORS_THREE) {
    JpegGeo g;
    uint32_t sb;
    if (!make_geo(&g, n, h, w, hs, vs, nc, factors) || !set_restart(&g, restart_interval) || !jpegd_subseq_ok(subseq_bits, PROG_SUBSEQ_DEFAULT, &sb) || n_scans < 1 ||
        n_scans > JPEGDPROG_SCANS_MAX || ecd_bytes > (size_t)n * n_scans * JPEGD_ECD_MAX)
        return 0;
    return carve_p(g, n_scans, ecd_bytes, sb, nullptr).bytes;
}

int progressive_launch(const uint8_t* ecd, const uint64_t* ecd_off, const int32_t* script, int n_scans, const uint8_t* huffman, int n, int h,
                       int w, int hs, int vs, int nc, int restart_interval, int subseq_bits, int16_t* coef, uint32_t* status,
                       uint32_t* rounds, void* workspace, size_t workspace_bytes, void* stream, int factors = JPEG_FACTORS_THREE) {
    JpegGeo g;
    uint32_t sb;
    PArgs a;
    int top;
    if (!ecd || !ecd_off || !huffman || !coef || !status || !rounds || !workspace || !make_geo(&g, n, h, w, hs, vs, nc, factors) ||
        !set_restart(&g, restart_interval) || !jpegd_subseq_ok(subseq_bits, PROG_SUBSEQ_DEFAULT, &sb) || !take_script(script, n_scans, nc, &a.script, &top))
        return NIMG_ERR_ARG;
    const auto bytes_for = [&](uint64_t ecd_bytes) { return carve_p(g, n_scans, ecd_bytes, sb, workspace).bytes; };
    if (bytes_for(0) > workspace_bytes) return NIMG_ERR_ARG;
    const uint64_t lo = jpegd_ecd_capacity(bytes_for, (uint64_t)n * n_scans * JPEGD_ECD_MAX, workspace_bytes);
    const PLayout d = carve_p(g, n_scans, lo, sb, workspace);
    a.ecd = ecd; a.off = ecd_off; a.huffman = huffman; a.ecd_cap = lo; a.sb = sb; a.Kmax = intervals_max(g); a.g = g;
    a.coef = coef; a.status = status; a.rounds = rounds;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, (size_t)n * 4, st) != hipSuccess || hipMemsetAsync(coef, 0, (size_t)n * g.NB * 128, st) != hipSuccess ||
        hipMemsetAsync(d.dcdiff, 0, (size_t)n * g.SB * 4, st) != hipSuccess || hipMemsetAsync(d.raw, 0, d.raw_words * 4, st) != hipSuccess)
        return NIMG_ERR_LAUNCH;
    const dim3 per_scan((unsigned)n_scans, (unsigned)n);
    if (g.ri) hipLaunchKernelGGL(jpegd_prog_prepare_kernel<true>, per_scan, dim3(SCAN_THREADS), 0, st, a, d);
    else hipLaunchKernelGGL(jpegd_prog_prepare_kernel<false>, per_scan, dim3(SCAN_THREADS), 0, st, a, d);
    NIMG_CHECK_LAUNCH();
    for (int level = 1; level <= top; ++level) {
        bool first = false, dc = false, ac = false;
        for (int s = 0; s < n_scans; ++s) {
            const JpegdProgScan& sc = a.script.sc[s];
            if (sc.level != level) continue;
            if (jpegdprog_first(sc)) first = true;
            else if (sc.ss == 0) dc = true;
            else ac = true;
        }
        if (first) {
            hipLaunchKernelGGL(jpegd_prog_first_kernel, per_scan, dim3(FIRST_THREADS), 0, st, a, d, level);
            NIMG_CHECK_LAUNCH();
        }
        if (dc) {
            hipLaunchKernelGGL(jpegd_prog_dc_refine_kernel, dim3((unsigned)((g.SB + REFINE_THREADS - 1) / REFINE_THREADS), (unsigned)n_scans, (unsigned)n),
                               dim3(REFINE_THREADS), 0, st, a, d, level);
            NIMG_CHECK_LAUNCH();
        }
        if (ac) {
            hipLaunchKernelGGL(jpegd_prog_ac_refine_kernel, dim3(a.Kmax, (unsigned)n_scans, (unsigned)n), dim3(64), 0, st, a, d, level);
            NIMG_CHECK_LAUNCH();
        }
    }
    return NIMG_OK;
}

}  // namespace

extern "C" {

size_t nimg_jpeg_decode_progressive_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval, int n_scans, size_t ecd_bytes,
                                                    int subseq_bits) {
    return progressive_workspace_size(n, h, w, hs, vs, 3, restart_interval, n_scans, ecd_bytes, subseq_bits);
}

int nimg_jpeg_decode_progressive(const uint8_t* ecd, const uint64_t* ecd_off, const int32_t* script, int n_scans, const uint8_t* huffman, int n,
                                 int h, int w, int hs, int vs, int restart_interval, int subseq_bits, int16_t* coef, uint32_t* status,
                                 uint32_t* rounds, void* workspace, size_t workspace_bytes, void* stream) {
    return progressive_launch(ecd, ecd_off, script, n_scans, huffman, n, h, w, hs, vs, 3, restart_interval, subseq_bits, coef, status, rounds,
                              workspace, workspace_bytes, stream);
}

// the same launcher with the wide set of sampling factors
size_t nimg_jpeg_sampling_decode_progressive_workspace_bytes(int n, int h, int w, int hs, int vs, int restart_interval, int n_scans,
                                                             size_t ecd_bytes, int subseq_bits) {
    return progressive_workspace_size(n, h, w, hs, vs, 3, restart_interval, n_scans, ecd_bytes, subseq_bits, JPEG_FACTORS_WIDE);
}

int nimg_jpeg_sampling_decode_progressive(const uint8_t* ecd, const uint64_t* ecd_off, const int32_t* script, int n_scans,
                                          const uint8_t* huffman, int n, int h, int w, int hs, int vs, int restart_interval, int subseq_bits,
                                          int16_t* coef, uint32_t* status, uint32_t* rounds, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    return progressive_launch(ecd, ecd_off, script, n_scans, huffman, n, h, w, hs, vs, 3, restart_interval, subseq_bits, coef, status, rounds,
                              workspace, workspace_bytes, stream, JPEG_FACTORS_WIDE);
}

size_t nimg_jpeg_grey_decode_progressive_workspace_bytes(int n, int h, int w, int restart_interval, int n_scans, size_t ecd_bytes,
                                                         int subseq_bits) {
    return progressive_workspace_size(n, h, w, 1, 1, 1, restart_interval, n_scans, ecd_bytes, subseq_bits);
}

int nimg_jpeg_grey_decode_progressive(const uint8_t* ecd, const uint64_t* ecd_off, const int32_t* script, int n_scans, const uint8_t* huffman,
                                      int n, int h, int w, int restart_interval, int subseq_bits, int16_t* coef, uint32_t* status,
                                      uint32_t* rounds, void* workspace, size_t workspace_bytes, void* stream) {
    if (n == 0) return NIMG_OK;
    return progressive_launch(ecd, ecd_off, script, n_scans, huffman, n, h, w, 1, 1, 1, restart_interval, subseq_bits, coef, status, rounds,
                              workspace, workspace_bytes, stream);
}

}  // extern "C"
