// The sequential core of writing progressive JPEG files (libjpeg's jpeg_simple_progression): the scan script,
// the block walks of the four scan kinds (DC first, DC refine, AC first, AC refine; T.81 Annex G with libjpeg's choices) over one sink
// interface, and the resolution of the end-of-band runs from one summary word per block.  jpegc_prog.hip runs the walks one thread per
// (scan, block) behind a histogram, a bit-length and an emit sink; tests/jpegprog_host.cpp runs the same copy on the host.  Everything
// here is `__host__ __device__` under hipcc and plain C++ otherwise.
//
// A block of an AC scan writes, in this order: the symbols and bits of its own coefficients; if an end-of-band run starts with it, the
// run's EOBn symbol and its n run bits; the correction bits it leaves behind its last symbol.  libjpeg writes the EOBn symbol when the
// run ends and the waiting correction bits of all the run's blocks behind it - the same bits in the same order, so every block's bits
// are contiguous and a block needs nothing of its neighbours but the length of the run it starts.
#pragma once
#include <stdint.h>

#include "jpeg_geo.h"
#include "jpegopt.h"

#define JPEGPROG_HD JPEGOPT_HD

#define JPEGPROG_SCANS 10
#define JPEGPROG_TABLES 10               // in the order of the file's DHT segments: DC 00, DC 01, the AC tables of scans 1 2 3 4 5 7 8 9
#define JPEGPROG_CODE_WORDS 2080         // one image's code words: two DC tables [16], eight AC tables [256]
#define JPEGPROG_RUN_MAX 0x7fff          // a run of this many blocks is written at once
#define JPEGPROG_BE_FLUSH 937            // and so is a run with more correction bits waiting (libjpeg: MAX_CORR_BITS - DCTSIZE2 + 1)
// The longest block of a scan.  DC first: a code of 16 bits and 11 value bits.  AC first: the point transform leaves at most 9 value bits
// (|v| <= 1023, Al >= 1), so 63 coefficients are 63 * 25 bits; 62 and a trailing zero that starts a run of 0x7fff blocks are
// 62 * 25 + 16 + 14, which is more.  AC refine: 63 new coefficients of 16 + 1 bits, less.
#define JPEGPROG_DC_BITS_MAX 27
#define JPEGPROG_AC_BITS_MAX 1580

// a block's summary word
#define JPEGPROG_SUM_FLUSH 1u            // it emits a symbol: a run that waits is written in front of it
#define JPEGPROG_SUM_RUN 2u              // it ends in zeros or correction bits: it joins (or starts) a run
#define JPEGPROG_SUM_BITS_SHIFT 2        // the correction bits it leaves to the run, 0..63

// comp: 0 Y, 1 Cb, 2 Cr, -1 all three interleaved.  table: which of the ten tables (the DC first scan: 0 for Y, 1 for chroma; the DC
// refine scan: none).  cls / idx: the scans of one class have the same block grid - 0 interleaved, 1 Y, 2 one chroma component.
struct JpegProgScan { int comp, ss, se, ah, al, table, cls, idx; };

JPEGPROG_HD inline JpegProgScan jpegprog_scan(int i) {
    switch (i) {
        case 0: return JpegProgScan{-1, 0, 0, 0, 1, 0, 0, 0};
        case 1: return JpegProgScan{0, 1, 5, 0, 2, 2, 1, 0};
        case 2: return JpegProgScan{2, 1, 63, 0, 1, 3, 2, 0};
        case 3: return JpegProgScan{1, 1, 63, 0, 1, 4, 2, 1};
        case 4: return JpegProgScan{0, 6, 63, 0, 2, 5, 1, 1};
        case 5: return JpegProgScan{0, 1, 63, 2, 1, 6, 1, 2};
        case 6: return JpegProgScan{-1, 0, 0, 1, 0, -1, 0, 1};
        case 7: return JpegProgScan{2, 1, 63, 1, 0, 7, 2, 2};
        case 8: return JpegProgScan{1, 1, 63, 1, 0, 8, 2, 3};
        default: return JpegProgScan{0, 1, 63, 1, 0, 9, 1, 3};
    }
}

JPEGPROG_HD inline int jpegprog_class_scans(int cls) { return cls == 0 ? 2 : 4; }
// blocks of a scan of class cls: the MCU grid with its dummy blocks, or the real blocks of the component
JPEGPROG_HD inline int jpegprog_class_blocks(const JpegGeo& g, int cls) { return cls == 0 ? g.SB : (cls == 1 ? g.nbY : g.nbC); }
JPEGPROG_HD inline int jpegprog_class_bits(int cls) { return cls == 0 ? JPEGPROG_DC_BITS_MAX : JPEGPROG_AC_BITS_MAX; }
// where the code words of table t stand in an image's code words
JPEGPROG_HD inline int jpegprog_code_base(int t) { return t < 2 ? 16 * t : 32 + 256 * (t - 2); }

// The geometry the offset scan and the restart markers of a scan of class cls see: for a single-component scan every real block is an
// MCU, in raster order over the component's own grid.
JPEGPROG_HD inline JpegGeo jpegprog_class_geo(const JpegGeo& g, int cls) {
    JpegGeo c = g;
    c.n = g.n * jpegprog_class_scans(cls);
    if (cls != 0) {
        c.my = cls == 1 ? g.bhY : g.bhC;
        c.mx = cls == 1 ? g.bwY : g.bwC;
        c.per = 1; c.ny = 1;
        c.SB = c.my * c.mx;
    }
    return c;
}

// the words of one scan's un-stuffed bits, c = jpegprog_class_geo(g, cls): every block at its longest, a restart marker's 16 bits and
// up to 7 of padding in front of it, a multiple of 4 words (jpegc.h's carve has the same form)
JPEGPROG_HD inline unsigned jpegprog_raw_words(const JpegGeo& c, int cls) {
    const unsigned long words = ((unsigned long)c.SB * (unsigned long)jpegprog_class_bits(cls) + 23ul * (unsigned long)jpeg_markers(c) + 31) / 32 + 1;
    return (unsigned)((words + 3) & ~3ul);
}

// the first coefficient of block b of a single-component scan
JPEGPROG_HD inline const int16_t* jpegprog_block(const int16_t* ci, const JpegGeo& g, int comp, int b) {
    return ci + ((long)(comp == 0 ? 0 : g.nbY + (comp - 1) * g.nbC) + b) * 64;
}

// what the coder can carry, as the baseline coder clamps: a DC coefficient to +-2047 (the difference of two point-transformed ones then
// has at most 11 bits), an AC coefficient to +-1023 - before the point transform
JPEGPROG_HD inline int jpegprog_clamp_dc(int v) { return v < -2047 ? -2047 : (v > 2047 ? 2047 : v); }
JPEGPROG_HD inline int jpegprog_clamp_ac(int v) { return v < -1023 ? -1023 : (v > 1023 ? 1023 : v); }

// A sink has symbol(table, symbol, value bits, their number) and raw(bits, their number <= 63).
// Block s (scan order, dummies included) of an interleaved DC scan.  First scan: the difference of the point-transformed DC to that of
// the component's block before it, 0 at the start of a restart interval; table 0 for Y, 1 for chroma.  Refine scan: one bit.
template <typename Sink>
JPEGPROG_HD inline void jpegprog_walk_dc(const int16_t* ci, const JpegGeo& g, int s, bool refine, int al, Sink& sink) {
    const int m = s / g.per, k = s - m * g.per, mr = m / g.mx, mc = m - mr * g.mx, ny = g.ny;
    int dc, pred = 0;
    bool real, have = true;
    if (k < ny) {
        dc = jpegopt_y_dc(ci, g, mr, mc, k, real);
        if (k > 0) pred = jpegopt_y_dc(ci, g, mr, mc, k - 1, real);
        else if (!jpeg_interval_start(g, m)) pred = jpegopt_y_dc(ci, g, (m - 1) / g.mx, (m - 1) % g.mx, ny - 1, real);
        else have = false;
    } else {
        const int16_t* blk = ci + ((long)g.nbY + (long)(k - ny) * g.nbC + m) * 64;
        dc = blk[0];
        if (!jpeg_interval_start(g, m)) pred = blk[-64];
        else have = false;
    }
    const int v = jpegprog_clamp_dc(dc) >> al;
    if (refine) {
        sink.raw((uint64_t)(v & 1), 1);
        return;
    }
    const int diff = v - (have ? jpegprog_clamp_dc(pred) >> al : 0);
    const int sz = jpegopt_category(__builtin_abs(diff));
    sink.symbol(k < ny ? 0 : 1, sz, (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << sz) - 1u), sz);
}

// what a block of an AC scan leaves to the run resolution and to its own end
struct JpegProgTail {
    uint32_t summary;
    uint64_t bits;                     // the correction bits behind its last symbol, the first in the highest place
    JPEGPROG_HD int nbits() const { return (int)(summary >> JPEGPROG_SUM_BITS_SHIFT); }
};

// one block of an AC first scan: blk[ss..se] in zig-zag order
template <typename Sink>
JPEGPROG_HD inline JpegProgTail jpegprog_walk_ac_first(const int16_t* blk, int ss, int se, int al, int table, Sink& sink) {
    uint32_t sum = 0;
    int r = 0;
    for (int k = ss; k <= se; ++k) {
        const int v = jpegprog_clamp_ac(blk[k]), a = __builtin_abs(v) >> al;
        if (a == 0) { ++r; continue; }
        sum |= JPEGPROG_SUM_FLUSH;
        while (r > 15) {
            sink.symbol(table, 0xf0, 0u, 0);
            r -= 16;
        }
        const int sz = jpegopt_category(a);
        sink.symbol(table, (r << 4) | sz, (uint32_t)(v < 0 ? ~a : a) & ((1u << sz) - 1u), sz);
        r = 0;
    }
    if (r > 0) sum |= JPEGPROG_SUM_RUN;
    return JpegProgTail{sum, 0};
}

// one block of an AC refine scan.  A zero run of 16 is written only in front of a coefficient that becomes non-zero in this scan
// (k <= eob); behind the last such coefficient the zeros and the correction bits go to the run.
template <typename Sink>
JPEGPROG_HD inline JpegProgTail jpegprog_walk_ac_refine(const int16_t* blk, int ss, int se, int al, int table, Sink& sink) {
    int eob = 0;
    for (int k = ss; k <= se; ++k)
        if ((__builtin_abs(jpegprog_clamp_ac(blk[k])) >> al) == 1) eob = k;
    uint32_t sum = 0;
    uint64_t br = 0;
    int r = 0, nbr = 0;
    for (int k = ss; k <= se; ++k) {
        const int v = jpegprog_clamp_ac(blk[k]), a = __builtin_abs(v) >> al;
        if (a == 0) { ++r; continue; }
        while (r > 15 && k <= eob) {
            sum |= JPEGPROG_SUM_FLUSH;
            sink.symbol(table, 0xf0, 0u, 0);
            r -= 16;
            sink.raw(br, nbr);
            br = 0; nbr = 0;
        }
        if (a > 1) {
            br = (br << 1) | (uint64_t)(a & 1);
            ++nbr;
            continue;
        }
        sum |= JPEGPROG_SUM_FLUSH;
        sink.symbol(table, (r << 4) | 1, v > 0 ? 1u : 0u, 1);
        sink.raw(br, nbr);
        br = 0; nbr = 0; r = 0;
    }
    if (r > 0 || nbr > 0) sum |= JPEGPROG_SUM_RUN | ((uint32_t)nbr << JPEGPROG_SUM_BITS_SHIFT);
    return JpegProgTail{sum, br};
}

// block b of single-component scan sc
template <typename Sink>
JPEGPROG_HD inline JpegProgTail jpegprog_walk_ac(const int16_t* ci, const JpegGeo& g, const JpegProgScan& sc, int b, Sink& sink) {
    const int16_t* blk = jpegprog_block(ci, g, sc.comp, b);
    return sc.ah ? jpegprog_walk_ac_refine(blk, sc.ss, sc.se, sc.al, sc.table, sink)
                 : jpegprog_walk_ac_first(blk, sc.ss, sc.se, sc.al, sc.table, sink);
}

// ---- the end-of-band runs ---------------------------------------------------------------------------------------------------
// The state of one scan between two blocks; walked over the summaries of its blocks in order.  rec.run(first block, length) is called
// once per run, when it ends: in front of a block that emits a symbol, at the start of a restart interval, at JPEGPROG_RUN_MAX blocks,
// with more than JPEGPROG_BE_FLUSH correction bits waiting, and at the end of the scan.
struct JpegProgRun { int length = 0, waiting = 0, first = 0; };

template <typename Rec>
JPEGPROG_HD inline void jpegprog_run_end(JpegProgRun& r, Rec& rec) {
    if (r.length > 0) rec.run(r.first, r.length);
    r.length = 0;
    r.waiting = 0;
}

template <typename Rec>
JPEGPROG_HD inline void jpegprog_run_block(JpegProgRun& r, int b, int restart_interval, uint32_t summary, Rec& rec) {
    if ((summary & JPEGPROG_SUM_FLUSH) || (restart_interval > 0 && b % restart_interval == 0)) jpegprog_run_end(r, rec);
    if (summary & JPEGPROG_SUM_RUN) {
        if (r.length == 0) r.first = b;
        ++r.length;
        r.waiting += (int)(summary >> JPEGPROG_SUM_BITS_SHIFT);
        if (r.length == JPEGPROG_RUN_MAX || r.waiting > JPEGPROG_BE_FLUSH) jpegprog_run_end(r, rec);
    }
}

// a run of `length` blocks as its EOBn symbol: n << 4 with the low n bits of the length
JPEGPROG_HD inline int jpegprog_run_category(int length) { return 31 - __builtin_clz((unsigned)length); }

// what a block's own end adds behind its symbols: the EOBn symbol of the run that starts with it (length 0: none), then its correction bits
template <typename Sink>
JPEGPROG_HD inline void jpegprog_block_end(const JpegProgTail& t, int table, int run_length, Sink& sink) {
    if (run_length > 0) {
        const int n = jpegprog_run_category(run_length);
        sink.symbol(table, n << 4, (uint32_t)run_length & ((1u << n) - 1u), n);
    }
    if (t.summary & JPEGPROG_SUM_RUN) sink.raw(t.bits, t.nbits());
}

// the ten tables of an image as DHT segments have them -> its JPEGPROG_CODE_WORDS code words; false = one is refused, all words zero
JPEGPROG_HD inline bool jpegprog_derive_image(const uint8_t* tables, uint32_t* codes) {
    bool ok = true;
    for (int t = 0; t < JPEGPROG_TABLES; ++t)
        ok = jpegopt_derive(tables + t * JPEGOPT_TABLE_BYTES, codes + jpegprog_code_base(t), t < 2 ? 16 : 256) && ok;
    if (!ok)
        for (int i = 0; i < JPEGPROG_CODE_WORDS; ++i) codes[i] = 0;
    return ok;
}
