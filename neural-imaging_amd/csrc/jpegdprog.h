// The sequential core of reading progressive JPEG files (T.81 Annex G as libjpeg's jdphuff.c reads it): the rules
// of a scan script and its levels, the place of a scan's block, and the decode of the four scan kinds.  DC and AC first scans are
// decoded a subsequence at a time from a state, counting or writing, as jpegd.h's baseline run is - the state between two symbols is
// (bit, block of the MCU) or (bit, zig-zag position), and the counter is the blocks COMPLETED, so that an end-of-band run, whose
// skipped blocks cost no bits, advances the counter and never enters the state.  A DC refine scan is one bit per block.  An AC refine
// scan is decoded one restart interval at a time in order: what a block consumes depends on which of its coefficients are non-zero.
// jpegd_prog.hip runs this copy on the device, tests/jpegdprog_host.cpp on the host; everything is `__host__ __device__` under hipcc
// and plain C++ otherwise.  Every loop is bounded by the stream's bits or the scan's blocks, no load leaves the bit buffer, no store
// leaves the block and band it belongs to.
#pragma once
#include <stdint.h>

#include "jpegd.h"
#include "jpegprog.h"

#define JPEGD_ST_RUN 1024u               // an end-of-band run beyond the blocks of the scan (of its restart interval)
#define JPEGDPROG_SCANS_MAX 64

// one scan as the library's callers pass it: six int32
struct JpegdProgScan {
    int32_t mask;                        // components: bit c = component c; 7 = all three interleaved (DC scans only)
    int32_t ss, se, ah, al;
    int32_t level;                       // 1 + the highest level of an earlier scan of a shared component whose band overlaps
};

JPEGD_HD inline int jpegdprog_cls(const JpegdProgScan& sc) { return sc.mask == 7 ? 0 : (sc.mask == 1 ? 1 : 2); }
// the component of a single-component scan
JPEGD_HD inline int jpegdprog_comp(const JpegdProgScan& sc) { return sc.mask == 1 ? 0 : (sc.mask == 2 ? 1 : 2); }
JPEGD_HD inline bool jpegdprog_first(const JpegdProgScan& sc) { return sc.ah == 0; }

// The rules of a script: a DC scan (Ss = Se = 0) holds one component or all three, an AC scan (1 <= Ss <= Se <= 63) exactly one; a
// coefficient's first scan has Ah = 0, each later one Ah = the Al before and Al = Ah - 1; a component's DC first scan precedes its AC
// scans; every coefficient of every component reaches Al = 0.  levels (may be null) takes the level of every scan.  A frame of one
// component (nc = 1, a grey-scale file) has scans of that component alone: every mask is 1.
JPEGD_HD inline bool jpegdprog_check_script(const int32_t* script, int n_scans, int32_t* levels, int nc = 3) {
    if (n_scans < 1 || n_scans > JPEGDPROG_SCANS_MAX) return false;
    int8_t al_of[3][64];
    int32_t lev[JPEGDPROG_SCANS_MAX];
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 64; ++k) al_of[c][k] = -1;
    for (int s = 0; s < n_scans; ++s) {
        const int32_t* q = script + 6 * s;
        const int mask = q[0], ss = q[1], se = q[2], ah = q[3], al = q[4];
        if (mask != 7 && mask != 1 && mask != 2 && mask != 4) return false;
        if (nc == 1 && mask != 1) return false;
        if (ss < 0 || se > 63 || ss > se || (ss == 0 && se != 0) || (ss > 0 && mask == 7)) return false;
        if (ah < 0 || ah > 13 || al < 0 || al > 13) return false;
        for (int c = 0; c < 3; ++c) {
            if (!(mask >> c & 1)) continue;
            if (ss > 0 && al_of[c][0] < 0) return false;
            for (int k = ss; k <= se; ++k) {
                if (ah == 0 ? al_of[c][k] != -1 : (al_of[c][k] != ah || al != ah - 1)) return false;
                al_of[c][k] = (int8_t)al;
            }
        }
        int l = 0;
        for (int t = 0; t < s; ++t) {
            const int32_t* e = script + 6 * t;
            if ((e[0] & mask) && e[1] <= se && ss <= e[2] && lev[t] > l) l = lev[t];
        }
        lev[s] = l + 1;
        if (levels) levels[s] = l + 1;
    }
    for (int c = 0; c < nc; ++c)
        for (int k = 0; k < 64; ++k)
            if (al_of[c][k] != 0) return false;
    return true;
}

// the geometry a scan's blocks, restart intervals and subsequences see (jpegprog.h): the MCU grid of an interleaved scan, the real
// blocks of a single component in raster order
JPEGD_HD inline JpegGeo jpegdprog_geo(const JpegGeo& g, const JpegdProgScan& sc) {
    JpegGeo c = jpegprog_class_geo(g, jpegdprog_cls(sc));
    c.n = g.n;
    return c;
}

// where the blocks of component c begin in an image's tensor
JPEGD_HD inline long jpegdprog_base(const JpegGeo& g, int c) { return c == 0 ? 0 : (long)g.nbY + (long)(c - 1) * g.nbC; }

// block b of a scan -> the offset (in blocks) of its coefficients in the image's tensor, -1 for a dummy block
JPEGD_HD inline long jpegdprog_place(const JpegGeo& g, const JpegdProgScan& sc, uint32_t b) {
    int comp;
    return sc.mask == 7 ? jpegd_place(g, b, comp) : jpegdprog_base(g, jpegdprog_comp(sc)) + (long)b;
}

// where the DC difference of block b of a DC first scan waits for the sums: an image has g.SB slots, an interleaved scan uses them in
// scan order, a single-component scan those of its component's real blocks (NB <= SB)
JPEGD_HD inline long jpegdprog_dc_slot(const JpegGeo& g, const JpegdProgScan& sc, uint32_t b) {
    return sc.mask == 7 ? (long)b : jpegdprog_base(g, jpegdprog_comp(sc)) + (long)b;
}

// the restart intervals of a scan, cg = jpegdprog_geo: interval j holds the blocks [j * per, min((j + 1) * per, cg.SB))
JPEGD_HD inline uint32_t jpegdprog_interval_blocks(const JpegGeo& cg) {
    return cg.ri > 0 ? (uint32_t)cg.ri * (uint32_t)cg.per : (uint32_t)cg.SB;
}

JPEGD_HD inline int jpegdprog_extend(uint32_t window, int len, int sz) {
    if (sz == 0) return 0;
    const int raw = (int)((window << len) >> (32 - sz));        // len + sz <= 27 bits of the window
    return (raw >> (sz - 1)) ? raw : raw - (1 << sz) + 1;
}

// One subsequence of a DC or AC first scan, as jpegd_run_interval: decodes from state `s` (mz = block of the MCU << 8 | zig-zag
// position; a DC scan keeps the position 0, an AC scan the block 0) until a symbol starts at or beyond `limit`, leaves the exit state
// in `s` and the blocks completed in `done`.  Every failure ends the run with s.p = JPEGD_INVALID.  The run belongs to one restart
// interval: total_bits is its end, [block_begin, block_end) its blocks in the scan's order.  tabs: the tables of the scan's components
// in its order.  g: the frame's geometry, per: the scan's blocks per MCU.
// WRITE: `block` is the first block completed here (the one in progress at entry).  AC values go to coef as v << Al, DC differences to
// dcdiff (jpegdprog_dc_slot), errors to `status`; the run ends with the interval's blocks and stores nothing outside them.
template <bool WRITE>
JPEGD_HD inline void jpegdprog_run_first(const uint32_t* bits, uint32_t nwords, uint32_t total_bits, uint32_t limit, const JpegdTable* tabs,
                                         const JpegGeo& g, const JpegdProgScan& sc, int per, JpegdState& s, uint32_t& done, uint32_t block,
                                         uint32_t block_begin, uint32_t block_end, int16_t* coef, int32_t* dcdiff, uint32_t& status) {
    done = 0;
    uint32_t p = s.p;
    if (p == JPEGD_INVALID) return;
    const bool dc = sc.ss == 0;
    int m = (int)(s.mz >> 8), k = (int)(s.mz & 255u);
    if (m >= per || (dc ? k != 0 : (k < sc.ss || k > sc.se))) { s.p = JPEGD_INVALID; s.mz = 0; return; }        // never a state left here
    uint32_t cur = block;
    if (WRITE && (cur < block_begin || cur > block_end)) return;
    const int ny = g.ny;
    uint32_t fail = 0;
    while (p < limit) {
        if (WRITE && cur >= block_end) break;
        const uint32_t window = jpegd_peek(bits, nwords, p);
        int len;
        const int sym = jpegd_symbol(tabs[dc && per > 1 && m >= ny ? m - ny + 1 : 0], window, len);
        if (sym < 0) { fail = JPEGD_ST_CODE; break; }
        if (dc) {
            if (sym > 11) { fail = JPEGD_ST_CATEGORY; break; }
            if (p + (uint32_t)(len + sym) > total_bits) { fail = JPEGD_ST_END; break; }
            if (WRITE) dcdiff[jpegdprog_dc_slot(g, sc, cur)] = jpegdprog_extend(window, len, sym);
            p += (uint32_t)(len + sym);
            m = m + 1 == per ? 0 : m + 1;
            ++done; ++cur;
            continue;
        }
        const int sz = sym & 15, r = sym >> 4;
        if (sz > 10) { fail = JPEGD_ST_CATEGORY; break; }
        if (sz == 0 && r < 15) {                       // EOBr: this block and 2^r - 1 + (r bits) further ones are complete
            if (p + (uint32_t)(len + r) > total_bits) { fail = JPEGD_ST_END; break; }
            const uint32_t run = (1u << r) + (r ? (window << len) >> (32 - r) : 0u);
            if (WRITE && run > block_end - cur) { fail = JPEGD_ST_RUN; break; }
            p += (uint32_t)(len + r);
            done += run; cur += run;
            k = sc.ss;
        } else if (sz == 0) {                          // ZRL
            if (p + (uint32_t)len > total_bits) { fail = JPEGD_ST_END; break; }
            p += (uint32_t)len;
            k += 16;
            if (k > sc.se) { k = sc.ss; ++done; ++cur; }
        } else {
            if (p + (uint32_t)(len + sz) > total_bits) { fail = JPEGD_ST_END; break; }
            k += r;
            if (k > sc.se) { fail = JPEGD_ST_ZIGZAG; break; }
            if (WRITE) {
                const long at = jpegdprog_place(g, sc, cur);
                if (at >= 0) coef[at * 64 + k] = (int16_t)(jpegdprog_extend(window, len, sz) * (1 << sc.al));
            }
            p += (uint32_t)(len + sz);
            if (++k > sc.se) { k = sc.ss; ++done; ++cur; }
        }
    }
    if (fail) {
        if (WRITE) status |= fail;
        s.p = JPEGD_INVALID; s.mz = 0;
        return;
    }
    s.p = p; s.mz = (uint32_t)m << 8 | (uint32_t)k;
}

// the state a restart interval (the scan) starts from
JPEGD_HD inline JpegdState jpegdprog_start(const JpegdProgScan& sc, uint32_t p) { return JpegdState{p, (uint32_t)sc.ss}; }

// The DC value of a block from the sum of the differences of its component since the interval's start: sum << Al into position 0;
// returns JPEGD_ST_DC for a value outside int16.  at: jpegdprog_place (-1: nothing is stored).
JPEGD_HD inline uint32_t jpegdprog_dc_store(int16_t* coef, long at, int sum, int al) {
    const long v = (long)sum * (1L << al);
    if (at >= 0) coef[at * 64] = (int16_t)v;
    return (v < -32768 || v > 32767) ? JPEGD_ST_DC : 0u;
}

// Block b of a DC refine scan: its bit is the (b - interval's first block)-th of its interval; a set bit ORs 1 << Al into position 0.
// ibit: the bit every interval of the scan begins at, ibit[K] = the end of the stream.  cg = jpegdprog_geo.  Returns status bits.
JPEGD_HD inline uint32_t jpegdprog_dc_refine_block(const uint32_t* bits, uint32_t nwords, const uint32_t* ibit, const JpegGeo& g,
                                                   const JpegGeo& cg, const JpegdProgScan& sc, uint32_t b, int16_t* coef) {
    const uint32_t per = jpegdprog_interval_blocks(cg), j = b / per, pos = ibit[j] + (b - j * per);
    if (pos < ibit[j] || pos >= ibit[j + 1u]) return JPEGD_ST_END;
    const long at = jpegdprog_place(g, sc, b);
    if (at >= 0 && (jpegd_peek(bits, nwords, pos) >> 31)) coef[at * 64] = (int16_t)(coef[at * 64] | (1 << sc.al));
    return 0u;
}

// one correction bit of an AC refine scan for the non-zero coefficient c
JPEGD_HD inline int16_t jpegdprog_correct(int c, uint32_t bit, int p1) {
    if (bit && (c & p1) == 0) c = c >= 0 ? c + p1 : c - p1;
    return (int16_t)c;
}

// One restart interval (the whole scan where there is none) of an AC refine scan, libjpeg's decode_mcu_AC_refine: the bits [p, end)
// over the `nblocks` consecutive blocks from blk on, read and updated in place, band Ss..Se only.  Returns status bits, 0 = decoded.
JPEGD_HD inline uint32_t jpegdprog_ac_refine_interval(const uint32_t* bits, uint32_t nwords, uint32_t p, uint32_t end, const JpegdTable& tab,
                                                      const JpegdProgScan& sc, int16_t* blk, uint32_t nblocks) {
    const int p1 = 1 << sc.al;
    uint32_t eobrun = 0;
    for (uint32_t b = 0; b < nblocks; ++b, blk += 64) {
        int k = sc.ss;
        if (eobrun == 0) {
            for (; k <= sc.se; ++k) {
                const uint32_t window = jpegd_peek(bits, nwords, p);
                int len;
                const int sym = jpegd_symbol(tab, window, len);
                if (sym < 0) return JPEGD_ST_CODE;
                const int sz = sym & 15;
                int r = sym >> 4, fresh = 0;
                if (sz) {
                    if (sz != 1) return JPEGD_ST_CATEGORY;
                    if (p + (uint32_t)len + 1u > end) return JPEGD_ST_END;
                    fresh = ((window << len) >> 31) ? p1 : -p1;
                    p += (uint32_t)len + 1u;
                } else if (r != 15) {
                    if (p + (uint32_t)(len + r) > end) return JPEGD_ST_END;
                    const uint32_t run = (1u << r) + (r ? (window << len) >> (32 - r) : 0u);
                    if (run > nblocks - b) return JPEGD_ST_RUN;
                    p += (uint32_t)(len + r);
                    eobrun = run;
                    break;
                } else {
                    if (p + (uint32_t)len > end) return JPEGD_ST_END;
                    p += (uint32_t)len;
                }
                // over the coefficients that are non-zero already, each with its correction bit, and r zeros
                do {
                    const int c = blk[k];
                    if (c != 0) {
                        if (p >= end) return JPEGD_ST_END;
                        blk[k] = jpegdprog_correct(c, jpegd_peek(bits, nwords, p) >> 31, p1);
                        ++p;
                    } else if (--r < 0) {
                        break;
                    }
                    ++k;
                } while (k <= sc.se);
                if (fresh) {
                    if (k > sc.se) return JPEGD_ST_ZIGZAG;
                    blk[k] = (int16_t)fresh;
                }
            }
        }
        if (eobrun > 0) {                              // inside a run: the rest of the band takes correction bits only
            for (; k <= sc.se; ++k) {
                const int c = blk[k];
                if (c == 0) continue;
                if (p >= end) return JPEGD_ST_END;
                blk[k] = jpegdprog_correct(c, jpegd_peek(bits, nwords, p) >> 31, p1);
                ++p;
            }
            --eobrun;
        }
    }
    return 0u;
}
