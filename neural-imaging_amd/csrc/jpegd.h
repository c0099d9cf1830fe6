// The sequential core of the baseline JPEG decoder: Huffman tables in libjpeg's maxcode / valptr form with an
// 8-bit lookahead, the place of a scan-order block in the coefficient tensor, and the function that decodes one subsequence of the
// un-stuffed bit stream from a state, counting or writing.  jpegd.hip runs it one thread per subsequence; everything here is
// `__host__ __device__` under hipcc and plain C++ otherwise, so that a host compiler can build it into a stand-alone program
// (tests/jpegd_host.cpp) and hold it to sanitizers.  No load leaves the bit buffer, no store leaves the block it belongs to.
#pragma once
#include <stdint.h>

#include "jpeg_geo.h"

#if defined(__HIPCC__)
#define JPEGD_HD __host__ __device__
#else
#define JPEGD_HD
#endif

// status bits of one image (0 = decoded)
#define JPEGD_ST_MARKER 1u        // an FF followed by anything but 00 inside the entropy-coded segment
#define JPEGD_ST_CODE 2u          // a bit pattern that is no code of the table in force
#define JPEGD_ST_ZIGZAG 4u        // a coefficient beyond zig-zag position 63
#define JPEGD_ST_CATEGORY 8u      // a DC category above 11 or an AC category above 10
#define JPEGD_ST_END 16u          // a symbol needs bits beyond the end of the stream
#define JPEGD_ST_BLOCKS 32u       // the stream holds fewer blocks than the scan has
#define JPEGD_ST_DC 64u           // a DC value outside int16
#define JPEGD_ST_TABLE 128u       // DHT counts that are no prefix code or name more than 256 symbols
#define JPEGD_ST_OFFSETS 256u     // segment offsets that descend or exceed what the workspace was sized for
#define JPEGD_ST_RESTART 512u     // restart markers missing, surplus or out of sequence (files with a restart interval, section 4i)

#define JPEGD_INVALID 0xffffffffu        // JpegdState::p of a decoder that met an invalid symbol
#define JPEGD_BLOCK_BITS_MAX 1728        // 64 x (16 + 11): no table makes a block longer
#define JPEGD_DHT_BYTES 272              // one table as the caller passes it: 16 counts, 256 symbols in code order

// one Huffman table.  Code `c` of length l > 8 is valid iff c <= maxcode[l]; its symbol is sym[(c + valoff[l]) & 255]
struct JpegdTable {
    int32_t maxcode[17];          // [l], l = 1..16: the largest code of length l, -1 if there is none
    int32_t valoff[17];           // [l]: index of the first symbol of length l minus its code
    uint16_t look[256];           // the next 8 bits -> length << 8 | symbol of a code of up to 8 bits, 0 for a longer one
    uint8_t sym[256];
};

// between two symbols: p = bit position in the un-stuffed stream (JPEGD_INVALID after an invalid symbol), mz = m << 8 | z with
// m = the block's index inside its MCU (selects the component) and z = the zig-zag position, 0 = a DC code comes next
struct JpegdState {
    uint32_t p, mz;
};

// false = `dht` is no prefix code or overflows the table; the table is then still safe to decode with
JPEGD_HD inline bool jpegd_build_table(const uint8_t* dht, JpegdTable* t) {
    bool ok = true;
    for (int i = 0; i < 256; ++i) { t->look[i] = 0; t->sym[i] = 0; }
    t->maxcode[0] = -1; t->valoff[0] = 0;
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        int cnt = dht[l - 1];
        if (k + cnt > 256) { ok = false; cnt = 256 - k; }
        if (cnt == 0) {
            t->maxcode[l] = -1; t->valoff[l] = 0;
        } else {
            if (code + cnt > (1 << l)) ok = false;
            t->valoff[l] = k - code;
            t->maxcode[l] = code + cnt - 1;
            for (int j = 0; j < cnt; ++j) {
                const uint8_t s = dht[16 + k + j];
                t->sym[k + j] = s;
                if (l <= 8)
                    for (int f = 0; f < (1 << (8 - l)); ++f) {
                        const int idx = ((code + j) << (8 - l)) + f;
                        if (idx < 256) t->look[idx] = (uint16_t)(l << 8 | s);
                    }
            }
        }
        k += cnt;
        code = (code + cnt) << 1;
    }
    return ok;
}

// the 32 bits from position p on, MSB first; bits beyond the buffer read as 0
JPEGD_HD inline uint32_t jpegd_peek(const uint32_t* bits, uint32_t nwords, uint32_t p) {
    const uint32_t i = p >> 5, sh = p & 31u;
    const uint32_t hi = i < nwords ? bits[i] : 0u, lo = (i + 1u < nwords && sh) ? bits[i + 1u] : 0u;
    return sh ? (hi << sh) | (lo >> (32u - sh)) : hi;
}

// the symbol at the head of `window` and its code length; -1 = no code
JPEGD_HD inline int jpegd_symbol(const JpegdTable& t, uint32_t window, int& len) {
    const uint32_t e = t.look[window >> 24];
    if (e) { len = (int)(e >> 8); return (int)(e & 255u); }
    for (int l = 9; l <= 16; ++l) {
        const int code = (int)(window >> (32 - l));
        if (code <= t.maxcode[l]) { len = l; return t.sym[(code + t.valoff[l]) & 255]; }
    }
    return -1;
}

// scan-order block b -> the offset (in blocks) of its coefficients in the image's [Y | Cb | Cr][row][col] tensor, -1 for a dummy
// block; comp = its component
JPEGD_HD inline long jpegd_place(const JpegGeo& g, uint32_t b, int& comp) {
    const int mcu = (int)(b / (uint32_t)g.per), k = (int)(b - (uint32_t)mcu * (uint32_t)g.per), ny = g.ny;
    if (k >= ny) {                                     // the chroma grid is the MCU grid
        comp = k - ny + 1;
        return (long)g.nbY + (long)(comp - 1) * g.nbC + mcu;
    }
    comp = 0;
    const int mr = mcu / g.mx, mc = mcu - mr * g.mx;
    const int br = mr * g.vs + (k >> g.hsh), bc = mc * g.hs + (k & (g.hs - 1));
    return (br < g.bhY && bc < g.bwY) ? (long)br * g.bwY + bc : -1;
}

// the scan-order index of the j-th block of component `comp` in an interleaved scan of MCUs of `per` blocks, the first ny of them luma
JPEGD_HD inline uint32_t jpegd_dc_block(int ny, int per, int comp, int j) {
    return comp ? (uint32_t)(j * per + ny + comp - 1) : (uint32_t)((j / ny) * per + j % ny);
}

// Decodes from state `s` until a symbol starts at or beyond `limit` (the caller passes min(next boundary, total_bits)) and leaves
// the exit state in `s`, the number of blocks begun (DC symbols met) in `begun`.  An invalid code, a category out of range and a
// symbol that runs beyond total_bits all end the run with s.p = JPEGD_INVALID.  The run belongs to one restart interval (the whole
// scan where the file has none): total_bits is the interval's end in the stream, [block_begin, block_end) its scan-order blocks.
// WRITE: `block` is the scan-order index of the first block begun here (the one in progress at entry is block - 1).  AC values go to
// coef (the image's tensor; real blocks only), DC differences to dcdiff[scan-order block], errors to `status`; the run ends after
// block block_end - 1 - what follows in the interval is skipped, as libjpeg skips it - and nothing outside the interval's blocks is
// stored.  Not WRITE: coef, dcdiff and status are not touched.
template <bool WRITE>
JPEGD_HD inline void jpegd_run_interval(const uint32_t* bits, uint32_t nwords, uint32_t total_bits, uint32_t limit, const JpegdTable* tabs,
                                        const JpegGeo& g, JpegdState& s, uint32_t& begun, uint32_t block, uint32_t block_begin,
                                        uint32_t block_end, int16_t* coef, int32_t* dcdiff, uint32_t& status) {
    begun = 0;
    uint32_t p = s.p;
    if (p == JPEGD_INVALID) return;
    int m = (int)(s.mz >> 8), z = (int)(s.mz & 255u);
    if (m >= g.per || z > 63) { s.p = JPEGD_INVALID; s.mz = 0; return; }        // never a state this function left
    const int ny = g.ny;
    uint32_t cur = block - (z ? 1u : 0u);              // WRITE: the block in progress, or the one the next DC code begins
    int16_t* dst = nullptr;                            // WRITE: the block in progress, if it is real
    if (WRITE && z) {
        if (block <= block_begin || cur >= block_end) return;
        int comp;
        const long at = jpegd_place(g, cur, comp);
        if (at >= 0) dst = coef + at * 64;
    }
    uint32_t fail = 0;
    while (p < limit) {
        if (WRITE && z == 0 && cur >= block_end) break;
        const int c = m < ny ? 0 : m - ny + 1;
        const uint32_t window = jpegd_peek(bits, nwords, p);
        int len;
        const int sym = jpegd_symbol(tabs[2 * c + (z ? 1 : 0)], window, len);
        if (sym < 0) { fail = JPEGD_ST_CODE; break; }
        const int sz = z ? (sym & 15) : sym, run = z ? (sym >> 4) : 0;
        if (sz > (z ? 10 : 11)) { fail = JPEGD_ST_CATEGORY; break; }
        if (p + (uint32_t)(len + sz) > total_bits) { fail = JPEGD_ST_END; break; }
        int v = 0;
        if (sz) {                                      // len + sz <= 27 bits of the window
            const int raw = (int)((window << len) >> (32 - sz));
            v = (raw >> (sz - 1)) ? raw : raw - (1 << sz) + 1;
        }
        p += (uint32_t)(len + sz);
        bool end = false;
        if (z == 0) {
            ++begun;
            if (WRITE) {
                int comp;
                const long at = jpegd_place(g, cur, comp);
                dcdiff[cur] = v;
                dst = at >= 0 ? coef + at * 64 : nullptr;
            }
            z = 1;
        } else if (sz == 0) {                          // ZRL, or end of block (libjpeg ends the block on every other run too)
            z += 16;
            end = run != 15 || z > 63;
        } else {
            z += run;
            if (z > 63) {
                if (WRITE) status |= JPEGD_ST_ZIGZAG;
                end = true;
            } else {
                if (WRITE && dst) dst[z] = (int16_t)v;
                end = ++z == 64;
            }
        }
        if (end) {
            z = 0;
            m = m + 1 == g.per ? 0 : m + 1;
            if (WRITE) { ++cur; dst = nullptr; }
        }
    }
    if (fail) {
        if (WRITE) status |= fail;
        s.p = JPEGD_INVALID; s.mz = 0;
        return;
    }
    s.p = p; s.mz = (uint32_t)m << 8 | (uint32_t)z;
}

// the run of a file without restart markers: one interval, the whole scan
template <bool WRITE>
JPEGD_HD inline void jpegd_run(const uint32_t* bits, uint32_t nwords, uint32_t total_bits, uint32_t limit, const JpegdTable* tabs,
                               const JpegGeo& g, JpegdState& s, uint32_t& begun, uint32_t block, int16_t* coef, int32_t* dcdiff,
                               uint32_t& status) {
    jpegd_run_interval<WRITE>(bits, nwords, total_bits, limit, tabs, g, s, begun, block, 0u, (uint32_t)g.SB, coef, dcdiff, status);
}

// ---- restart intervals -----------------------------------------------------------------------------
// An image with g.ri > 0 has K = jpegd_intervals(g) intervals and K - 1 markers.  Its interval table ibit[K + 1] holds the bit at
// which every interval begins in the un-stuffed stream, markers taken out; ibit[K] = the end of the stream.  Its subsequence table
// sub0[K + 1] holds the index of every interval's first subsequence; sub0[K] = the number of subsequences.
JPEGD_HD inline uint32_t jpegd_intervals(const JpegGeo& g) {
    return g.ri > 0 ? (uint32_t)((g.my * g.mx + g.ri - 1) / g.ri) : 1u;
}

// the marker FF `second` met as the idx-th of the image (from 0) after `kept` bytes of un-stuffed data: the start of interval
// idx + 1.  Returns JPEGD_ST_RESTART for a marker out of sequence or beyond the K - 1 the image has, else 0.
JPEGD_HD inline uint32_t jpegd_marker(uint32_t idx, uint32_t second, uint32_t kept, uint32_t K, uint32_t* ibit) {
    if (idx + 1u >= K) return JPEGD_ST_RESTART;
    ibit[idx + 1u] = 8u * kept;
    return (second & 7u) == (idx & 7u) ? 0u : JPEGD_ST_RESTART;
}

// subsequences of an interval of `len` bits: at least one, so that every interval has a first one
JPEGD_HD inline uint32_t jpegd_interval_subs(uint32_t len, uint32_t sb) { return len == 0 ? 1u : (len + sb - 1u) / sb; }

// the interval of subsequence i: the last k with sub0[k] <= i (i < sub0[K])
JPEGD_HD inline uint32_t jpegd_interval_of(const uint32_t* sub0, uint32_t K, uint32_t i) {
    uint32_t lo = 0, hi = K;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sub0[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// where subsequence i of an image with restart intervals stands
struct JpegdSpan {
    uint32_t k, j;                     // its interval, and its index inside it: 0 = its state at entry is known, (start, m 0, z 0)
    uint32_t start, limit, end;        // its first bit, the bit its last symbol starts before, the interval's end
    uint32_t block_begin, block_end;   // the interval's scan-order blocks
};
JPEGD_HD inline JpegdSpan jpegd_span(const JpegGeo& g, const uint32_t* ibit, const uint32_t* sub0, uint32_t K, uint32_t sb, uint32_t i) {
    JpegdSpan sp;
    sp.k = jpegd_interval_of(sub0, K, i);
    sp.j = i - sub0[sp.k];
    sp.end = ibit[sp.k + 1u];
    const uint32_t first = ibit[sp.k], room = sp.end - first;
    sp.start = sp.j < (room + sb - 1u) / sb ? first + sp.j * sb : sp.end;              // (never past the end, whatever the tables say)
    sp.limit = sp.end - sp.start > sb ? sp.start + sb : sp.end;
    const uint32_t per = g.ri > 0 ? (uint32_t)g.ri * (uint32_t)g.per : (uint32_t)g.SB;          // without an interval: the whole scan
    sp.block_begin = sp.k * per;
    sp.block_end = sp.block_begin + per < (uint32_t)g.SB ? sp.block_begin + per : (uint32_t)g.SB;
    return sp;
}
