// The sequential core of the JPEG entropy coders (DESIGN.md sections 4c and 4f): the symbols of one scan-order block - the one block
// walk of the baseline coder (jpegc.hip), the histogram and the coder with the caller's tables (jpegc_opt.hip) -, libjpeg's
// jpeg_gen_optimal_table over a 257-entry histogram, and the step from a table as a DHT segment has it to the code words the coder
// looks up.  The kernels run the block walk one thread per block and the length limiting and the derive step one thread per
// table; the merging jpegc_opt.hip does a wave per table, and jpegopt_optimal_table below is that merging in its sequential form.  Everything here
// is `__host__ __device__` under hipcc and plain C++ otherwise, so that a host compiler can build it into a stand-alone program
// (tests/jpegopt_host.cpp) and hold it to sanitizers.
#pragma once
#include <stdint.h>

#include "jpeg_geo.h"

#if defined(__HIPCC__)
#define JPEGOPT_HD __host__ __device__
#else
#define JPEGOPT_HD
#endif

#define JPEGOPT_HIST 257                 // one histogram: the 256 symbols and the pseudo-symbol that keeps the all-ones code unused
#define JPEGOPT_TABLE_BYTES 272          // one table: 16 counts, 256 symbols in code order (nimg_jpeg_decode's layout)
#define JPEGOPT_CODE_WORDS 544           // one image's code words: Y DC [16] | chroma DC [16] | Y AC [256] | chroma AC [256]
#define JPEGOPT_BLOCK_BITS_MAX 1665      // DC 16 + 11, 63 x (AC 16 + 10): no table makes a block longer

// nimg_jpeg_optimal_tables, per table
#define JPEGOPT_ST_OVERFLOW 1u           // a code size above 32 (libjpeg: "Huffman code size table overflow")
#define JPEGOPT_ST_TOTAL 2u              // a histogram total of 2^32 or more, the pseudo-symbol counted
// nimg_jpeg_encode_tables, per image
#define JPEGOPT_ST_TABLE 1u              // counts that are no prefix code of lengths 1..16 with at most 256 symbols
#define JPEGOPT_ST_SYMBOL 2u             // a symbol that occurs in the image has no code

JPEGOPT_HD inline int jpegopt_category(int a) {        // of |value|; 0 for 0
    return a ? 32 - __builtin_clz((unsigned)a) : 0;
}

// the DC of Y block k of MCU (mr, mc) as it is coded: a dummy block (beyond the real extent, to the right or below) carries the DC of
// the block before it in the MCU; block 0 of an MCU is always real
JPEGOPT_HD inline int jpegopt_y_dc(const int16_t* cy, const JpegGeo& g, int mr, int mc, int k, bool& real) {
    real = true;
    for (;; --k) {
        const int br = mr * g.vs + (k >> g.hsh), bc = mc * g.hs + (k & (g.hs - 1));
        if ((br < g.bhY && bc < g.bwY) || k == 0) return cy[((long)br * g.bwY + bc) * 64];
        real = false;
    }
}

// Scan block s of one image (ci: its coefficients, real blocks only) as the symbols nimg_jpeg_encode codes, with its clamps (DC
// difference +-2047, AC +-1023): sink.symbol(table, symbol, value bits, their number) with table = 0 Y DC, 1 Y AC, 2 chroma DC,
// 3 chroma AC - the DHT-id order 00 10 01 11.  A dummy block is its DC difference and one end-of-block.  The first block of a
// component in a restart interval (g.ri MCUs, section 4i) is predicted from 0, like the first of the image.
template <typename Sink>
JPEGOPT_HD inline void jpegopt_walk_block(const int16_t* ci, const JpegGeo& g, int s, Sink& sink) {
    const int m = s / g.per, k = s - m * g.per, mr = m / g.mx, mc = m - mr * g.mx, ny = g.ny;
    const int16_t* blk;
    int dc, pred, t;
    bool real = true;
    if (k < ny) {
        t = 0;
        bool other;
        dc = jpegopt_y_dc(ci, g, mr, mc, k, real);
        if (k > 0) pred = jpegopt_y_dc(ci, g, mr, mc, k - 1, other);
        else if (!jpeg_interval_start(g, m)) pred = jpegopt_y_dc(ci, g, (m - 1) / g.mx, (m - 1) % g.mx, ny - 1, other);
        else pred = 0;
        blk = ci + ((long)(mr * g.vs + (k >> g.hsh)) * g.bwY + mc * g.hs + (k & (g.hs - 1))) * 64;     // not read unless real
    } else {                       // the chroma grid is the MCU grid: block m, never a dummy
        t = 2;
        blk = ci + ((long)g.nbY + (long)(k - ny) * g.nbC + m) * 64;
        dc = blk[0];
        pred = jpeg_interval_start(g, m) ? 0 : blk[-64];
    }
    int diff = dc - pred;
    diff = diff < -2047 ? -2047 : (diff > 2047 ? 2047 : diff);
    int sz = jpegopt_category(__builtin_abs(diff));
    sink.symbol(t, sz, (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << sz) - 1u), sz);
    int run = 0;
    if (real) {
        for (int c = 0; c < 8; ++c) {
            uint32_t row[4];                           // eight coefficients, the even one in the low half (little endian)
            __builtin_memcpy(row, __builtin_assume_aligned(blk + 8 * c, 16), 16);
            for (int j = 0; j < 8; ++j) {
                if (c == 0 && j == 0) continue;
                int v = (int16_t)(row[j >> 1] >> (16 * (j & 1)));
                if (v == 0) { ++run; continue; }
                v = v < -1023 ? -1023 : (v > 1023 ? 1023 : v);
                while (run >= 16) {
                    sink.symbol(t + 1, 0xf0, 0u, 0);
                    run -= 16;
                }
                sz = jpegopt_category(__builtin_abs(v));
                sink.symbol(t + 1, (run << 4) | sz, (uint32_t)(v < 0 ? v - 1 : v) & ((1u << sz) - 1u), sz);
                run = 0;
            }
        }
    } else {
        run = 63;
    }
    if (run > 0) sink.symbol(t + 1, 0x00, 0u, 0);
}

// Annex K.3 on bits[0..32], the number of codes of every size: sizes above 16 are folded back, then the pseudo-symbol is taken out of
// the longest size in use.  No search runs below index 1.
JPEGOPT_HD inline void jpegopt_limit_bits(uint32_t* bits) {
    for (int i = 32; i > 16; --i)
        while (bits[i] > 0) {
            int j = i - 2;
            while (j > 1 && bits[j] == 0) --j;
            bits[i] -= 2;
            bits[i - 1] += 1;
            bits[j + 1] += 2;
            bits[j] -= 1;
        }
    int i = 16;
    while (i > 1 && bits[i] == 0) --i;
    if (bits[i] > 0) bits[i] -= 1;
}

// libjpeg's jpeg_gen_optimal_table: hist[257] (entry 256 is not read: the pseudo-symbol counts 1) -> table[272], the counts of the
// sizes 1..16 and the symbols ordered by their unlimited code size, then by value.  Returns the status; a table with a status, and the
// table of an all-zero histogram, is all zeros.  A symbol's tree is named by the entry that carries the tree's frequency.
JPEGOPT_HD inline uint32_t jpegopt_optimal_table(const uint32_t* hist, uint8_t* table) {
    for (int i = 0; i < JPEGOPT_TABLE_BYTES; ++i) table[i] = 0;
    uint64_t total = 1;
    for (int i = 0; i < 256; ++i) total += hist[i];
    if (total >= (1ull << 32)) return JPEGOPT_ST_TOTAL;
    if (total == 1) return 0;
    uint32_t freq[JPEGOPT_HIST];
    uint16_t size[JPEGOPT_HIST], tree[JPEGOPT_HIST];
    for (int i = 0; i < JPEGOPT_HIST; ++i) {
        freq[i] = i < 256 ? hist[i] : 1u;
        size[i] = 0;
        tree[i] = (uint16_t)i;
    }
    for (;;) {
        int c1 = -1, c2 = -1;                          // the smallest non-zero frequencies; of equal ones the largest index
        for (int i = 0; i < JPEGOPT_HIST; ++i)
            if (freq[i] && (c1 < 0 || freq[i] <= freq[c1])) c1 = i;
        for (int i = 0; i < JPEGOPT_HIST; ++i)
            if (freq[i] && i != c1 && (c2 < 0 || freq[i] <= freq[c2])) c2 = i;
        if (c2 < 0) break;
        freq[c1] += freq[c2];
        freq[c2] = 0;
        for (int i = 0; i < JPEGOPT_HIST; ++i)
            if (tree[i] == c1 || tree[i] == c2) {
                ++size[i];
                tree[i] = (uint16_t)c1;
            }
    }
    uint32_t bits[33];
    for (int i = 0; i <= 32; ++i) bits[i] = 0;
    for (int i = 0; i < JPEGOPT_HIST; ++i) {
        if (size[i] > 32) return JPEGOPT_ST_OVERFLOW;
        if (size[i]) ++bits[size[i]];
    }
    jpegopt_limit_bits(bits);
    for (int l = 1; l <= 16; ++l) table[l - 1] = (uint8_t)bits[l];
    int k = 0;
    for (int l = 1; l <= 32; ++l)
        for (int v = 0; v < 256; ++v)
            if (size[v] == l) table[16 + k++] = (uint8_t)v;
    return 0;
}

// One table as a DHT segment has it -> codes[nsym]: symbol -> code << 5 | length, 0 = no code; nsym = 16 for a DC table (larger
// symbols are left out), 256 for an AC table.  Of a symbol listed twice the last code counts.  false = the counts are no prefix code of
// lengths 1..16 or name more than 256 symbols (the decoder's check, jpegd_build_table); codes[] is then all zeros.
JPEGOPT_HD inline bool jpegopt_derive(const uint8_t* dht, uint32_t* codes, int nsym) {
    for (int i = 0; i < nsym; ++i) codes[i] = 0;
    uint32_t code = 0;
    int k = 0;
    bool ok = true;
    for (int l = 1; l <= 16 && ok; ++l) {
        const int cnt = dht[l - 1];
        if (k + cnt > 256 || code + (uint32_t)cnt > (1u << l)) { ok = false; break; }
        for (int j = 0; j < cnt; ++j) {
            const int s = dht[16 + k + j];
            if (s < nsym) codes[s] = (code + (uint32_t)j) << 5 | (uint32_t)l;
        }
        k += cnt;
        code = (code + (uint32_t)cnt) << 1;
    }
    if (!ok)
        for (int i = 0; i < nsym; ++i) codes[i] = 0;
    return ok;
}

// the tables an image's coder and histograms have: 00 10 01 11, or 00 10 alone in a grey-scale file
JPEGOPT_HD inline int jpegopt_tables(const JpegGeo& g) { return g.nc == 1 ? 2 : 4; }

// the n_tables (4, or 2 of a grey-scale file) tables of an image (DHT-id order 00 10 01 11) -> its JPEGOPT_CODE_WORDS code words, those
// of a table it has not all zero; false = one of them is refused, and all code words are zero
JPEGOPT_HD inline bool jpegopt_derive_image(const uint8_t* tables, uint32_t* codes, int n_tables = 4) {
    bool ok = jpegopt_derive(tables, codes, 16);
    ok = jpegopt_derive(tables + JPEGOPT_TABLE_BYTES, codes + 32, 256) && ok;
    if (n_tables == 4) {
        ok = jpegopt_derive(tables + 2 * JPEGOPT_TABLE_BYTES, codes + 16, 16) && ok;
        ok = jpegopt_derive(tables + 3 * JPEGOPT_TABLE_BYTES, codes + 288, 256) && ok;
    } else {
        for (int i = 0; i < 16; ++i) codes[16 + i] = 0;
        for (int i = 0; i < 256; ++i) codes[288 + i] = 0;
    }
    if (!ok)
        for (int i = 0; i < JPEGOPT_CODE_WORDS; ++i) codes[i] = 0;
    return ok;
}

// where the code word of (table, symbol) stands in an image's code words; a DC symbol is below 12
JPEGOPT_HD inline int jpegopt_code_index(int table, int symbol) {
    return (table & 1) ? 32 + (table >> 1) * 256 + symbol : (table >> 1) * 16 + symbol;
}
