// Stand-alone host program over the sequential core of the progressive writer (csrc/jpegprog.h, with csrc/jpegopt.h's table
// construction and csrc/jpegrst.h's offsets and markers), built by tests/jpegprog_cases.py - with -fsanitize=address,undefined for
// test_jpegprog_host.py - and run as a process of its own.  It goes the device's way: histograms with the runs resolved over 256
// summaries at a time, optimal tables, code words, bit lengths, offsets, the bits of every block at its offset, stuffing.  Every buffer
// has exactly the size the device code gives it, so that a sanitizer sees any access beyond one.
//   jpegprog_host in.bin out.bin
// in.bin:  u32 images | per image: i32 h, w, hs, vs, restart interval, u32 given, u32 count, count x i16 coefficients (the device layout),
//          given ? 10 x 272 bytes of tables to code with : nothing (the optimal tables are used)
// out.bin: per image: 10 x 257 u32 histograms, 10 x 272 bytes of optimal tables, u32 status, 10 x u32 lengths, the ten segments
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpegprog.h"
#include "jpegrst.h"

namespace {

struct Reader {
    std::vector<uint8_t> data;
    size_t at = 0;
    void take(void* dst, size_t n) {
        if (at + n > data.size()) { std::fprintf(stderr, "input too short\n"); std::exit(2); }
        if (n) std::memcpy(dst, data.data() + at, n);
        at += n;
    }
    uint32_t u32() { uint32_t v; take(&v, 4); return v; }
};

void put(std::FILE* f, const void* p, size_t n) {
    if (n && std::fwrite(p, 1, n, f) != n) { std::fprintf(stderr, "write failed\n"); std::exit(2); }
}

struct HistSink {
    uint32_t* hist;               // [10][257]
    void symbol(int table, int sym, uint32_t, int) { ++hist[table * JPEGOPT_HIST + sym]; }
    void raw(uint64_t, int) {}
};
struct HistRec {
    uint32_t* hist;               // the scan's [257]
    void run(int, int length) { ++hist[jpegprog_run_category(length) << 4]; }
};

// bits into words, MSB first, at a bit offset; words == nullptr only counts.  No bounds check: the buffer has the device's size.
struct CodeSink {
    const uint32_t* codes;        // the image's JPEGPROG_CODE_WORDS
    uint32_t* words;
    uint32_t at, count = 0;
    bool missing = false;
    void bits(uint32_t v, int n) {
        count += (uint32_t)n;
        if (words)
            for (int i = n - 1; i >= 0; --i, ++at)
                if ((v >> i) & 1u) words[at >> 5] |= 0x80000000u >> (at & 31u);
    }
    void symbol(int table, int sym, uint32_t value, int nbits) {
        const uint32_t e = codes[jpegprog_code_base(table) + sym];
        if (e == 0) { missing = true; return; }
        bits(e >> 5, (int)(e & 31u));
        bits(value, nbits);
    }
    void raw(uint64_t v, int n) {
        for (int i = n - 1; i >= 0; --i) bits((uint32_t)(v >> i) & 1u, 1);
    }
};
struct LenRec {
    const uint32_t* codes;        // the scan's table
    uint32_t *len, *runs;
    bool missing;
    void run(int first, int length) {
        const int n = jpegprog_run_category(length);
        const uint32_t e = codes[n << 4];
        if (e == 0) { missing = true; return; }
        len[first] += (e & 31u) + (uint32_t)n;
        runs[first] = (uint32_t)length;
    }
};

template <typename Sink>
JpegProgTail walk(const int16_t* ci, const JpegGeo& g, const JpegProgScan& sc, int b, Sink& sink) {
    if (sc.cls == 0) {
        jpegprog_walk_dc(ci, g, b, sc.ah != 0, sc.al, sink);
        return JpegProgTail{0u, 0u};
    }
    return jpegprog_walk_ac(ci, g, sc, b, sink);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: jpegprog_host in.bin out.bin\n"); return 2; }
    Reader in;
    {
        std::FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        std::fseek(f, 0, SEEK_END);
        in.data.resize((size_t)std::ftell(f));
        std::fseek(f, 0, SEEK_SET);
        if (!in.data.empty() && std::fread(in.data.data(), 1, in.data.size(), f) != in.data.size()) return 2;
        std::fclose(f);
    }
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    const uint32_t images = in.u32();
    for (uint32_t k = 0; k < images; ++k) {
        int dims[5];
        in.take(dims, 20);
        const uint32_t given = in.u32(), count = in.u32();
        JpegGeo g;
        if (!make_geo(&g, 1, dims[0], dims[1], dims[2], dims[3]) || !set_restart(&g, dims[4])) {
            std::fprintf(stderr, "image %u: no geometry\n", k);
            return 2;
        }
        if (count != (uint32_t)g.NB * 64u) { std::fprintf(stderr, "image %u: %u coefficients\n", k, count); return 2; }
        std::vector<int16_t> coef(count);
        in.take(coef.data(), 2 * (size_t)count);

        // histograms: the runs resolved over 256 summaries at a time
        std::vector<uint32_t> hist(JPEGPROG_TABLES * JPEGOPT_HIST, 0u);
        for (int scan = 0; scan < JPEGPROG_SCANS; ++scan) {
            const JpegProgScan sc = jpegprog_scan(scan);
            const int nblk = jpegprog_class_blocks(g, sc.cls);
            HistSink sink{hist.data()};
            JpegProgRun state;
            for (int b0 = 0; b0 < nblk; b0 += 256) {
                const int cnt = nblk - b0 < 256 ? nblk - b0 : 256;
                std::vector<uint32_t> sums((size_t)cnt);
                for (int j = 0; j < cnt; ++j) sums[(size_t)j] = walk(coef.data(), g, sc, b0 + j, sink).summary;
                if (sc.cls == 0) continue;
                HistRec rec{hist.data() + sc.table * JPEGOPT_HIST};
                for (int j = 0; j < cnt; ++j) jpegprog_run_block(state, b0 + j, g.ri, sums[(size_t)j], rec);
                if (b0 + cnt == nblk) jpegprog_run_end(state, rec);
            }
        }
        std::vector<uint8_t> optimal(JPEGPROG_TABLES * JPEGOPT_TABLE_BYTES);
        for (int t = 0; t < JPEGPROG_TABLES; ++t) {
            std::vector<uint32_t> one(hist.begin() + t * JPEGOPT_HIST, hist.begin() + (t + 1) * JPEGOPT_HIST);
            std::vector<uint8_t> table(JPEGOPT_TABLE_BYTES);
            if (jpegopt_optimal_table(one.data(), table.data()) != 0) { std::fprintf(stderr, "image %u: table %d refused\n", k, t); return 2; }
            std::memcpy(optimal.data() + t * JPEGOPT_TABLE_BYTES, table.data(), JPEGOPT_TABLE_BYTES);
        }
        std::vector<uint8_t> tables(optimal);
        if (given) in.take(tables.data(), tables.size());

        // the coder
        std::vector<uint32_t> codes(JPEGPROG_CODE_WORDS);
        uint32_t status = jpegprog_derive_image(tables.data(), codes.data()) ? 0u : JPEGOPT_ST_TABLE;
        uint32_t lengths[JPEGPROG_SCANS];
        std::vector<uint8_t> segments;
        for (int scan = 0; scan < JPEGPROG_SCANS; ++scan) {
            const JpegProgScan sc = jpegprog_scan(scan);
            const JpegGeo c = jpegprog_class_geo(g, sc.cls);
            const int nblk = c.SB;
            const uint32_t* scan_codes = codes.data() + jpegprog_code_base(sc.table < 0 ? 0 : sc.table);
            std::vector<uint32_t> len((size_t)nblk, 0u), runs((size_t)nblk, 0u);
            if (!(status & JPEGOPT_ST_TABLE)) {
                JpegProgRun state;
                LenRec rec{scan_codes, len.data(), runs.data(), false};
                for (int b = 0; b < nblk; ++b) {
                    CodeSink sink{codes.data(), nullptr, 0u};
                    const JpegProgTail tail = walk(coef.data(), g, sc, b, sink);
                    len[(size_t)b] = sink.count + ((tail.summary & JPEGPROG_SUM_RUN) ? (uint32_t)tail.nbits() : 0u);
                    if (sink.missing) status |= JPEGOPT_ST_SYMBOL;
                    if (sc.cls != 0) jpegprog_run_block(state, b, g.ri, tail.summary, rec);
                }
                if (sc.cls != 0) jpegprog_run_end(state, rec);
                if (rec.missing) status |= JPEGOPT_ST_SYMBOL;
            }
            // offsets: the composition jpegc.hip scans
            std::vector<uint32_t> off((size_t)nblk);
            BitFn carry{0u, 0u, 0u};
            for (int b = 0; b < nblk; ++b) {
                off[(size_t)b] = carry.at(0u);
                carry = carry + jpegrst_block_fn(len[(size_t)b], c, b);
            }
            const uint32_t total = carry.at(0u), nbytes = (total + 7u) / 8u;
            const unsigned raw_words = jpegprog_raw_words(c, sc.cls);
            if ((nbytes + 3u) / 4u > raw_words) {
                std::fprintf(stderr, "image %u scan %d: %u bytes in %u words\n", k, scan, nbytes, raw_words);
                return 2;
            }
            std::vector<uint32_t> raw(raw_words, 0u);
            if (!(status & JPEGOPT_ST_TABLE))
                for (int b = 0; b < nblk; ++b) {
                    CodeSink sink{codes.data(), raw.data(), off[(size_t)b]};
                    const JpegProgTail tail = walk(coef.data(), g, sc, b, sink);
                    if (sc.cls != 0) jpegprog_block_end(tail, sc.table, (int)runs[(size_t)b], sink);
                    if (sink.count != len[(size_t)b]) {
                        std::fprintf(stderr, "image %u scan %d block %d: %u bits, %u counted\n", k, scan, b, sink.count, len[(size_t)b]);
                        return 2;
                    }
                    const int pad = jpegrst_pad_bits(c, b, off[(size_t)b] + sink.count);
                    if (pad) sink.bits((1u << pad) - 1u, pad);
                }
            const size_t before = segments.size();
            for (uint32_t pos = 0; pos < nbytes; ++pos) {
                const uint32_t byte = (raw[pos >> 2] >> (24 - 8 * (pos & 3u))) & 0xffu;
                const uint32_t mark = c.ri ? jpegrst_marker_byte(off.data(), c, jpegrst_first_marker(off.data(), c, pos & ~3u), pos) : 0u;
                segments.push_back((uint8_t)(mark ? mark : byte));
                if (byte == 0xffu) segments.push_back(0);
            }
            lengths[scan] = (uint32_t)(segments.size() - before);
        }
        put(out, hist.data(), 4 * hist.size());
        put(out, optimal.data(), optimal.size());
        put(out, &status, 4);
        put(out, lengths, sizeof lengths);
        put(out, segments.data(), segments.size());
    }
    std::fclose(out);
    return 0;
}
