// Stand-alone host program over the sequential core of the optimised-Huffman writer (csrc/jpegopt.h), built by
// tests/jpegopt_cases.py - with -fsanitize=address,undefined for test_jpegopt_host.py - and run as a process of its own.  Every buffer
// has exactly the size the device code gives it, so that a sanitizer sees any access beyond one.
//   jpegopt_host in.bin out.bin
// in.bin:  u32 m, u32 images, u32 given | m x 257 u32 histograms | per image: i32 h, w, hs, vs, u32 count, count x i16 coefficients
//          (the device layout, real blocks only) | given x 4 x 272 bytes of tables
// out.bin: m x 272 bytes of tables | m x u32 status | per image: 4 x 257 u32 histograms, 4 x 272 bytes of optimal tables, 4 x u32
//          status, u32 valid, 544 u32 code words | per given set: u32 valid, 544 u32 code words
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpegopt.h"

namespace {

struct Reader {
    std::vector<uint8_t> data;
    size_t at = 0;
    void take(void* dst, size_t n) {
        if (at + n > data.size()) { std::fprintf(stderr, "input too short\n"); std::exit(2); }
        std::memcpy(dst, data.data() + at, n);
        at += n;
    }
    uint32_t u32() { uint32_t v; take(&v, 4); return v; }
};

struct HistSink {
    uint32_t* hist;               // [4][257]
    void symbol(int table, int sym, uint32_t, int) { ++hist[table * JPEGOPT_HIST + sym]; }
};

void put(std::FILE* f, const void* p, size_t n) {
    if (n && std::fwrite(p, 1, n, f) != n) { std::fprintf(stderr, "write failed\n"); std::exit(2); }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: jpegopt_host in.bin out.bin\n"); return 2; }
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
    const uint32_t m = in.u32(), images = in.u32(), given = in.u32();

    std::vector<uint8_t> tables((size_t)m * JPEGOPT_TABLE_BYTES);
    std::vector<uint32_t> status(m);
    for (uint32_t k = 0; k < m; ++k) {
        std::vector<uint32_t> hist(JPEGOPT_HIST);
        std::vector<uint8_t> table(JPEGOPT_TABLE_BYTES);
        in.take(hist.data(), 4 * JPEGOPT_HIST);
        status[k] = jpegopt_optimal_table(hist.data(), table.data());
        std::memcpy(tables.data() + (size_t)k * JPEGOPT_TABLE_BYTES, table.data(), JPEGOPT_TABLE_BYTES);
    }
    put(out, tables.data(), tables.size());
    put(out, status.data(), 4 * status.size());

    for (uint32_t k = 0; k < images; ++k) {
        int dims[4];
        in.take(dims, 16);
        const int h = dims[0], w = dims[1], hs = dims[2], vs = dims[3];
        const uint32_t count = in.u32();
        JpegGeo g;
        if (!make_geo(&g, 1, h, w, hs, vs)) { std::fprintf(stderr, "image %u: no geometry\n", k); return 2; }
        if (count != (uint32_t)g.NB * 64u) { std::fprintf(stderr, "image %u: %u coefficients\n", k, count); return 2; }
        std::vector<int16_t> coef(count);
        in.take(coef.data(), 2 * (size_t)count);
        std::vector<uint32_t> hist(4 * JPEGOPT_HIST, 0u);
        HistSink sink{hist.data()};
        for (int s = 0; s < g.SB; ++s) jpegopt_walk_block(coef.data(), g, s, sink);
        std::vector<uint8_t> tabs(4 * JPEGOPT_TABLE_BYTES);
        uint32_t st[5];
        for (int t = 0; t < 4; ++t) st[t] = jpegopt_optimal_table(hist.data() + t * JPEGOPT_HIST, tabs.data() + t * JPEGOPT_TABLE_BYTES);
        std::vector<uint32_t> codes(JPEGOPT_CODE_WORDS);
        st[4] = jpegopt_derive_image(tabs.data(), codes.data()) ? 1u : 0u;
        put(out, hist.data(), 4 * hist.size());
        put(out, tabs.data(), tabs.size());
        put(out, st, sizeof st);
        put(out, codes.data(), 4 * codes.size());
    }

    for (uint32_t k = 0; k < given; ++k) {
        std::vector<uint8_t> tabs(4 * JPEGOPT_TABLE_BYTES);
        in.take(tabs.data(), tabs.size());
        std::vector<uint32_t> codes(JPEGOPT_CODE_WORDS);
        const uint32_t valid = jpegopt_derive_image(tabs.data(), codes.data()) ? 1u : 0u;
        put(out, &valid, 4);
        put(out, codes.data(), 4 * codes.size());
    }
    std::fclose(out);
    return 0;
}
