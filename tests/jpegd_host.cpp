// Stand-alone host program around the sequential core of the JPEG decoder (neural-imaging_amd/csrc/jpegd.h): steps 1 to 6 of
// DESIGN.md section 4e run one after the other over the subsequences, exactly as the kernels of csrc/jpegd.hip order them.
// tests/test_jpegd_host.py builds it with -fsanitize=address,undefined and feeds it valid and damaged streams.
//   jpegd_host IN OUT SB [SB ...]        SB = subsequence bits, 0 = one subsequence as long as the stream
// IN:  uint32 count, then per stream: int32 h, w, hs, vs; uint32 len; 6 x 272 table bytes; len segment bytes (stuffed)
// OUT: per stream and setting: uint32 status, rounds, subsequences, ncoef; ncoef int16 coefficients (the device tensor of one image)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpegd.h"

struct Result {
    uint32_t status, rounds, subsequences;
    std::vector<int16_t> coef;
};

static Result decode(const JpegGeo& g, const uint8_t* huffman, const uint8_t* ecd, uint32_t len, uint32_t sb) {
    Result r;
    r.status = 0;
    JpegdTable tabs[6];
    for (int t = 0; t < 6; ++t)
        if (!jpegd_build_table(huffman + t * JPEGD_DHT_BYTES, tabs + t)) r.status |= JPEGD_ST_TABLE;
    // 1. un-stuff: exactly (len + 3) / 4 + 1 words, as the kernels size an image's buffer
    const uint32_t nwords = (len + 3) / 4 + 1;
    std::vector<uint32_t> bits(nwords, 0u);
    uint32_t kept = 0;
    for (uint32_t k = 0; k < len; ++k) {
        if (ecd[k] == 0xff && (k + 1 >= len || ecd[k + 1] != 0)) r.status |= JPEGD_ST_MARKER;
        if (ecd[k] == 0 && k > 0 && ecd[k - 1] == 0xff) continue;
        bits[kept >> 2] |= (uint32_t)ecd[k] << (24 - 8 * (kept & 3));
        ++kept;
    }
    const uint32_t total = 8 * kept;
    if (sb == 0) sb = total < 32 ? 32 : (total + 31) / 32 * 32;
    const uint32_t S = total == 0 ? 1 : (total + sb - 1) / sb;
    r.subsequences = S;
    auto limit = [&](uint32_t i) { const uint32_t e = (i + 1) * sb; return e < total ? e : total; };
    uint32_t unused = 0;
    // 2. speculate
    std::vector<JpegdState> exit(S);
    std::vector<uint32_t> cnt(S);
    for (uint32_t i = 0; i < S; ++i) {
        JpegdState s = {i * sb, 0};
        jpegd_run<false>(bits.data(), nwords, total, limit(i), tabs, g, s, cnt[i], 0, nullptr, nullptr, unused);
        exit[i] = s;
    }
    // 3. synchronise: every round reads the states of the round before
    r.rounds = 0;
    while (r.rounds + 1 < S) {
        ++r.rounds;
        const std::vector<JpegdState> before = exit;
        bool changed = false;
        for (uint32_t i = r.rounds; i < S; ++i) {
            JpegdState s = before[i - 1];
            jpegd_run<false>(bits.data(), nwords, total, limit(i), tabs, g, s, cnt[i], 0, nullptr, nullptr, unused);
            changed |= s.p != before[i].p || s.mz != before[i].mz;
            exit[i] = s;
        }
        if (!changed) break;
    }
    // 4. place
    uint32_t blocks = 0;
    for (uint32_t i = 0; i < S; ++i) {
        const uint32_t c = cnt[i];
        cnt[i] = blocks;
        blocks += c;
    }
    if (blocks < (uint32_t)g.SB) r.status |= JPEGD_ST_BLOCKS;
    // 5. write: buffers of exactly the size the device gives them
    r.coef.assign((size_t)g.NB * 64, 0);
    std::vector<int32_t> dcdiff(g.SB, 0);
    for (uint32_t i = 0; i < S; ++i) {
        JpegdState s = {0, 0};
        if (i) s = exit[i - 1];
        uint32_t begun;
        jpegd_run<true>(bits.data(), nwords, total, limit(i), tabs, g, s, begun, cnt[i], r.coef.data(), dcdiff.data(), r.status);
    }
    // 6. DC: libjpeg predicts through the dummy blocks
    int pred[3] = {0, 0, 0};
    for (uint32_t b = 0; b < (uint32_t)g.SB; ++b) {
        int comp;
        const long at = jpegd_place(g, b, comp);
        pred[comp] += dcdiff[b];
        if (pred[comp] < -32768 || pred[comp] > 32767) r.status |= JPEGD_ST_DC;
        if (at >= 0) r.coef[(size_t)at * 64] = (int16_t)pred[comp];
    }
    return r;
}

int main(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s IN OUT SB [SB ...]\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t count = 0;
    if (fread(&count, 4, 1, in) != 1) return 2;
    for (uint32_t k = 0; k < count; ++k) {
        int32_t head[4];
        uint32_t len;
        std::vector<uint8_t> huffman(6 * JPEGD_DHT_BYTES);
        if (fread(head, 4, 4, in) != 4 || fread(&len, 4, 1, in) != 1 || fread(huffman.data(), 1, huffman.size(), in) != huffman.size())
            return 2;
        std::vector<uint8_t> ecd(len);                 // exactly len bytes: a read past the segment is a sanitizer finding
        if (len && fread(ecd.data(), 1, len, in) != len) return 2;
        JpegGeo g;
        if (!make_geo(&g, 1, head[0], head[1], head[2], head[3])) return 2;
        for (int a = 3; a < argc; ++a) {
            const Result r = decode(g, huffman.data(), ecd.data(), len, (uint32_t)strtoul(argv[a], nullptr, 10));
            const uint32_t rec[4] = {r.status, r.rounds, r.subsequences, (uint32_t)r.coef.size()};
            fwrite(rec, 4, 4, out);
            fwrite(r.coef.data(), 2, r.coef.size(), out);
            printf("stream %u subseq_bits %s status %u rounds %u subsequences %u\n", k, argv[a], r.status, r.rounds, r.subsequences);
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
