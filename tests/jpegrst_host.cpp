// Stand-alone host program around the sequential cores of the JPEG codec with restart intervals:
// neural-imaging_amd/csrc/jpegd.h - the interval table and marker check, the per-interval run - in steps 1 to 6 of section 4e as
// csrc/jpegd.hip orders them, and csrc/jpegopt.h + jpegrst.h - the block walk with restarting predictors, the offset scan's
// functions, the padding rule, the marker placement - as csrc/jpegc.hip orders the writer's passes.  Every buffer has exactly the
// size the device gives it.  tests/test_jpegrst_host.py builds it with -fsanitize=address,undefined and feeds it valid and damaged
// streams.
//   jpegrst_host IN OUT SB [SB ...]        SB = subsequence bits, 0 = subsequences as long as the stream
// IN:  uint32 count, then per stream: int32 h, w, hs, vs, ri; uint32 len; 6 x 272 table bytes; len segment bytes (stuffed, with markers)
// OUT: per stream: per setting uint32 status, rounds, subsequences, ncoef and ncoef int16 coefficients (the device tensor of one
//      image); then uint32 recoded: 1 = the coefficients of the first setting, coded again with the stream's tables and interval,
//      are the stream byte for byte, 0 = they are not, 2 = not tried (a status bit is set)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpegd.h"
#include "jpegopt.h"
#include "jpegrst.h"

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
    // 1. un-stuff, take the markers out, fill the interval table: (len + 3) / 4 + 1 words and K + 1 entries, as the kernels size them
    const bool rst = g.ri > 0;
    const uint32_t K = jpegd_intervals(g), nwords = (len + 3) / 4 + 1;
    std::vector<uint32_t> bits(nwords, 0u), ibit(K + 1), sub0(K + 1);
    uint32_t kept = 0, met = 0;
    for (uint32_t k = 0; k < len; ++k) {
        const uint8_t b = ecd[k], next = k + 1 < len ? ecd[k + 1] : 1, prev = k > 0 ? ecd[k - 1] : 1;
        if (rst && b == 0xff && (next & 0xf8) == 0xd0) { r.status |= jpegd_marker(met++, next, kept, K, ibit.data()); continue; }
        if (rst && prev == 0xff && (b & 0xf8) == 0xd0) continue;
        if (b == 0xff && next != 0) r.status |= JPEGD_ST_MARKER;
        if (b == 0 && prev == 0xff) continue;
        bits[kept >> 2] |= (uint32_t)b << (24 - 8 * (kept & 3));
        ++kept;
    }
    const uint32_t total = 8 * kept;
    if (met + 1 != K) r.status |= JPEGD_ST_RESTART;
    ibit[0] = 0;
    for (uint32_t k = (met < K - 1 ? met : K - 1) + 1; k <= K; ++k) ibit[k] = total;
    if (sb == 0) sb = total < 32 ? 32 : (total + 31) / 32 * 32;
    uint32_t S = 0, longest = 0;
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t subs = jpegd_interval_subs(ibit[k + 1] - ibit[k], sb);
        sub0[k] = S;
        S += subs;
        longest = subs > longest ? subs : longest;
    }
    sub0[K] = S;
    r.subsequences = S;
    uint32_t unused = 0;
    // 2. speculate: the first subsequence of an interval starts from its true state
    std::vector<JpegdState> exit(S);
    std::vector<uint32_t> cnt(S);
    for (uint32_t i = 0; i < S; ++i) {
        const JpegdSpan sp = jpegd_span(g, ibit.data(), sub0.data(), K, sb, i);
        JpegdState s = {sp.start, 0};
        jpegd_run_interval<false>(bits.data(), nwords, sp.end, sp.limit, tabs, g, s, cnt[i], 0, 0, 0, nullptr, nullptr, unused);
        exit[i] = s;
    }
    // 3. synchronise: every round reads the states of the round before; after round r the subsequences 0 .. r of every interval are true
    r.rounds = 0;
    while (r.rounds + 1 < longest) {
        ++r.rounds;
        const std::vector<JpegdState> before = exit;
        bool changed = false;
        for (uint32_t i = r.rounds; i < S; ++i) {
            const JpegdSpan sp = jpegd_span(g, ibit.data(), sub0.data(), K, sb, i);
            if (sp.j < r.rounds) continue;
            JpegdState s = before[i - 1];
            jpegd_run_interval<false>(bits.data(), nwords, sp.end, sp.limit, tabs, g, s, cnt[i], 0, 0, 0, nullptr, nullptr, unused);
            changed |= s.p != before[i].p || s.mz != before[i].mz;
            exit[i] = s;
        }
        if (!changed) break;
    }
    // 4. place: one sum over the image; every interval must have begun its own blocks
    uint32_t blocks = 0;
    for (uint32_t i = 0; i < S; ++i) {
        const uint32_t c = cnt[i];
        cnt[i] = blocks;
        blocks += c;
    }
    const uint32_t per = rst ? (uint32_t)g.ri * (uint32_t)g.per : (uint32_t)g.SB;
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t begun = (k + 1 < K ? cnt[sub0[k + 1]] : blocks) - cnt[sub0[k]], own = (uint32_t)g.SB - k * per;
        if (begun < (per < own ? per : own)) r.status |= JPEGD_ST_BLOCKS;
    }
    // 5. write: buffers of exactly the size the device gives them
    r.coef.assign((size_t)g.NB * 64, 0);
    std::vector<int32_t> dcdiff(g.SB, 0);
    for (uint32_t i = 0; i < S; ++i) {
        const JpegdSpan sp = jpegd_span(g, ibit.data(), sub0.data(), K, sb, i);
        JpegdState s = {sp.start, 0};
        if (sp.j) s = exit[i - 1];
        uint32_t begun;
        jpegd_run_interval<true>(bits.data(), nwords, sp.end, sp.limit, tabs, g, s, begun, sp.block_begin + (cnt[i] - cnt[sub0[sp.k]]),
                                 sp.block_begin, sp.block_end, r.coef.data(), dcdiff.data(), r.status);
    }
    // 6. DC: libjpeg predicts through the dummy blocks, from 0 in every interval
    int pred[3] = {0, 0, 0};
    for (uint32_t b = 0; b < (uint32_t)g.SB; ++b) {
        if (b % (uint32_t)g.per == 0 && jpeg_interval_start(g, (int)(b / (uint32_t)g.per))) pred[0] = pred[1] = pred[2] = 0;
        int comp;
        const long at = jpegd_place(g, b, comp);
        pred[comp] += dcdiff[b];
        if (pred[comp] < -32768 || pred[comp] > 32767) r.status |= JPEGD_ST_DC;
        if (at >= 0) r.coef[(size_t)at * 64] = (int16_t)pred[comp];
    }
    return r;
}

// the bit sink of the host: counts, or ORs its bits into a zeroed buffer of `cap` words, never beyond it
struct HostSink {
    const uint32_t* codes;
    uint32_t* raw;
    uint32_t cap, pos, count;
    bool missing;
    void put(uint32_t v, int len) {
        count += (uint32_t)len;
        if (!raw) return;
        for (int k = len - 1; k >= 0; --k, ++pos)
            if ((v >> k & 1u) && (pos >> 5) < cap) raw[pos >> 5] |= 0x80000000u >> (pos & 31u);
    }
    void symbol(int table, int sym, uint32_t value, int nbits) {
        const uint32_t e = codes[jpegopt_code_index(table, sym)];
        if (e == 0) { missing = true; return; }
        put(((e >> 5) << nbits) | value, (int)(e & 31u) + nbits);
    }
};

// the writer's passes over one image: bit lengths | offsets by the composed functions | emit with the padding | count and scatter
static bool recode(const JpegGeo& g, const uint8_t* huffman, const std::vector<int16_t>& coef, const uint8_t* ecd, uint32_t len) {
    std::vector<uint32_t> codes(JPEGOPT_CODE_WORDS);
    // the first four tables - Y DC, Y AC, Cb DC, Cb AC - are the image's in DHT-id order 00 10 01 11
    if (!jpegopt_derive_image(huffman, codes.data())) return false;
    std::vector<uint32_t> off(g.SB);
    for (int s = 0; s < g.SB; ++s) {
        HostSink sink = {codes.data(), nullptr, 0, 0, 0, false};
        jpegopt_walk_block(coef.data(), g, s, sink);
        if (sink.missing) return false;
        off[s] = sink.count;
    }
    BitFn run = {0, 0, 0};
    for (int s = 0; s < g.SB; ++s) {
        const BitFn f = jpegrst_block_fn(off[s], g, s);
        off[s] = run.at(0);
        run = run + f;
    }
    const uint32_t total = run.at(0);
    const unsigned long words = ((unsigned long)g.SB * JPEGOPT_BLOCK_BITS_MAX + 23ul * (unsigned long)jpeg_markers(g) + 31) / 32 + 1;
    const uint32_t raw_words = (uint32_t)((words + 3) & ~3ul);
    std::vector<uint32_t> raw(raw_words, 0u);
    for (int s = 0; s < g.SB; ++s) {
        HostSink sink = {codes.data(), raw.data(), raw_words, off[s], 0, false};
        jpegopt_walk_block(coef.data(), g, s, sink);
        const int pad = jpegrst_pad_bits(g, s, off[s] + sink.count);
        if (pad) sink.put((1u << pad) - 1u, pad);
    }
    const uint32_t nbytes = (total + 7) / 8;
    std::vector<uint8_t> out;
    for (uint32_t pos = 0; pos < nbytes; ++pos) {
        const uint32_t byte = (pos >> 2) < raw_words ? (raw[pos >> 2] >> (24 - 8 * (pos & 3))) & 0xffu : 0u;
        const uint32_t mark = g.ri ? jpegrst_marker_byte(off.data(), g, jpegrst_first_marker(off.data(), g, pos & ~3u), pos) : 0u;
        out.push_back((uint8_t)(mark ? mark : byte));
        if (byte == 0xff) out.push_back(0);
    }
    return out.size() == len && (len == 0 || memcmp(out.data(), ecd, len) == 0);
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
        int32_t head[5];
        uint32_t len;
        std::vector<uint8_t> huffman(6 * JPEGD_DHT_BYTES);
        if (fread(head, 4, 5, in) != 5 || fread(&len, 4, 1, in) != 1 || fread(huffman.data(), 1, huffman.size(), in) != huffman.size())
            return 2;
        std::vector<uint8_t> ecd(len);                 // exactly len bytes: a read past the segment is a sanitizer finding
        if (len && fread(ecd.data(), 1, len, in) != len) return 2;
        JpegGeo g;
        if (!make_geo(&g, 1, head[0], head[1], head[2], head[3]) || !set_restart(&g, head[4])) return 2;
        uint32_t recoded = 2;
        for (int a = 3; a < argc; ++a) {
            const Result r = decode(g, huffman.data(), ecd.data(), len, (uint32_t)strtoul(argv[a], nullptr, 10));
            const uint32_t rec[4] = {r.status, r.rounds, r.subsequences, (uint32_t)r.coef.size()};
            fwrite(rec, 4, 4, out);
            fwrite(r.coef.data(), 2, r.coef.size(), out);
            uint32_t hash = 2166136261u;               // FNV-1a over the coefficient bytes
            for (size_t i = 0; i < r.coef.size(); ++i) {
                hash = (hash ^ ((uint16_t)r.coef[i] & 0xffu)) * 16777619u;
                hash = (hash ^ ((uint16_t)r.coef[i] >> 8)) * 16777619u;
            }
            printf("stream %u subseq_bits %s status %u rounds %u subsequences %u coefficients %08x\n", k, argv[a], r.status, r.rounds,
                   r.subsequences, hash);
            if (a == 3 && r.status == 0) recoded = recode(g, huffman.data(), r.coef, ecd.data(), len) ? 1u : 0u;
        }
        fwrite(&recoded, 4, 1, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
