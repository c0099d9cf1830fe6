// Stand-alone host program around the sequential core of the progressive JPEG decoder (neural-imaging_amd/csrc/jpegdprog.h): the
// scans of a file decoded one after the other in buffers of exactly the sizes csrc/jpegd_prog.hip gives them, first scans through
// speculation, synchronisation rounds, placement and writing as the kernels order them.  tests/test_jpegdprog_host.py builds it with
// -fsanitize=address,undefined and feeds it valid and damaged streams.
//   jpegdprog_host IN OUT SB [SB ...]        SB = subsequence bits, 0 = one subsequence per restart interval
// IN:  uint32 count, then per image: int32 h, w, hs, vs, ri, n_scans; n_scans x 6 int32 (mask, Ss, Se, Ah, Al, level - the level is
//      ignored); per scan 3 x 272 table bytes, uint32 len, len segment bytes (stuffed, restart markers in place)
// OUT: per image: int32 legal (0 = the script breaks the rules: nothing follows), n_scans int32 levels; then per setting: uint32 status,
//      n_scans uint32 rounds, uint32 ncoef, ncoef int16 coefficients (the device tensor of one image)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpegdprog.h"

struct Segment {
    std::vector<uint8_t> tables, ecd;
};

// the segment without stuffing and restart markers, the bit every interval begins at, the flags - byte by byte what the prepare
// kernel decides from a byte and its two neighbours
static uint32_t unstuff(const std::vector<uint8_t>& ecd, bool rst, uint32_t K, std::vector<uint32_t>& bits, std::vector<uint32_t>& ibit,
                        uint32_t& total) {
    const uint32_t len = (uint32_t)ecd.size();
    auto at = [&](long k) { return k >= 0 && k < (long)len ? ecd[(size_t)k] : (uint8_t)1; };
    bits.assign((len + 3) / 4 + 1, 0u);
    ibit.assign(K + 1, 0u);
    uint32_t flags = 0, kept = 0, met = 0;
    for (long k = 0; k < (long)len; ++k) {
        const uint8_t b = at(k), before = at(k - 1), after = at(k + 1);
        if (rst && b == 0xff && (after & 0xf8) == 0xd0) { flags |= jpegd_marker(met++, after, kept, K, ibit.data()); continue; }
        if (rst && before == 0xff && (b & 0xf8) == 0xd0) continue;
        if (b == 0xff && after != 0) flags |= JPEGD_ST_MARKER;
        if (b == 0 && before == 0xff) continue;
        bits[kept >> 2] |= (uint32_t)b << (24 - 8 * (kept & 3));
        ++kept;
    }
    total = 8 * kept;
    if (rst && met + 1 != K) flags |= JPEGD_ST_RESTART;
    for (uint32_t k = (met < K - 1 ? met : K - 1) + 1; k <= K; ++k) ibit[k] = total;
    ibit[0] = 0;
    return flags;
}

static uint32_t first_scan(const JpegGeo& g, const JpegdProgScan& sc, const JpegdTable* tabs, const std::vector<uint32_t>& bits,
                           const std::vector<uint32_t>& ibit, uint32_t K, uint32_t sb, std::vector<int16_t>& coef, uint32_t& rounds) {
    const JpegGeo cg = jpegdprog_geo(g, sc);
    const uint32_t nwords = (uint32_t)bits.size();
    uint32_t status = 0, unused = 0;
    std::vector<uint32_t> sub0(K + 1);
    uint32_t S = 0, longest = 0;
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t subs = jpegd_interval_subs(ibit[k + 1] - ibit[k], sb);
        sub0[k] = S;
        S += subs;
        if (subs > longest) longest = subs;
    }
    sub0[K] = S;
    std::vector<JpegdState> exit(S);
    std::vector<uint32_t> cnt(S);
    auto run_count = [&](uint32_t i, JpegdState s) {
        const JpegdSpan sp = jpegd_span(cg, ibit.data(), sub0.data(), K, sb, i);
        jpegdprog_run_first<false>(bits.data(), nwords, sp.end, sp.limit, tabs, g, sc, cg.per, s, cnt[i], 0, 0, 0, nullptr, nullptr, unused);
        return s;
    };
    for (uint32_t i = 0; i < S; ++i) exit[i] = run_count(i, jpegdprog_start(sc, jpegd_span(cg, ibit.data(), sub0.data(), K, sb, i).start));
    rounds = 0;
    while (rounds + 1 < longest) {
        ++rounds;
        const std::vector<JpegdState> before = exit;
        bool changed = false;
        for (uint32_t i = rounds; i < S; ++i) {
            if (jpegd_span(cg, ibit.data(), sub0.data(), K, sb, i).j < rounds) continue;
            const JpegdState s = run_count(i, before[i - 1]);
            changed |= s.p != before[i].p || s.mz != before[i].mz;
            exit[i] = s;
        }
        if (!changed) break;
    }
    uint32_t blocks = 0;
    for (uint32_t i = 0; i < S; ++i) {
        const uint32_t c = cnt[i];
        cnt[i] = blocks;
        blocks += c;
    }
    const uint32_t per = jpegdprog_interval_blocks(cg);
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t have = (k + 1 < K ? cnt[sub0[k + 1]] : blocks) - cnt[sub0[k]], room = (uint32_t)cg.SB - k * per;
        if (have < (per < room ? per : room)) status |= JPEGD_ST_BLOCKS;
    }
    std::vector<int32_t> dcdiff(g.SB, 0);
    for (uint32_t i = 0; i < S; ++i) {
        const JpegdSpan sp = jpegd_span(cg, ibit.data(), sub0.data(), K, sb, i);
        JpegdState s = sp.j ? exit[i - 1] : jpegdprog_start(sc, sp.start);
        uint32_t done;
        jpegdprog_run_first<true>(bits.data(), nwords, sp.end, sp.limit, tabs, g, sc, cg.per, s, done, sp.block_begin + (cnt[i] - cnt[sub0[sp.k]]),
                                  sp.block_begin, sp.block_end, coef.data(), dcdiff.data(), status);
    }
    if (sc.ss == 0) {
        int pred[3] = {0, 0, 0};
        for (uint32_t b = 0; b < (uint32_t)cg.SB; ++b) {
            int comp = jpegdprog_comp(sc);
            if (sc.mask == 7) jpegd_place(g, b, comp);
            if (b % per == 0) pred[0] = pred[1] = pred[2] = 0;
            pred[comp] += dcdiff[jpegdprog_dc_slot(g, sc, b)];
            status |= jpegdprog_dc_store(coef.data(), jpegdprog_place(g, sc, b), pred[comp], sc.al);
        }
    }
    return status;
}

static uint32_t decode_scan(const JpegGeo& g, const JpegdProgScan& sc, const Segment& seg, uint32_t sb, std::vector<int16_t>& coef,
                            uint32_t& rounds) {
    const JpegGeo cg = jpegdprog_geo(g, sc);
    const uint32_t K = jpegd_intervals(cg), per = jpegdprog_interval_blocks(cg);
    uint32_t status = 0, total;
    JpegdTable tabs[3];
    for (int t = 0; t < 3; ++t)
        if (!jpegd_build_table(seg.tables.data() + t * JPEGD_DHT_BYTES, tabs + t)) status |= JPEGD_ST_TABLE;
    std::vector<uint32_t> bits, ibit;
    status |= unstuff(seg.ecd, g.ri != 0, K, bits, ibit, total);
    rounds = 0;
    if (sb == 0) sb = total < 32 ? 32 : (total + 31) / 32 * 32;
    if (jpegdprog_first(sc)) return status | first_scan(g, sc, tabs, bits, ibit, K, sb, coef, rounds);
    if (sc.ss == 0) {
        for (uint32_t b = 0; b < (uint32_t)cg.SB; ++b)
            status |= jpegdprog_dc_refine_block(bits.data(), (uint32_t)bits.size(), ibit.data(), g, cg, sc, b, coef.data());
        return status;
    }
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t b0 = k * per, b1 = b0 + per < (uint32_t)cg.SB ? b0 + per : (uint32_t)cg.SB;
        status |= jpegdprog_ac_refine_interval(bits.data(), (uint32_t)bits.size(), ibit[k], ibit[k + 1], tabs[0], sc,
                                               coef.data() + jpegdprog_place(g, sc, b0) * 64, b1 - b0);
    }
    return status;
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
        int32_t head[6];
        if (fread(head, 4, 6, in) != 6 || head[5] < 0 || head[5] > 1024) return 2;
        const int n_scans = head[5];
        std::vector<int32_t> script((size_t)n_scans * 6), levels(n_scans, 0);
        if (n_scans && fread(script.data(), 4, script.size(), in) != script.size()) return 2;
        std::vector<Segment> segs(n_scans);
        for (Segment& s : segs) {
            uint32_t len;
            s.tables.resize(3 * JPEGD_DHT_BYTES);
            if (fread(s.tables.data(), 1, s.tables.size(), in) != s.tables.size() || fread(&len, 4, 1, in) != 1) return 2;
            s.ecd.resize(len);                         // exactly len bytes: a read past the segment is a sanitizer finding
            if (len && fread(s.ecd.data(), 1, len, in) != len) return 2;
        }
        JpegGeo g;
        if (!make_geo(&g, 1, head[0], head[1], head[2], head[3]) || !set_restart(&g, head[4])) return 2;
        const int32_t legal = jpegdprog_check_script(script.data(), n_scans, levels.data()) ? 1 : 0;
        fwrite(&legal, 4, 1, out);
        if (!legal) continue;
        fwrite(levels.data(), 4, levels.size(), out);
        for (int a = 3; a < argc; ++a) {
            const uint32_t sb = (uint32_t)strtoul(argv[a], nullptr, 10);
            std::vector<int16_t> coef((size_t)g.NB * 64, 0);
            std::vector<uint32_t> rounds(n_scans, 0);
            uint32_t status = 0;
            // level after level, the scans of a level in file order: the order the device is free to take
            int top = 0;
            for (int s = 0; s < n_scans; ++s) top = levels[s] > top ? levels[s] : top;
            for (int l = 1; l <= top; ++l)
                for (int s = 0; s < n_scans; ++s) {
                    if (levels[s] != l) continue;
                    JpegdProgScan sc;
                    memcpy(&sc, script.data() + 6 * s, sizeof sc);
                    status |= decode_scan(g, sc, segs[s], sb, coef, rounds[s]);
                }
            const uint32_t ncoef = (uint32_t)coef.size();
            fwrite(&status, 4, 1, out);
            fwrite(rounds.data(), 4, rounds.size(), out);
            fwrite(&ncoef, 4, 1, out);
            fwrite(coef.data(), 2, coef.size(), out);
            printf("image %u subseq_bits %s status %u\n", k, argv[a], status);
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
