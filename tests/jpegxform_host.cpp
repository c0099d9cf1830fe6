// Host program over csrc/jpegxform.h: the sequential form of the lossless transforms, built by a host compiler with
// -fsanitize=address,undefined and run stand-alone by tests/jpegxform_cases.py.  Input and output are exactly-sized heap buffers, so a
// source or output block outside its tensor is an error the sanitizer reports.
//   in :  uint32 records; per record 14 int32 - kind (0 geometry, 1 run), n, h, w, hs, vs, nc, op, crop x, y, w, h, trim, values - and then
//         `values` int16 coefficients (n, source blocks, 64)
//   out:  per record int32 reason (JPEGXFORM_OK = 0, or why jpegxform_make refuses); where 0: int32 h', w', hs', vs', blocks per image
//         and, for a run, the (n, blocks, 64) int16 coefficients
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpegxform.h"

// the tables the kernel selects from are the closed forms' values: checked against a plain restatement before anything runs
static bool self_check() {
    int nat_of[64], k = 0;
    for (int d = 0; d < 15; ++d)
        for (int j = 0; j <= d; ++j) {
            const int v = (d & 1) ? j : d - j, u = d - v;
            if (v < 8 && u < 8) nat_of[k++] = 8 * v + u;
        }
    if (k != 64) return false;
    for (k = 0; k < 64; ++k) {
        if (jpegxform_natural(k) != nat_of[k]) return false;
        const int t = jpegxform_transposed(k);
        if (t < 0 || t > 63 || nat_of[t] != 8 * (nat_of[k] & 7) + (nat_of[k] >> 3)) return false;
        if ((int)((jpegxform_transposed_octet(k >> 3) >> (8 * (k & 7))) & 0xff) != t) return false;
        if ((int)(jpegxform_odd_mask(false) >> k & 1) != (nat_of[k] & 1) || (int)(jpegxform_odd_mask(true) >> k & 1) != (nat_of[k] >> 3 & 1))
            return false;
    }
    return jpegxform_negate(INT16_MIN) == INT16_MIN && jpegxform_negate(INT16_MAX) == -INT16_MAX && jpegxform_negate(0) == 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    if (!self_check()) {
        std::fprintf(stderr, "jpegxform.h: the closed forms disagree with the zig-zag scan\n");
        return 3;
    }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t records = 0;
    if (std::fread(&records, 4, 1, in) != 1) return 2;
    for (uint32_t rec = 0; rec < records; ++rec) {
        int32_t a[14];
        if (std::fread(a, 4, 14, in) != 14) return 2;
        const int kind = a[0], n = a[1];
        if (a[13] < 0) return 2;
        std::vector<int16_t> coef((size_t)a[13]);
        if (!coef.empty() && std::fread(coef.data(), 2, coef.size(), in) != coef.size()) return 2;
        JpegXform x;
        const int32_t reason = jpegxform_make(&x, a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12]);
        std::fwrite(&reason, 4, 1, out);
        if (reason != JPEGXFORM_OK) continue;
        const int32_t geo[5] = {x.h, x.w, x.hs, x.vs, x.NB};
        std::fwrite(geo, 4, 5, out);
        if (kind != 1) continue;
        if (n < 1 || coef.size() != (size_t)n * x.sNB * 64) return 2;
        std::vector<int16_t> result((size_t)n * x.NB * 64);
        jpegxform_run(x, coef.data(), n, result.data());
        std::fwrite(result.data(), 2, result.size(), out);
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 2;
}
