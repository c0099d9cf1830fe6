// Stand-alone host program that holds the sequential cores of the JPEG reader to the WIDE set of sampling factors (DESIGN.md section 4r:
// luma 1x2, 4x1, 4x2, 1x4, 2x4 next to 1x1, 2x1, 2x2, over 1x1 chroma).  JPEG_FACTORS_DEFAULT makes every make_geo of the cores admit
// that set; what is compiled is chosen by a macro, so that the programs around jpegd.h / jpegopt.h / jpegrst.h and around jpegdprog.h are
// their siblings' to the letter, arguments and file formats included:
//   -DJPEGSAMP_RST     tests/jpegrst_host.cpp: baseline files with or without restart intervals, decoded in the order of csrc/jpegd.hip
//                      and coded again by the walks of csrc/jpegopt.h
//   -DJPEGSAMP_PROG    tests/jpegdprog_host.cpp: progressive files of any script
//   neither            the program below: the geometry (csrc/jpeg_geo.h, csrc/jpegscale.h) and the reconstruction at scale 1, 2, 4, 8 over
//                      buffers of exactly the size the device gives them.  What the device takes from csrc/jpegc.h (HIP only) is restated in
//                      plain C++: the 8 x 8 inverse DCT, the full-size h1v2 filter and replication, the colour conversion.
//   jpegsamp_host IN OUT
//   IN:  uint32 count, then per job: int32 kind (0 = geometry, 1 = image), h, w, hs, vs, scale; for an image 3 x 64 uint16 tables in
//        natural order and real blocks x 64 int16 coefficients in the layout of the device tensor
//   OUT: geometry: int32 admitted by the three, admitted by the wide set, then (if the wide set admits it) per, ny, SB, my, mx, bhY, bwY,
//        bhC, bwC, ceh, cew, nbY, nbC, NB, hsh, and for scale 2, 4, 8: ok, nY, nC, ehC, ewC, rx, ry, mode, oh, ow
//        image: (ceil(h / scale), ceil(w / scale), 3) uint8
// Exit status 2: a file could not be read or written; 3: a geometry or scale the core refuses.
#define JPEG_FACTORS_DEFAULT JPEG_FACTORS_WIDE
#if defined(JPEGSAMP_RST)
#include "jpegrst_host.cpp"
#elif defined(JPEGSAMP_PROG)
#include "jpegdprog_host.cpp"
#else
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "jpegscale.h"

static int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jidctint over 8 values S apart (csrc/jpegc.h idct8)
static void idct8(int* d, int S, int n) {
    int z1 = (d[2 * S] + d[6 * S]) * 4433;
    const int t2 = z1 - d[6 * S] * 15137, t3 = z1 + d[2 * S] * 6270;
    const int t0 = (d[0] + d[4 * S]) * 8192, t1 = (d[0] - d[4 * S]) * 8192;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a0 = d[7 * S], a1 = d[5 * S], a2 = d[3 * S], a3 = d[S];
    z1 = a0 + a3;
    int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int z5 = (z3 + z4) * 9633;
    a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    d[0] = descale(t10 + a3, n); d[7 * S] = descale(t10 - a3, n);
    d[S] = descale(t11 + a2, n); d[6 * S] = descale(t11 - a2, n);
    d[2 * S] = descale(t12 + a1, n); d[5 * S] = descale(t12 - a1, n);
    d[3 * S] = descale(t13 + a0, n); d[4 * S] = descale(t13 - a0, n);
}

struct Block {
    const int16_t* c;
    int operator()(int k) const { return c[k]; }
};

static void block_samples(int N, const int16_t* c, const uint16_t* q, int* d) {
    const Block b{c};
    if (N == 1) jpegscale_idct<1>(b, q, d);
    else if (N == 2) jpegscale_idct<2>(b, q, d);
    else if (N == 4) jpegscale_idct<4>(b, q, d);
    else {
        for (int nat = 0; nat < 64; ++nat) d[nat] = c[jpegscale_zz_of_nat(nat)] * (int)q[nat];
        for (int col = 0; col < 8; ++col) idct8(d + col, 8, 11);
        for (int row = 0; row < 8; ++row) idct8(d + 8 * row, 1, 18);
        for (int k = 0; k < 64; ++k) d[k] = jpegscale_limit(d[k] + 128);
    }
}

static void put(FILE* out, std::initializer_list<int32_t> v) {
    for (int32_t x : v) fwrite(&x, 4, 1, out);
}

static void geometry(FILE* out, int h, int w, int hs, int vs) {
    JpegGeo g;
    const bool three = make_geo(&g, 1, h, w, hs, vs, 3, JPEG_FACTORS_THREE), wide = make_geo(&g, 1, h, w, hs, vs);
    put(out, {three, wide});
    if (!wide) return;
    put(out, {g.per, g.ny, g.SB, g.my, g.mx, g.bhY, g.bwY, g.bhC, g.bwC, g.ceh, g.cew, g.nbY, g.nbC, g.NB, g.hsh});
    for (int s = 2; s <= 8; s *= 2) {
        JpegScaleGeo sg;
        memset(&sg, 0, sizeof sg);
        const bool ok = make_scale_geo(&sg, g, s);
        put(out, {ok, sg.nY, sg.nC, sg.ehC, sg.ewC, sg.rx, sg.ry, sg.mode, sg.oh, sg.ow});
    }
}

static int colour(int yy, int cb, int cr, int k) {
    cb -= 128; cr -= 128;
    return jpegscale_limit(k == 0 ? yy + ((91881 * cr + 32768) >> 16)
                                  : k == 1 ? yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16) : yy + ((116130 * cb + 32768) >> 16));
}

// the chroma sample of full-size pixel (y, x) for the five samplings: csrc/jpegc.h chroma_h1v2_at and chroma_replicated_at
static int full_chroma(const uint8_t* p, const JpegGeo& g, int y, int x) {
    const int stride = 8 * g.bwC;
    if (g.hs == 1 && g.vs == 2) {
        const int j = y >> 1, nb = (y & 1) ? (j + 1 < g.ceh ? j + 1 : g.ceh - 1) : (j > 0 ? j - 1 : 0);
        return (3 * p[(size_t)j * stride + x] + p[(size_t)nb * stride + x] + 1 + (y & 1)) >> 2;
    }
    return p[(size_t)(y / g.vs) * stride + (x >> g.hsh)];
}

static bool image(FILE* in, FILE* out, int h, int w, int hs, int vs, int scale) {
    JpegGeo g;
    if (!make_geo(&g, 1, h, w, hs, vs) || jpeg_factors_ok(hs, vs, JPEG_FACTORS_THREE)) exit(3);        // the five: the three have their own
    std::vector<uint16_t> qtabs(3 * 64);
    std::vector<int16_t> coef((size_t)g.NB * 64);
    if (fread(qtabs.data(), 2, qtabs.size(), in) != qtabs.size() || fread(coef.data(), 2, coef.size(), in) != coef.size()) return false;
    JpegScaleGeo sg;
    if (scale == 1) {                                          // csrc/jpegc.h: planes over the real blocks, N = 8
        memset(&sg, 0, sizeof sg);
        sg.nY = sg.nC = 8; sg.oh = h; sg.ow = w; sg.strideY = 8 * g.bwY; sg.strideC = 8 * g.bwC;
        sg.planeY = (size_t)g.nbY * 64; sg.planeC = (size_t)g.nbC * 64; sg.per = (size_t)g.NB * 64;
    } else if (!make_scale_geo(&sg, g, scale)) exit(3);
    std::vector<uint8_t> planes(sg.per, 0);
    for (int t = 0; t < g.NB; ++t) {
        int b = t, comp = 0;
        if (b >= g.nbY) {
            b -= g.nbY;
            comp = b < g.nbC ? 1 : 2;
            b -= (comp - 1) * g.nbC;
        }
        const int bw = comp ? g.bwC : g.bwY, br = b / bw, bc = b - br * bw;
        const int N = comp ? sg.nC : sg.nY, stride = comp ? sg.strideC : sg.strideY;
        int d[64];
        block_samples(N, coef.data() + (size_t)t * 64, qtabs.data() + comp * 64, d);
        uint8_t* p = planes.data() + jpegscale_plane_offset(sg, 0, comp) + (size_t)(N * br) * stride + N * bc;
        for (int r = 0; r < N; ++r)
            for (int c = 0; c < N; ++c) p[(size_t)r * stride + c] = (uint8_t)d[N * r + c];
    }
    std::vector<uint8_t> px((size_t)sg.oh * sg.ow * 3);
    const uint8_t* pb = planes.data() + jpegscale_plane_offset(sg, 0, 1);
    const uint8_t* pr = pb + sg.planeC;
    for (int y = 0; y < sg.oh; ++y)
        for (int x = 0; x < sg.ow; ++x) {
            const int yy = planes[(size_t)y * sg.strideY + x];
            const int cb = scale == 1 ? full_chroma(pb, g, y, x) : jpegscale_chroma_at(pb, sg, y, x);
            const int cr = scale == 1 ? full_chroma(pr, g, y, x) : jpegscale_chroma_at(pr, sg, y, x);
            for (int k = 0; k < 3; ++k) px[((size_t)y * sg.ow + x) * 3 + k] = (uint8_t)colour(yy, cb, cr, k);
        }
    return fwrite(px.data(), 1, px.size(), out) == px.size();
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    uint32_t count = 0;
    bool ok = in && out && fread(&count, 4, 1, in) == 1;
    for (uint32_t k = 0; ok && k < count; ++k) {
        int32_t head[6];
        ok = fread(head, 4, 6, in) == 6;
        if (!ok) break;
        if (head[0] == 0) geometry(out, head[1], head[2], head[3], head[4]);
        else ok = image(in, out, head[1], head[2], head[3], head[4], head[5]);
    }
    if (in) fclose(in);
    if (out && fclose(out) != 0) ok = false;
    return ok ? 0 : 2;
}
#endif
