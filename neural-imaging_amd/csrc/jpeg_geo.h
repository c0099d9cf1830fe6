// The geometry of one batch of baseline JPEG images, for every unit of the JPEG family (jpegc.h, jpegopt.h, jpegd.h) and for the host
// programs that run their sequential cores (tests/jpegopt_host.cpp, tests/jpegd_host.cpp): plain C++, nothing of HIP
// but the attributes that let a kernel call the two restart-interval predicates.
#pragma once

struct JpegGeo {
    int n, h, w, hs, vs, hsh;          // hsh = log2(hs)
    int bhY, bwY, bhC, bwC;            // real extent in blocks: ceil(ceil(W * h / hmax) / 8), the same for the height
    int ceh, cew;                      // chroma extent in samples: ceil(H / vs), ceil(W / hs)
    int my, mx, per;                   // MCU grid; blocks per MCU = ny + nc - 1: hs * vs + 2, or 1 in a grey-scale file
    int nc, ny;                        // components, 3 or 1; luma blocks per MCU
    int nbY, nbC, NB;                  // real blocks per image: Y, one chroma component, all three
    int SB;                            // blocks per image in scan order, dummies included
    int ri;                            // restart interval in MCUs; 0 = none, which make_geo sets
};

#if defined(__HIPCC__)
#define JPEG_GEO_HD __host__ __device__
#else
#define JPEG_GEO_HD
#endif

// MCU m begins a restart interval: the DC predictors are 0 there (always true of MCU 0)
JPEG_GEO_HD inline bool jpeg_interval_start(const JpegGeo& g, int m) { return m == 0 || (g.ri > 0 && m % g.ri == 0); }

// scan block s is the last of a restart interval that a marker follows (never the last block of the image)
JPEG_GEO_HD inline bool jpeg_marker_follows(const JpegGeo& g, int s) {
    return g.ri > 0 && s + 1 < g.SB && (s + 1) % (g.ri * g.per) == 0;
}

// restart markers of one image: one behind every interval but the last
JPEG_GEO_HD inline int jpeg_markers(const JpegGeo& g) { return g.ri > 0 ? (g.my * g.mx + g.ri - 1) / g.ri - 1 : 0; }

// the restart interval of a call into the geometry; false = outside 0..65535
inline bool set_restart(JpegGeo* g, int restart_interval) {
    if (restart_interval < 0 || restart_interval > 65535) return false;
    g->ri = restart_interval;
    return true;
}

// The luma sampling factors a caller of make_geo admits over 1x1 chroma.  JPEG_FACTORS_THREE: 1x1, 2x1 and 2x2, what every entry point
// took before DESIGN.md section 4r and what all but the nimg_jpeg_sampling_* entries still take.  JPEG_FACTORS_WIDE: also 1x2, 4x1, 4x2,
// 1x4 and 2x4 - every power-of-two pair whose MCU has at most the ten blocks T.81 allows.
enum { JPEG_FACTORS_THREE = 0, JPEG_FACTORS_WIDE = 1 };
// the set of a call that names none: the three - but for a host program that holds the cores to the wide set (tests/jpegsamp_host.cpp)
#ifndef JPEG_FACTORS_DEFAULT
#define JPEG_FACTORS_DEFAULT JPEG_FACTORS_THREE
#endif

inline bool jpeg_factors_ok(int hs, int vs, int factors) {
    if ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)) return true;
    if (factors != JPEG_FACTORS_WIDE) return false;
    return (hs == 1 && vs == 2) || (hs == 4 && vs == 1) || (hs == 4 && vs == 2) || (hs == 1 && vs == 4) || (hs == 2 && vs == 4);
}

// nc = 1: a grey-scale file - one component, never sub-sampled, one block per MCU in raster order; it has no chroma blocks at all
inline bool make_geo(JpegGeo* g, int n, int h, int w, int hs, int vs, int nc = 3, int factors = JPEG_FACTORS_DEFAULT) {
    if (n < 1 || n > 65535 || h < 1 || w < 1 || h > 4096 || w > 4096) return false;
    if (!jpeg_factors_ok(hs, vs, factors)) return false;
    if (nc != 3 && !(nc == 1 && hs == 1 && vs == 1)) return false;
    g->n = n; g->h = h; g->w = w; g->hs = hs; g->vs = vs; g->hsh = hs == 4 ? 2 : hs - 1;
    g->bhY = (h + 7) / 8; g->bwY = (w + 7) / 8;
    g->ceh = (h + vs - 1) / vs; g->cew = (w + hs - 1) / hs;
    g->bhC = (g->ceh + 7) / 8; g->bwC = (g->cew + 7) / 8;
    g->my = (h + 8 * vs - 1) / (8 * vs); g->mx = (w + 8 * hs - 1) / (8 * hs);
    g->nc = nc; g->ny = hs * vs; g->per = g->ny + nc - 1;
    if (nc == 1) g->bhC = g->bwC = 0;
    g->nbY = g->bhY * g->bwY; g->nbC = g->bhC * g->bwC; g->NB = g->nbY + (nc - 1) * g->nbC;
    g->SB = g->my * g->mx * g->per;
    g->ri = 0;
    return (long)n * g->SB < 0x7fffffffL;
}
