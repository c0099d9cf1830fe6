// The geometry of one batch of baseline JPEG images, for every unit of the JPEG family (jpegc.h, jpegopt.h, jpegd.h) and for the host
// programs that run their sequential cores (tests/jpegopt_host.cpp, tests/jpegd_host.cpp): plain C++, nothing of HIP.
#pragma once

struct JpegGeo {
    int n, h, w, hs, vs, hsh;          // hsh = log2(hs)
    int bhY, bwY, bhC, bwC;            // real extent in blocks: ceil(ceil(W * h / hmax) / 8), the same for the height
    int ceh, cew;                      // chroma extent in samples: ceil(H / vs), ceil(W / hs)
    int my, mx, per;                   // MCU grid; blocks per MCU = hs * vs + 2
    int nbY, nbC, NB;                  // real blocks per image: Y, one chroma component, all three
    int SB;                            // blocks per image in scan order, dummies included
};

inline bool make_geo(JpegGeo* g, int n, int h, int w, int hs, int vs) {
    if (n < 1 || n > 65535 || h < 1 || w < 1 || h > 4096 || w > 4096) return false;
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
    g->n = n; g->h = h; g->w = w; g->hs = hs; g->vs = vs; g->hsh = hs - 1;
    g->bhY = (h + 7) / 8; g->bwY = (w + 7) / 8;
    g->ceh = (h + vs - 1) / vs; g->cew = (w + hs - 1) / hs;
    g->bhC = (g->ceh + 7) / 8; g->bwC = (g->cew + 7) / 8;
    g->my = (h + 8 * vs - 1) / (8 * vs); g->mx = (w + 8 * hs - 1) / (8 * hs);
    g->per = hs * vs + 2;
    g->nbY = g->bhY * g->bwY; g->nbC = g->bhC * g->bwC; g->NB = g->nbY + 2 * g->nbC;
    g->SB = g->my * g->mx * g->per;
    return (long)n * g->SB < 0x7fffffffL;
}
