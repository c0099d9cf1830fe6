// ConstrainedConv2D kernel re-normalisation (models/layers.py:45-53), the one copy of its arithmetic: constrained_fwd_kernel
// (constrained.hip) runs it on the raw kernel in global memory, adam_images_kernel (adam.hip) on the values it has just
// updated, in LDS.  Same sums in the same order, same divisions: the same bits.
#pragma once
#include "common.h"

namespace nimg {

__device__ __forceinline__ bool centre_mask(int e, int ks, int c) {
    // e indexes (kh,kw,ci,co) flattened
    const int co = e % c, ci = (e / c) % c, kw = (e / (c * c)) % ks, kh = e / (c * c * ks);
    return kh == ks / 2 && kw == ks / 2 && ci == co;
}

// Called by every thread of the workgroup.  k: ks x ks x c x c raw values (global or LDS), c <= 16; df: 16 floats of LDS;
// nf: the normalised filter; nft (optional): the same values laid out as nimg_conv_flip_weights(nf) - nft[taps-1-t][co][ci].
__device__ __forceinline__ void constrained_normalise(const float* k, float* __restrict__ nf, float* __restrict__ nft, float* df,
                                                      int ks, int c, float strength) {
    const int total = ks * ks * c * c, tid = threadIdx.x;
    if (tid < c) {
        float s = 0.f;
        for (int e = tid; e < total; e += c)            // all elements with co == tid
            if (!centre_mask(e, ks, c)) s += k[e];
        df[tid] = s;
    }
    __syncthreads();
    for (int e = tid; e < total; e += blockDim.x) {
        const bool m = centre_mask(e, ks, c);
        const float val = m ? -strength : strength * k[e] / df[e % c];
        nf[e] = val;
        if (nft) nft[((ks * ks - 1 - e / (c * c)) * c + e % c) * c + (e / c) % c] = val;
    }
}

}  // namespace nimg
