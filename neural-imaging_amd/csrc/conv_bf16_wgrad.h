// Shared by conv_bf16_wgrad.hip (the throughput-mode weight gradient and its dispatch) and conv_bf16_packed.hip (the few-channel
// kernels of the FAN front end, whose weight gradient that dispatch launches): the kernels' parameter block and tile constants.
#pragma once
#include "conv_bf16.h"

// The fields of WgradParamsB, with external linkage: what nimg_internal_wgrad_packed (common.h) carries from one translation
// unit to the other.  The kernels keep taking the file-local WgradParamsB below (their names do not change).
struct WgradArgsB {
    const float* in1;
    const float* in2;
    const float* dz;
    const unsigned char* dz_idx;   // optional (packed kernel): dz is the POOLED gradient (Hout/2 x Wout/2) of a fused
                                   // conv+pool layer and dz_idx its arg-max bytes - the 2x2 un-pooling happens while staging
    float* partial;
    float* db_partial;
    int C1, C2, Cout;
    int N, H, W, Hout, Wout, pad_t, pad_l;
    int tiles_y, tiles_x, splits, work_per_split, pad_mode;
    int flags;                     // NIMG_BF16_IN: in1 (and in2) hold bf16; NIMG_BF16_DZ: dz holds bf16
    // in-kernel finish of the split-K sums by the last-arriving workgroup of a dw tile (common.h ticket_finish); null: slabs only
    unsigned* tickets;
    float* dw;
    float* db;
    int group, accumulate;
    nimg::ReduceEntry pre;         // the reduction the PREVIOUS weight gradient of this stream owes (chained mode), or empty
};

namespace {

struct WgradParamsB : WgradArgsB {};      // what the kernels take

constexpr int B_TH = 8, B_TW = 16, B_CI = 32, B_CO = 64;

}  // namespace
