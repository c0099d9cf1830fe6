// Throughput-mode convolutions, kernel instantiations: 5x5 / stride 1 over bf16-stored inputs (tile, buffer-load and ring
// kernels).
#include "conv_bf16_tile.h"

template int conv_bf16_dispatch<5, 1, true>(const ConvArgsB&, hipStream_t);
template int conv_bf16_launch_16x16<5, true>(const ConvArgsB&, bool, hipStream_t);

int conv_bf16_pool_ring_tn(const ConvArgsB& a, bool tn32) { return tn32 ? 0 : conv5_ring_tn(ConvParamsB{a}); }
