// Throughput-mode convolutions, kernel instantiations: 5x5 over float32-stored inputs, stride 1 and 2.
#include "conv_bf16_tile.h"

template int conv_bf16_dispatch<5, 1, false>(const ConvArgsB&, hipStream_t);
template int conv_bf16_dispatch<5, 2, false>(const ConvArgsB&, hipStream_t);
template int conv_bf16_launch_16x16<5, false>(const ConvArgsB&, bool, hipStream_t);
