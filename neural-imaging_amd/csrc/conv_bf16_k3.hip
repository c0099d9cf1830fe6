// Throughput-mode convolutions, kernel instantiations: 3x3 / stride 1 over float32-stored inputs.
#include "conv_bf16_tile.h"

template int conv_bf16_dispatch<3, 1, false>(const ConvArgsB&, hipStream_t);
template int conv_bf16_launch_16x16<3, false>(const ConvArgsB&, bool, hipStream_t);
