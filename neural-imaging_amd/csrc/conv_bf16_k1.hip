// Throughput-mode convolutions, kernel instantiations: 1x1 (the Conv2DTranspose forward included).
#include "conv_bf16_tile.h"

template int conv_bf16_dispatch<1, 1, false>(const ConvArgsB&, hipStream_t);
template int conv_bf16_dispatch<1, 1, true>(const ConvArgsB&, hipStream_t);
