// Throughput-mode convolutions, kernel instantiations: 2x2 / stride 2 (input gradient of the UNet's Conv2DTranspose).
#include "conv_bf16_tile.h"

template int conv_bf16_dispatch<2, 2, false>(const ConvArgsB&, hipStream_t);
template int conv_bf16_dispatch<2, 2, true>(const ConvArgsB&, hipStream_t);
