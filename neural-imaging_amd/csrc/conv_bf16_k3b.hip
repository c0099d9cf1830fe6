// Throughput-mode convolutions, kernel instantiations: 3x3 / stride 1 over bf16-stored inputs (tile, buffer-load, LDS-DMA and
// ring kernels).
#include "conv_bf16_tile.h"

template int conv_bf16_dispatch<3, 1, true>(const ConvArgsB&, hipStream_t);
template int conv_bf16_launch_16x16<3, true>(const ConvArgsB&, bool, hipStream_t);

#ifdef NIMG_CONV3_TIMING
extern "C" int nimg_debug_conv3_timing(unsigned long long* host, int n_words) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_conv3_timing), (size_t)n_words * 8) == hipSuccess ? 0 : -2;
}
#endif
