// The step from a real-valued quantisation table entry - a learned weight of JPEG(trainable=True), or the reference's jpeg_qtable - to
// the entry a baseline file can carry: an integer 1..255.  One function, `__host__ __device__` under hipcc and
// plain C++ otherwise, so that the kernel (jpegc_tables.hip) and a host program share it; tests/jpegq_ref.py restates it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define JPEGQ_HD __host__ __device__
#else
#define JPEGQ_HD
#endif

#define JPEGQ_ST_RAISED 1u               // an entry was raised to 1
#define JPEGQ_ST_LOWERED 2u              // an entry was lowered to 255
#define JPEGQ_ST_NONFINITE 4u            // a NaN or an infinity: NaN and -inf become 1, +inf becomes 255

// rintf(v) - ties to even, the rounding mode neither side changes - clamped to 1..255; what had to be done is OR-ed into *status
JPEGQ_HD inline uint16_t jpegq_entry(float v, uint32_t* status) {
    if (!(v - v == 0.0f)) {                      // NaN or +-inf
        *status |= JPEGQ_ST_NONFINITE;
        return v > 0.0f ? (uint16_t)255 : (uint16_t)1;
    }
    const float r = rintf(v);
    if (r < 1.0f) { *status |= JPEGQ_ST_RAISED; return 1; }
    if (r > 255.0f) { *status |= JPEGQ_ST_LOWERED; return 255; }
    return (uint16_t)r;
}
