// Un-stuffing one entropy-coded segment by one workgroup (DESIGN.md sections 4e, 4i): shared by the baseline decoder (jpegd.hip, a
// segment per image) and the progressive one (jpegd_prog.hip, a segment per image and scan).
#pragma once
#include "jpegc.h"
#include "jpegd.h"

namespace {

// what the un-stuffing scan sums: the bytes kept - with restart intervals also the markers met, in the upper half
template <bool RST> struct PrepSum { typedef uint32_t type; };
template <> struct PrepSum<true> { typedef unsigned long long type; };

// The `len` bytes at src without their stuffing (FF 00 -> FF), MSB first in 32-bit words at `out` ((len + 3) / 4 + 1 words), by a
// block scan with a carry; *total_bits and *nsub, the subsequences of `sb` bits.  RST: the markers FF D0 .. D7 go too, their sequence
// is checked, ibit[K + 1] takes the bit every one of the K intervals begins at, sub0[K + 1] the first subsequence of every interval -
// each is cut on its own - and *maxsub the subsequences of the longest.  Flags are ORed into *status.  Called by all SCAN_THREADS
// threads of a workgroup.
template <bool RST>
__device__ __forceinline__ void jpegd_prepare_segment(const uint8_t* src, uint32_t len, uint8_t* out, uint32_t K, uint32_t sb, uint32_t* ibit,
                                                      uint32_t* sub0, uint32_t* status, uint32_t* total_bits, uint32_t* nsub,
                                                      uint32_t* maxsub) {
    typedef typename PrepSum<RST>::type Sum;
    __shared__ Sum wtot[SCAN_THREADS / 64];
    __shared__ uint32_t s_max;
    const int tid = threadIdx.x;
    const uint32_t cap_bytes = ((len + 3u) / 4u + 1u) * 4u;
    Sum carry = 0;
    uint32_t flags = 0;
    for (uint32_t base = 0; base < len; base += 4u * SCAN_THREADS) {
        const uint32_t j = base + 4u * tid;
        uint8_t b[6];                                  // the byte before, four of this thread's, the byte after
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const uint32_t k = j + (uint32_t)q - 1u;
            b[q] = (j + (uint32_t)q >= 1u && k < len) ? src[k] : (uint8_t)1;        // outside the segment: neither FF nor 00
        }
        uint32_t keep = 0, kept = 0, mark = 0, marks = 0;
#pragma unroll
        for (int q = 1; q <= 4; ++q) {
            if (j + (uint32_t)q - 1u >= len) break;
            if (RST && b[q] == 0xff && (b[q + 1] & 0xf8) == 0xd0) { mark |= 1u << q; ++marks; continue; }       // a restart marker:
            if (RST && b[q - 1] == 0xff && (b[q] & 0xf8) == 0xd0) continue;                                      // both bytes go
            if (b[q] == 0xff && b[q + 1] != 0) flags |= JPEGD_ST_MARKER;
            if (!(b[q] == 0 && b[q - 1] == 0xff)) { keep |= 1u << q; ++kept; }
        }
        Sum sum;
        const Sum before = carry + block_excl_scan((Sum)kept | (RST ? (Sum)((unsigned long long)marks << 32) : (Sum)0), wtot, sum);
        carry += sum;
        uint32_t at = (uint32_t)before, idx = RST ? (uint32_t)((unsigned long long)before >> 32) : 0u;
#pragma unroll
        for (int q = 1; q <= 4; ++q) {
            if (keep >> q & 1u) {
                if (at < cap_bytes) out[(at & ~3u) + 3u - (at & 3u)] = b[q];       // byte k of the stream: bits 31 - 8 (k & 3) .. of word k / 4
                ++at;
            }
            if (RST && (mark >> q & 1u)) flags |= jpegd_marker(idx++, b[q + 1], at, K, ibit);
        }
    }
    const uint32_t total = 8u * (uint32_t)carry;
    if (!RST) {
        if (flags) atomicOr(status, flags);
        if (tid == 0) {
            *total_bits = total;
            *nsub = total == 0 ? 1u : (total + sb - 1u) / sb;
        }
        return;
    }
    // the interval table: the markers met filled entries 1 .. their number; the intervals of missing markers are empty
    const uint32_t met = (uint32_t)((unsigned long long)carry >> 32);
    if (met + 1u != K) flags |= JPEGD_ST_RESTART;
    if (flags) atomicOr(status, flags);
    for (uint32_t k = min(met, K - 1u) + 1u + tid; k <= K; k += SCAN_THREADS) ibit[k] = total;
    if (tid == 0) { ibit[0] = 0; s_max = 0; }
    __syncthreads();
    // the subsequences: every interval is cut on its own
    uint32_t first = 0, longest = 0;
    for (uint32_t base = 0; base < K; base += SCAN_THREADS) {
        const uint32_t k = base + tid;
        const uint32_t subs = k < K ? jpegd_interval_subs(ibit[k + 1u] - ibit[k], sb) : 0u;
        uint32_t sum;
        const uint32_t ex = first + block_excl_scan(subs, (uint32_t*)wtot, sum);
        first += sum;
        if (k < K) sub0[k] = ex;
        longest = max(longest, subs);
    }
    atomicMax(&s_max, longest);
    __syncthreads();
    if (tid == 0) {
        sub0[K] = first;
        *total_bits = total;
        *nsub = first;
        *maxsub = s_max;
    }
}

}  // namespace
