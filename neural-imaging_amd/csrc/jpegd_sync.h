// What the two entropy decoders share beside the un-stuffing of jpegd_prepare.h (jpegd.hip: a segment per image; jpegd_prog.hip: a
// segment per image and first scan): the limits and checks of their launchers, and the synchronisation rounds and block placement that
// one workgroup runs on the exit states of a segment's subsequences (DESIGN.md sections 4e, 4i, 4n).  Device-only, internal linkage.
#pragma once
#include "jpegc.h"
#include "jpegd.h"

namespace {

// ---- the launchers' limits ----------------------------------------------------------------------------------------------------------
constexpr uint32_t JPEGD_SUBSEQ_MAX = 1u << 30;
constexpr uint64_t JPEGD_ECD_MAX = (1ull << 28) - 1;        // bytes of one segment: bit positions stay below 2^31

// subseq_bits as a caller passes it -> *sb, the bits of one subsequence: a multiple of 32, 0 = the unit's default
inline bool jpegd_subseq_ok(int subseq_bits, uint32_t default_bits, uint32_t* sb) {
    if (subseq_bits < 0 || (subseq_bits & 31) || (uint32_t)subseq_bits > JPEGD_SUBSEQ_MAX) return false;
    *sb = subseq_bits ? (uint32_t)subseq_bits : default_bits;
    return true;
}

// The segment offsets are on the device, so the largest total of segment bytes the workspace serves bounds every index derived from
// them: the largest t <= hi with bytes_for(t) <= workspace_bytes.  bytes_for(t), what the unit carves for t bytes, grows; bytes_for(0) fits.
template <class BytesFor>
inline uint64_t jpegd_ecd_capacity(BytesFor bytes_for, uint64_t hi, size_t workspace_bytes) {
    uint64_t lo = 0;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (bytes_for(mid) <= workspace_bytes) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the `count` tables of a segment into LDS
__device__ __forceinline__ void jpegd_load_tables(JpegdTable* dst, const JpegdTable* src, int count, int threads) {
    const uint32_t* s = (const uint32_t*)src;
    uint32_t* t = (uint32_t*)dst;
    for (int k = threadIdx.x; k < (int)(count * sizeof(JpegdTable) / 4); k += threads) t[k] = s[k];
    __syncthreads();
}

// ---- synchronise ----------------------------------------------------------------------------------------------------------------------
// ex[i], cnt[i]: the exit state of subsequence i of a segment's S and the blocks it counted, as the speculation left them.  In a round,
// thread i decodes subsequence i again from the stored exit state of i - 1 and compares; the rounds end when one changes nothing.  After
// round r the subsequences 0 .. r of every restart interval are true, so round r skips them and `longest` - 1 rounds always suffice
// (longest: the subsequences of the longest interval): a stream that never synchronises costs a sequential decode and is still decoded
// correctly.  Returns the rounds taken, the states visible to the whole workgroup.
// The rounds are driven inside ONE workgroup of THREADS threads: states are exchanged behind its barrier only, so nothing waits on
// another workgroup and no flag crosses a kernel.  More than THREADS subsequences are walked in chunks FROM THE LAST TO THE FIRST, a chunk
// reading its predecessors' states before the barrier and writing its own behind it.  The one state a chunk reads that another chunk
// writes is the last of the chunk before it, which is walked later in the round; inside a chunk the barrier stands between all reads
// and all writes.  So thread i reads i - 1 before any thread of this round has written it: a round is a pure function of the states of
// the round before, and `rounds` is the same for every chunking, on the host (tests/*_host.cpp run one chunk of S) as on the device.
// Every exact test of `rounds` depends on this.
// The caller's two functors (force-inlined: each has this one call):
//   active(i, r, sp)   subsequence i (r <= i < S) is still decoded in round r: it is not among the first r of its interval.  sp is the
//                      loop's, for what active found about i (jpegd_span) and run needs again; it may be left alone
//   run(i, sp, s, n)   decodes subsequence i from state s without writing -> s its exit state, n the blocks it counts
template <int THREADS, class Active, class Run>
__device__ __forceinline__ uint32_t jpegd_sync_rounds(uint32_t S, uint32_t longest, JpegdState* ex, uint32_t* cnt, Active active, Run run) {
    const uint32_t tid = threadIdx.x, chunks = (S + THREADS - 1) / THREADS;
    uint32_t rounds = 0;
    while (rounds + 1 < longest) {
        ++rounds;
        int changed = 0;
        for (uint32_t c = chunks; c-- > 0;) {
            const uint32_t i = c * THREADS + tid;
            JpegdSpan sp;
            const bool live = i >= rounds && i < S && active(i, rounds, sp);        // (i < rounds: true whatever its interval)
            JpegdState s;
            if (live) s = ex[i - 1];
            __syncthreads();                           // every state of this chunk's predecessors is read before one is written
            if (live) {
                const JpegdState old = ex[i];
                uint32_t count;
                run(i, sp, s, count);
                if (s.p != old.p || s.mz != old.mz) changed = 1;
                ex[i] = s; cnt[i] = count;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    __syncthreads();
    return rounds;
}

// ---- place --------------------------------------------------------------------------------------------------------------------------
// cnt[S]: the blocks every subsequence counted -> in place, the index of the first of them among the segment's; returns their total.
// wtot: THREADS / 64 words of LDS
template <int THREADS>
__device__ __forceinline__ uint32_t jpegd_place_blocks(uint32_t S, uint32_t* cnt, uint32_t* wtot) {
    const uint32_t tid = threadIdx.x, chunks = (S + THREADS - 1) / THREADS;
    uint32_t carry = 0;
    for (uint32_t c = 0; c < chunks; ++c) {
        const uint32_t i = c * THREADS + tid;
        const uint32_t v = i < S ? cnt[i] : 0u;
        uint32_t sum;
        const uint32_t exq = block_excl_scan<uint32_t, THREADS>(v, wtot, sum);
        if (i < S) cnt[i] = carry + exq;
        carry += sum;
    }
    return carry;
}

// Behind jpegd_place_blocks, by all threads of the workgroup: true in a thread that found a restart interval which counted fewer blocks
// than it owns - `per` each, the last one what is left of SB.  sub0[K + 1]: the first subsequence of every interval (jpegd.h)
__device__ __forceinline__ bool jpegd_intervals_short(const uint32_t* cnt, const uint32_t* sub0, uint32_t K, uint32_t total, uint32_t per,
                                                      uint32_t SB, uint32_t tid, uint32_t threads) {
    __syncthreads();                                   // the placement is in cnt
    bool few = false;
    for (uint32_t k = tid; k < K; k += threads) {
        const uint32_t have = (k + 1u < K ? cnt[sub0[k + 1u]] : total) - cnt[sub0[k]];
        few |= have < min(per, SB - k * per);
    }
    return few;
}

}  // namespace
