// The l3ic bitstream of the learned codec (compression/codec.py:87-265 of the reference) on the GPU.  The container and
// the RLE / RAW layer payloads are the reference's; the entropy-coded payload is interleaved rANS instead of FSE (format:
// DESIGN.md "l3ic bitstream", restated in Python by tests/l3ic_ref.py).
//
//   quantise  float32 NHWC latent -> uint8 codebook indices, planar [image][layer][H*W] (scipy.cluster.vq.vq on float32)
//   encode    one wave per (image, layer) stream: histogram, integer normalisation to 4096, RLE / rANS / RAW choice, the
//             L rANS lanes in lock-step writing their words backwards into the stream's slot (ballot + popcount places
//             each step's words in ascending lane order)
//   scan + gather   the payloads of all streams packed back to back (the host copies the lengths, then one buffer)
//   decode    one wave per stream: every payload byte is read through a bounds-checked helper; a malformed stream sets
//             its error word and cannot read outside its own bytes
#include "common.h"

namespace {

using namespace nimg;

constexpr uint32_t M_BITS = 12, M = 1u << M_BITS;       // probability scale 4096
constexpr uint32_t LOW = 1u << 16;                      // state interval [2^16, 2^32), 16-bit words
constexpr int TAB_PAD = M + M / 64;                     // decode table, one pad word per 64 entries (conflict-free build)

__device__ __forceinline__ uint32_t wsum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ uint32_t wmax(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ uint32_t wmin(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ uint32_t wor(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ uint32_t wscan_sum(uint32_t v, int lane) {      // inclusive
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

__device__ __forceinline__ uint32_t wscan_max(uint32_t v, int lane) {      // inclusive
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o, 64);
        if (lane >= o) v = max(v, t);
    }
    return v;
}

// number of set bits of m below this lane
__device__ __forceinline__ uint32_t rank_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__host__ __device__ __forceinline__ int lanes_for(int n_sym) {
    const int q = n_sym / 2048 > 1 ? n_sym / 2048 : 1;
    int l = 1;
    while (l * 2 <= q) l *= 2;
    return l < 64 ? l : 64;
}

inline size_t slot_stride(int n_sym) { return ((size_t)n_sym + 15) / 16 * 16; }

// ---- quantise -----------------------------------------------------------------------------------------------------
// A workgroup takes 64 consecutive pixels of one image with all c features (coalesced NHWC reads) and writes them back
// per feature layer (64 consecutive bytes per layer).  The nearest-entry search is scipy's _vq for one feature: the
// float32 squared difference, strict < (ties -> lower index); a non-finite value sets *err.
__global__ void __launch_bounds__(256) l3ic_quantise_kernel(const float* __restrict__ z, const float* __restrict__ cb, int k,
                                                            uint8_t* __restrict__ idx, int* __restrict__ err, int n_sym, int c) {
    __shared__ float scb[256];
    extern __shared__ __attribute__((aligned(16))) uint8_t tile[];      // [c][64]
    const int b = blockIdx.y, p0 = blockIdx.x * 64, tid = threadIdx.x;
    for (int j = tid; j < k; j += 256) scb[j] = cb[j];
    __syncthreads();
    const int np = min(64, n_sym - p0);
    const float* zb = z + ((long)b * n_sym + p0) * c;
    bool bad = false;
    for (int j = tid; j < np * c; j += 256) {
        const float v = zb[j];
        float best = __int_as_float(0x7f800000);
        int bi = 0;
        for (int q = 0; q < k; ++q) {
            const float d = __fsub_rn(scb[q], v);
            const float d2 = __fmul_rn(d, d);
            if (d2 < best) {
                best = d2;
                bi = q;
            }
        }
        if (!isfinite(v)) bad = true;
        const int p = j / c;
        tile[(j - p * c) * 64 + p] = (uint8_t)bi;
    }
    if (bad) atomicOr(err, 1);
    __syncthreads();
    uint8_t* ob = idx + (long)b * c * n_sym + p0;
    for (int j = tid; j < np * c; j += 256) {
        const int f = j / np, p = j - f * np;
        ob[(long)f * n_sym + p] = tile[f * 64 + p];
    }
}

// ---- encode -------------------------------------------------------------------------------------------------------
struct EncArgs {
    const uint8_t* idx;
    uint8_t* slots;       // [streams][stride]
    uint32_t* len;        // [streams] payload bytes
    uint32_t* soff;       // [streams] payload offset inside the slot
    uint32_t* hist;       // [streams][256] (optional)
    uint32_t* freq;       // [streams][256] (optional)
    int n_sym, stride;
};

__global__ void __launch_bounds__(64) l3ic_encode_kernel(EncArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t sym[];      // the stream's n_sym symbols
    __shared__ uint32_t h[256];
    __shared__ uint32_t fc[256];                                       // f | cum << 16
    const int s = blockIdx.x, lane = threadIdx.x, n = p.n_sym;
    const uint8_t* src = p.idx + (long)s * n;
#pragma unroll
    for (int q = 0; q < 4; ++q) h[lane + 64 * q] = 0;
    __syncthreads();
    int j = lane;
    for (; j + 7 * 64 < n; j += 8 * 64) {
        uint8_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[j + u * 64];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            sym[j + u * 64] = v[u];
            atomicAdd(&h[v[u]], 1u);
        }
    }
    for (; j < n; j += 64) {
        const uint8_t v = src[j];
        sym[j] = v;
        atomicAdd(&h[v], 1u);
    }
    __syncthreads();

    // this lane's symbols: 4 lane .. 4 lane + 3
    const uint32_t s0 = 4 * lane;
    uint32_t c[4], f[4];
    uint32_t lo = 256, hi = 0, nd = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        c[q] = h[s0 + q];
        if (c[q]) {
            lo = min(lo, s0 + q);
            hi = max(hi, s0 + q);
            ++nd;
        }
        f[q] = c[q] ? max(1u, c[q] * M / (uint32_t)n) : 0u;        // c * 4096 < 2^32 for n <= 65535
        tot += f[q];
    }
    const uint32_t a = wmin(lo), b = wmax(hi), distinct = wsum(nd);
    tot = wsum(tot);
    if (tot < M) {                    // the whole deficit to the largest count (lowest index on ties)
        uint32_t key = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (c[q]) key = max(key, (c[q] << 8) | (255u - (s0 + q)));
        const uint32_t w = 255u - (wmax(key) & 255u);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (w == s0 + q) f[q] += M - tot;
    } else if (tot > M) {
        // "while the sum exceeds 4096, take 1 from the largest f > 1 (lowest index on ties)" in closed form: every f above
        // the lowest level v with D(v) = sum(max(0, f - v)) <= surplus comes down to v, then the remaining surplus - D(v)
        // symbols at v, in index order, to v - 1
        const uint32_t r = tot - M;
        uint32_t vl = 1, vh = M;
        while (vl < vh) {
            const uint32_t mid = (vl + vh) >> 1;
            uint32_t d = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) d += f[q] > mid ? f[q] - mid : 0u;
            if (wsum(d) <= r) vh = mid;
            else vl = mid + 1;
        }
        const uint32_t v = vl;
        uint32_t d = 0, at = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            d += f[q] > v ? f[q] - v : 0u;
            at += f[q] >= v ? 1u : 0u;
        }
        const uint32_t left = r - wsum(d);
        uint32_t before = wscan_sum(at, lane) - at;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (f[q] >= v) f[q] = before++ < left ? v - 1 : v;
    }
    if (p.hist) {
#pragma unroll
        for (int q = 0; q < 4; ++q) p.hist[(long)s * 256 + s0 + q] = c[q];
    }
    if (p.freq) {
#pragma unroll
        for (int q = 0; q < 4; ++q) p.freq[(long)s * 256 + s0 + q] = f[q];
    }
    uint8_t* slot = p.slots + (long)s * p.stride;
    if (distinct == 1) {              // RLE: uint16 count, uint8 symbol
        if (lane == 0) {
            slot[0] = (uint8_t)(n & 255);
            slot[1] = (uint8_t)(n >> 8);
            slot[2] = (uint8_t)a;
            p.len[s] = 3;
            p.soff[s] = 0;
        }
        return;
    }
    // cumulative frequencies (low half) and table byte offsets (high half) in one scan
    uint32_t wd[4], loc = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        wd[q] = (s0 + q >= a && s0 + q <= b) ? (f[q] < 128 ? 1u : 2u) : 0u;
        loc += f[q] | (wd[q] << 16);
    }
    const uint32_t incl = wscan_sum(loc, lane);
    const uint32_t table = (uint32_t)__shfl(incl, 63, 64) >> 16;
    uint32_t run = incl - loc, toff[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        toff[q] = run >> 16;
        fc[s0 + q] = f[q] | ((run & 0xffffu) << 16);
        run += f[q] | (wd[q] << 16);
    }
    __syncthreads();

    const int L = lanes_for(n);
    const int hdr = 3 + (int)table + 4 * L;
    const int max_words = (n - hdr - 1) >> 1;           // rANS only if strictly shorter than the raw layer
    uint16_t* wend = reinterpret_cast<uint16_t*>(slot + p.stride);
    const bool lane_on = lane < L;
    const int T = (n + L - 1) / L;
    uint32_t x = LOW;
    int nw = 0;
    bool raw = max_words < 0;
    int i = (T - 1) * L + lane;
    uint32_t e = (lane_on && i < n) ? fc[sym[i]] : 0u;
    for (int t = T - 1; t >= 0 && !raw; --t) {
        const bool act = lane_on && i < n;
        const uint32_t ec = e;
        i -= L;
        e = (lane_on && i >= 0) ? fc[sym[i]] : 0u;        // the next step's (f, cum), off the state's dependency chain
        const uint32_t fs = act ? (ec & 0xffffu) : 1u, cs = ec >> 16;
        const bool emit = act && (uint64_t)x >= ((uint64_t)fs << 20);
        const uint64_t m = __ballot(emit);
        const int cnt = __popcll(m);
        if (nw + cnt > max_words) {
            raw = true;
            break;
        }
        if (emit) {
            wend[(int)rank_below(m) - (nw + cnt)] = (uint16_t)(x & 0xffffu);
            x >>= 16;
        }
        nw += cnt;
        if (act) x = ((x / fs) << M_BITS) + (x % fs) + cs;
    }
    if (raw) {
        for (int k2 = lane; k2 < n; k2 += 64) slot[k2] = sym[k2];
        if (lane == 0) {
            p.len[s] = n;
            p.soff[s] = 0;
        }
        return;
    }
    const int total = hdr + 2 * nw;
    uint8_t* out = slot + (p.stride - total);
    if (lane == 0) {
        out[0] = (uint8_t)L;
        out[1] = (uint8_t)a;
        out[2] = (uint8_t)b;
        p.len[s] = total;
        p.soff[s] = p.stride - total;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint8_t* d = out + 3 + toff[q];
        if (wd[q] == 1) {
            d[0] = (uint8_t)f[q];
        } else if (wd[q] == 2) {
            d[0] = (uint8_t)((f[q] & 0x7fu) | 0x80u);
            d[1] = (uint8_t)(f[q] >> 7);
        }
    }
    if (lane_on) {
        uint8_t* d = out + 3 + table + 4 * lane;
        d[0] = (uint8_t)x;
        d[1] = (uint8_t)(x >> 8);
        d[2] = (uint8_t)(x >> 16);
        d[3] = (uint8_t)(x >> 24);
    }
}

// exclusive scan of the payload lengths (one workgroup, any number of streams)
__global__ void __launch_bounds__(1024) l3ic_scan_kernel(const uint32_t* __restrict__ len, uint32_t* __restrict__ dst,
                                                         int streams) {
    __shared__ uint32_t wtot[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int per = (streams + 1023) / 1024, j0 = tid * per, j1 = min(streams, j0 + per);
    uint32_t loc = 0;
    for (int j = j0; j < j1; ++j) loc += len[j];
    const uint32_t incl = wscan_sum(loc, lane);
    if (lane == 63) wtot[wv] = incl;
    __syncthreads();
    uint32_t run = incl - loc;
    for (int w = 0; w < wv; ++w) run += wtot[w];
    for (int j = j0; j < j1; ++j) {
        dst[j] = run;
        run += len[j];
    }
}

__global__ void __launch_bounds__(256) l3ic_gather_kernel(const uint8_t* __restrict__ slots, int stride,
                                                          const uint32_t* __restrict__ soff, const uint32_t* __restrict__ len,
                                                          const uint32_t* __restrict__ dst, uint8_t* __restrict__ out) {
    const int s = blockIdx.x;
    const uint8_t* a = slots + (long)s * stride + soff[s];
    uint8_t* d = out + dst[s];
    const uint32_t n = len[s];
    for (uint32_t j = threadIdx.x; j < n; j += 256) d[j] = a[j];
}

// ---- decode -------------------------------------------------------------------------------------------------------
struct DecArgs {
    const uint8_t* data;
    const uint32_t* off;
    const uint32_t* len;
    const float* cb;
    float* z;             // (n, h, w, c) float32
    uint32_t* err;        // [streams] NIMG_L3IC_E_* bits
    int k, n_sym, c;
};

__global__ void __launch_bounds__(64) l3ic_decode_kernel(DecArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t buf[];      // the payload (a rANS payload is < n_sym bytes)
    __shared__ uint32_t tab[TAB_PAD];          // slot -> symbol | (f - 1) << 8 | (slot - cum) << 20, at slot + slot / 64
    __shared__ uint32_t fc[256];               // f | cum << 16
    __shared__ float scb[256];
    __shared__ uint32_t hdr[3];
    const int s = blockIdx.x, lane = threadIdx.x, n = p.n_sym, c = p.c, k = p.k;
    const uint32_t len = p.len[s];
    const uint8_t* src = p.data + p.off[s];
    float* zo = p.z + (long)(s / c) * n * c + (s % c);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = lane + 64 * q;
        scb[j] = j < k ? p.cb[j] : 0.0f;
        fc[j] = 0;
    }
    __syncthreads();
    uint32_t err = 0;
    if (len == (uint32_t)n) {                              // RAW
        for (int i = lane; i < n; i += 64) {
            uint32_t v = src[i];                           // i < n == len
            if (v >= (uint32_t)k) {
                err |= NIMG_L3IC_E_SYMBOL;
                v = 0;
            }
            zo[(long)i * c] = scb[v];
        }
    } else if (len == 3) {                                 // RLE
        const uint32_t count = src[0] | (src[1] << 8), v = src[2];
        if (count != (uint32_t)n) err |= NIMG_L3IC_E_RLE;
        if (v >= (uint32_t)k) err |= NIMG_L3IC_E_SYMBOL;
        if (!err)
            for (int i = lane; i < n; i += 64) zo[(long)i * c] = scb[v];
    } else if (len > (uint32_t)n) {
        err |= NIMG_L3IC_E_READ;
    } else {                                               // rANS
        uint32_t j = lane;
        for (; j + 7 * 64 < len; j += 8 * 64) {
            uint8_t v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = src[j + u * 64];
#pragma unroll
            for (int u = 0; u < 8; ++u) buf[j + u * 64] = v[u];
        }
        for (; j < len; j += 64) buf[j] = src[j];
        __syncthreads();
        // every payload read: inside the payload, else 0 and the error flag
        auto rd = [&](uint32_t o) -> uint32_t {
            if (o < len) return buf[o];
            err |= NIMG_L3IC_E_READ;
            return 0u;
        };
        if (lane == 0) {
            const uint32_t L = rd(0), a = rd(1), b = rd(2);
            if (L < 1 || L > 64) err |= NIMG_L3IC_E_LANES;
            if (a > b) err |= NIMG_L3IC_E_RANGE;
            if (b >= (uint32_t)k) err |= NIMG_L3IC_E_SYMBOL;
            uint32_t pos = 3, sum = 0;
            if (!err) {
                for (uint32_t q = a; q <= b; ++q) {
                    uint32_t v = rd(pos++);
                    if (v & 0x80u) {
                        const uint32_t v2 = rd(pos++);
                        if (v2 & 0x80u) err |= NIMG_L3IC_E_VARINT;
                        v = (v & 0x7fu) | ((v2 & 0x7fu) << 7);
                    }
                    if (sum + v > M) {
                        err |= NIMG_L3IC_E_FREQ;
                        break;
                    }
                    fc[q] = v | (sum << 16);
                    sum += v;
                }
                if (sum != M) err |= NIMG_L3IC_E_FREQ;
                if (!(fc[a] & 0xffffu) || !(fc[b] & 0xffffu)) err |= NIMG_L3IC_E_RANGE;   // a, b carry non-zero frequencies
            }
            hdr[0] = L;
            hdr[1] = pos;
            hdr[2] = err;
        }
        __syncthreads();
        err = hdr[2];                                      // the same on every lane: the branches below are uniform
        if (!err) {
            const uint32_t L = hdr[0], st = hdr[1];
            // slot -> symbol: mark each symbol's first slot, then a running maximum over the 4096 slots
#pragma unroll 8
            for (int q = 0; q < 64; ++q) tab[lane * 65 + q] = 0;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t e = fc[lane + 64 * q], cum = e >> 16;
                if (e & 0xffffu) tab[cum + (cum >> 6)] = lane + 64 * q + 1;
            }
            __syncthreads();
            uint32_t mx = 0;
#pragma unroll 8
            for (int q = 0; q < 64; ++q) mx = max(mx, tab[lane * 65 + q]);
            uint32_t carry = wscan_max(mx, lane);
            carry = __shfl_up(carry, 1, 64);
            if (lane == 0) carry = 0;
#pragma unroll 4
            for (int q = 0; q < 64; ++q) {
                carry = max(carry, tab[lane * 65 + q]);
                const uint32_t sv = carry - 1, e = fc[sv & 255u], slot = lane * 64 + q;
                tab[lane * 65 + q] = (sv & 255u) | (((e & 0xffffu) - 1) << 8) | ((slot - (e >> 16)) << 20);
            }
            __syncthreads();
            uint32_t x = LOW;
            if (lane < (int)L) {
                const uint32_t o = st + 4 * lane;
                x = rd(o) | (rd(o + 1) << 8) | (rd(o + 2) << 16) | (rd(o + 3) << 24);
            }
            const uint32_t ws = st + 4 * L;
            if (ws <= len && ((len - ws) & 1u)) err |= NIMG_L3IC_E_ODD;
            const uint32_t nwords = ws <= len ? (len - ws) >> 1 : 0u;
            uint32_t wp = 0;
            const int T = (n + (int)L - 1) / (int)L;
            int i = lane;
            for (int t = 0; t < T; ++t, i += (int)L) {
                const bool act = lane < (int)L && i < n;
                if (act) {
                    const uint32_t slot = x & (M - 1);
                    const uint32_t e = tab[slot + (slot >> 6)];
                    x = (((e >> 8) & 0xfffu) + 1) * (x >> M_BITS) + (e >> 20);
                    zo[(long)i * c] = scb[e & 255u];
                }
                const bool need = act && x < LOW;
                const uint64_t m = __ballot(need);
                if (need) {
                    const uint32_t o = ws + 2 * (wp + rank_below(m));
                    x = (x << 16) | rd(o) | (rd(o + 1) << 8);
                }
                wp += (uint32_t)__popcll(m);
            }
            if (wp < nwords) err |= NIMG_L3IC_E_UNUSED;
            if (lane < (int)L && x != LOW) err |= NIMG_L3IC_E_STATE;
        }
    }
    err = wor(err);
    if (lane == 0) p.err[s] = err;
}

}  // namespace

size_t nimg_l3ic_workspace_bytes(int n_streams, int n_sym) {
    if (n_streams < 1 || n_sym < 1) return 0;
    return align256((size_t)n_streams * slot_stride(n_sym)) + 2 * align256((size_t)n_streams * 4);
}

int nimg_l3ic_quantise(const float* z, const float* codebook, int codebook_size, uint8_t* idx, int* err, int n, int h,
                       int w, int c, void* stream) {
    if (!z || !codebook || !idx || !err || codebook_size < 1 || codebook_size > 256 || n < 1 || h < 1 || w < 1 || c < 1 ||
        n > 65535 || (long)h * w > 65535 || c > 2048)
        return NIMG_ERR_ARG;
    const int n_sym = h * w;
    hipLaunchKernelGGL(l3ic_quantise_kernel, dim3((unsigned)((n_sym + 63) / 64), (unsigned)n), dim3(256), (size_t)64 * c,
                       (hipStream_t)stream, z, codebook, codebook_size, idx, err, n_sym, c);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_l3ic_encode(const uint8_t* idx, int n_streams, int n_sym, uint8_t* out, uint32_t* lengths, uint32_t* hist,
                     uint32_t* freq, void* workspace, size_t workspace_bytes, void* stream) {
    if (!idx || !out || !lengths || !workspace || n_streams < 1 || n_sym < 4 || n_sym > 65535) return NIMG_ERR_ARG;
    if (workspace_bytes < nimg_l3ic_workspace_bytes(n_streams, n_sym)) return NIMG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t stride = slot_stride(n_sym);
    uint8_t* slots = (uint8_t*)workspace;
    uint32_t* soff = (uint32_t*)(slots + align256((size_t)n_streams * stride));
    uint32_t* dst = (uint32_t*)((uint8_t*)soff + align256((size_t)n_streams * 4));
    const size_t lds = stride;
    (void)hipFuncSetAttribute((const void*)l3ic_encode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    EncArgs a{idx, slots, lengths, soff, hist, freq, n_sym, (int)stride};
    hipLaunchKernelGGL(l3ic_encode_kernel, dim3((unsigned)n_streams), dim3(64), lds, st, a);
    NIMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(l3ic_scan_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)lengths, dst, n_streams);
    NIMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(l3ic_gather_kernel, dim3((unsigned)n_streams), dim3(256), 0, st, (const uint8_t*)slots, (int)stride,
                       (const uint32_t*)soff, (const uint32_t*)lengths, (const uint32_t*)dst, out);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}

int nimg_l3ic_decode(const uint8_t* data, const uint32_t* offsets, const uint32_t* lengths, const float* codebook,
                     int codebook_size, float* z, uint32_t* err, int n, int h, int w, int c, void* stream) {
    if (!data || !offsets || !lengths || !codebook || !z || !err || codebook_size < 1 || codebook_size > 256 || n < 1 ||
        h < 1 || w < 1 || c < 1 || (long)h * w > 65535 || (long)n * c > 0x7fffffffL)
        return NIMG_ERR_ARG;
    const int n_sym = h * w;
    const size_t lds = slot_stride(n_sym);
    (void)hipFuncSetAttribute((const void*)l3ic_decode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    DecArgs a{data, offsets, lengths, codebook, z, err, codebook_size, n_sym, c};
    hipLaunchKernelGGL(l3ic_decode_kernel, dim3((unsigned)(n * c)), dim3(64), lds, (hipStream_t)stream, a);
    NIMG_CHECK_LAUNCH();
    return NIMG_OK;
}
