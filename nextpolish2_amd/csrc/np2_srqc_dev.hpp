// Device helpers of the short-read filters, shared by the quality filter (np2_srqc.hip) and the adapter trimmer
// (np2_sradapt.hip): a wavefront's aligned loads, the window and N-run ballots, the masking stores, and steps 1 - 3 of the
// quality rule (np2_srqc_core.hpp) for one read.  Every function is called by all 64 lanes of a wavefront with the same
// arguments but `lane`; what it returns is the same in every lane.
#pragma once
#include <hip/hip_runtime.h>

#include "np2_srqc_core.hpp"

namespace np2 {
namespace srqc_dev {
using namespace np2srqc;

static constexpr uint32_t SRQC_BLOCK = 256, SRQC_WAVES = SRQC_BLOCK / 64;
static constexpr uint32_t SRQC_PASS = 256; // bytes a wavefront covers per pass
static constexpr uint32_t N4 = 0x4E4E4E4Eu;

// the 4 bytes at byte offset `off` of `base` (4-byte aligned; off may be a little negative), lowest address in bits 0 .. 7
__device__ __forceinline__ uint32_t load4(const uint8_t *base, int64_t off) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(base) + (off >> 2);
    const uint64_t v = (uint64_t)w[1] << 32 | w[0];
    return (uint32_t)(v >> (8u * (uint32_t)(off & 3)));
}
// the 4 bytes that END at byte offset `off` (exclusive), highest address in bits 0 .. 7: a backward walk's next 4
__device__ __forceinline__ uint32_t load4_back(const uint8_t *base, int64_t off) { return __builtin_bswap32(load4(base, off - 4)); }
__device__ __forceinline__ uint32_t byte_of(uint32_t w, uint32_t j) { return (w >> (8u * j)) & 255u; }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum of p over `w` positions from `at`, forward (dir > 0: at, at + 1, ..) or backward (at - 1, at - 2, ..)
template <int DIR> __device__ __forceinline__ uint32_t range_sum(const uint8_t *q, int64_t at, uint32_t w, uint32_t lane) {
    uint32_t s = 0;
    for (uint32_t o = 0; o < w; o += SRQC_PASS) {
        const uint32_t ob = o + 4 * lane;
        if (ob < w) {
            const uint32_t v = DIR > 0 ? load4(q, at + ob) : load4_back(q, at - ob);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) s += ob + j < w ? phred(byte_of(v, j)) : 0u;
        }
    }
    return wave_sum(s);
}

// The smallest u in [0, count) whose window passes, or count.  ws(0) = ws0, ws(u + 1) = ws(u) + p[add +- u] - p[sub +- u]
// (forward: + u, backward: the position before, - 1 - u).
template <int DIR>
__device__ __forceinline__ uint32_t first_window(const uint8_t *q, int64_t add, int64_t sub, uint32_t count, uint32_t ws0, const Opts &o,
                                                 uint32_t lane) {
    uint32_t carry = ws0; // ws(u0); sums are non-negative, the differences wrap modulo 2^32 on the way
    for (uint32_t u0 = 0; u0 < count; u0 += SRQC_PASS) {
        const uint32_t ub = u0 + 4 * lane;
        uint32_t d[4] = {0, 0, 0, 0};
        if (ub < count) {
            const uint32_t va = DIR > 0 ? load4(q, add + ub) : load4_back(q, add - ub);
            const uint32_t vs = DIR > 0 ? load4(q, sub + ub) : load4_back(q, sub - ub);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) d[j] = phred(byte_of(va, j)) - phred(byte_of(vs, j));
        }
        const uint32_t tot = d[0] + d[1] + d[2] + d[3];
        uint32_t inc = tot;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t t = __shfl_up(inc, s);
            if (lane >= (uint32_t)s) inc += t;
        }
        uint32_t w = carry + inc - tot, m = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            m |= (ub + j < count && window_ok(w, o)) ? 1u << j : 0u;
            w += d[j];
        }
        const uint64_t bal = __ballot(m != 0);
        if (bal) {
            const int l = __builtin_ctzll(bal);
            return u0 + 4 * (uint32_t)l + (uint32_t)__builtin_ctz(__shfl(m, l));
        }
        carry += __shfl(inc, 63);
    }
    return count;
}

// The number of N / n at the front (DIR > 0: from `at`) or at the back (the bytes before `at`) of `len` base bytes
template <int DIR> __device__ __forceinline__ uint32_t n_run(const uint8_t *s, int64_t at, uint32_t len, uint32_t lane) {
    for (uint32_t o = 0; o < len; o += SRQC_PASS) {
        const uint32_t ob = o + 4 * lane;
        uint32_t m = 0;
        if (ob < len) {
            const uint32_t v = DIR > 0 ? load4(s, at + ob) : load4_back(s, at - ob);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) m |= (ob + j < len && !is_n(byte_of(v, j))) ? 1u << j : 0u;
        }
        const uint64_t bal = __ballot(m != 0);
        if (bal) {
            const int l = __builtin_ctzll(bal);
            return o + 4 * (uint32_t)l + (uint32_t)__builtin_ctz(__shfl(m, l));
        }
    }
    return len;
}

// bytes [lo, hi) of the stream become 'N' (see `mask` above)
__device__ __forceinline__ void mask_range(uint8_t *seq, uint64_t lo, uint64_t hi, uint32_t lane) {
    if (hi <= lo) return;
    const uint64_t w_end = (hi + 3) >> 2;
    for (uint64_t w = (lo >> 2) + lane; w < w_end; w += 64) {
        const uint64_t p = w << 2;
        if (p >= lo && p + 4 <= hi) {
            reinterpret_cast<uint32_t *>(seq)[w] = N4;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (p + j >= lo && p + j < hi) seq[p + j] = 'N';
        }
    }
}

// steps 1 - 3 of the quality rule for the read of n bases at stream offset `start`: its kept span [a, b)
__device__ __forceinline__ void kept_span(const uint8_t *seq, const uint8_t *qual, uint32_t start, uint32_t n, const Opts &o, uint32_t lane,
                                          uint32_t &a, uint32_t &b) {
    fixed_trim(n, o, a, b);
    const int64_t at = start; // positions below are the read's own, the stream's are at + position
    if ((o.flags & CUT_FRONT) && b > a) {
        const uint32_t nw = n_windows(a, b, o);
        uint32_t u = nw;
        if (nw) u = first_window<1>(qual, at + a + o.cut_window, at + a, nw, range_sum<1>(qual, at + a, o.cut_window, lane), o, lane);
        if (u == nw) a = b;
        else {
            a += u;
            a += n_run<1>(seq, at + a, b - a, lane);
        }
    }
    if ((o.flags & CUT_TAIL) && b > a) {
        const uint32_t nw = n_windows(a, b, o);
        uint32_t u = nw;
        if (nw) u = first_window<-1>(qual, at + b - o.cut_window, at + b, nw, range_sum<-1>(qual, at + b, o.cut_window, lane), o, lane);
        if (u == nw) b = a;
        else {
            b -= u;
            b -= n_run<-1>(seq, at + b, b - a, lane);
        }
    }
}

// what step 4 counts over [a, b) of that read: N / n, and positions below the qualified quality
__device__ __forceinline__ void span_counts(const uint8_t *seq, const uint8_t *qual, uint32_t start, uint32_t a, uint32_t b, const Opts &o,
                                            uint32_t lane, uint32_t &n_n, uint32_t &lowq) {
    n_n = 0, lowq = 0;
    if (b <= a) return;
    const uint64_t lo = (uint64_t)start + a, hi = (uint64_t)start + b, w_end = (hi + 3) >> 2; // the aligned words that cover [a, b)
    for (uint64_t w = (lo >> 2) + lane; w < w_end; w += 64) {
        const uint32_t vs = reinterpret_cast<const uint32_t *>(seq)[w], vq = reinterpret_cast<const uint32_t *>(qual)[w];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const bool in = (w << 2) + j >= lo && (w << 2) + j < hi;
            n_n += in && is_n(byte_of(vs, j)) ? 1u : 0u;
            lowq += in && phred(byte_of(vq, j)) < o.qualified_q ? 1u : 0u;
        }
    }
    n_n = wave_sum(n_n), lowq = wave_sum(lowq);
}

} // namespace srqc_dev
} // namespace np2
