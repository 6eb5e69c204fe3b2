// Short-read quality filter in front of the k-mer counter: one piece of the separator stream and of its quality stream ->
// per read (begin, end, class), the base stream masked in place, the totals.  The rule is np2_srqc_core.hpp's.
//
// Layout: a persistent grid strides over the reads, one wavefront per read (reads are 100 .. 300 bases: one pass of 64
// lanes x 4 bytes covers 256 of them, so nearly every step below is a single pass; any length and any W <= 1000 go
// through the same loops).  Every load is a lane's aligned 4-byte word (an unaligned group of 4 bytes is the funnel shift
// of two neighbouring aligned words); no lane walks a read.
//   windows  ws(u + 1) = ws(u) + p[entering] - p[leaving]: a lane takes 4 consecutive differences, a wave add-scan of the
//            lanes' sums plus the carry of the pass before gives every window's sum; the first window at or above M * W
//            is a ballot.  The front cut scans forward from a, the tail cut backward from b (a byte-reversed word), so
//            both stop at the first hit.  ws(0) is a wave reduction over the first (last) W values.
//   N skip   the same ballots over the base bytes, forward from the front cut and backward from the tail cut.
//   class    nN and lowq over [a, b) from the aligned words that cover it, two wave reductions.
//   mask     bytes of the read outside the kept span (all of a failed read) become 'N'.  Nothing is loaded for it: a word
//            that lies wholly inside the range to mask is one 4-byte store, the bytes of a word that the range shares
//            with anything else (the separator, a neighbouring read, the kept span) are byte stores.  A shared word is
//            owned by nobody: every read writes its own bytes of it and never a neighbour's, so no store carries a stale
//            copy of a byte another wavefront may be rewriting, and a separator is never written.
//   totals   kept per wavefront in registers, summed per block through LDS, one 64-bit atomic per block and counter.
// Traffic: 2 bytes read (base, quality) and at most 1 written per base; no table traffic.
//
// Memory the kernel may touch: 8 bytes before and 16 bytes after the n bytes of either stream must be readable (the
// counter's pieces have HALO bytes in front and 64 behind); what is read there enters no result.
#include <hip/hip_runtime.h>

#include "np2_srqc.hpp"

namespace np2 {
using namespace np2srqc;

namespace {

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

__global__ __launch_bounds__(SRQC_BLOCK) void k_srqc(uint8_t *seq, const uint8_t *qual, const uint32_t *ends, uint32_t n_reads, Opts o,
                                                    np2_srqc_read_t *reads, unsigned long long *totals) {
    __shared__ unsigned long long s_tot[SRQC_WAVES][N_TOTALS];
    const uint32_t lane = threadIdx.x & 63, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t n_waves = gridDim.x * SRQC_WAVES;
    unsigned long long tot[N_TOTALS] = {0, 0, 0, 0, 0, 0, 0}; // (the same in every lane of the wavefront)
    for (uint32_t r = blockIdx.x * SRQC_WAVES + wv; r < n_reads; r += n_waves) {
        const uint32_t start = r ? ends[r - 1] + 1 : 0u, n = ends[r] - start;
        uint32_t a, b;
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
        uint32_t n_n = 0, lowq = 0;
        if (b > a) { // the aligned words that cover [a, b)
            const uint64_t lo = (uint64_t)start + a, hi = (uint64_t)start + b, w_end = (hi + 3) >> 2;
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
        const uint32_t cls = classify(b - a, n_n, lowq, o);
        if (cls == PASS) {
            mask_range(seq, start, (uint64_t)start + a, lane);
            mask_range(seq, (uint64_t)start + b, (uint64_t)start + n, lane);
        } else {
            mask_range(seq, start, (uint64_t)start + n, lane);
        }
        if (reads && lane == 0) reads[r] = np2_srqc_read_t{a, b, cls};
        tot[T_READS] += 1, tot[T_BASES_IN] += n, tot[T_BASES_OUT] += cls == PASS ? b - a : 0u;
#pragma unroll
        for (uint32_t c = 0; c < N_CLASSES; ++c) tot[T_PASS + c] += cls == c ? 1u : 0u;
    }
    if (lane == 0)
        for (uint32_t i = 0; i < N_TOTALS; ++i) s_tot[wv][i] = tot[i];
    __syncthreads();
    if (threadIdx.x < N_TOTALS) {
        unsigned long long v = 0;
        for (uint32_t w = 0; w < SRQC_WAVES; ++w) v += s_tot[w][threadIdx.x];
        if (v) atomicAdd(totals + threadIdx.x, v);
    }
}

} // namespace

void launch_srqc(hipStream_t s, uint8_t *seq, const uint8_t *qual, const uint32_t *ends, uint32_t n_reads, const Opts &o,
                 np2_srqc_read_t *reads, uint64_t *totals) {
    if (!n_reads) return;
    const uint32_t want = (n_reads + SRQC_WAVES - 1) / SRQC_WAVES;
    hipLaunchKernelGGL(k_srqc, dim3(want < 2048u ? want : 2048u), dim3(SRQC_BLOCK), 0, s, seq, qual, ends, n_reads, o, reads,
                       reinterpret_cast<unsigned long long *>(totals));
}

} // namespace np2
