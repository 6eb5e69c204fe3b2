// K-mer QV scan: an assembly's bytes -> per sequence the number of k-mers and of k-mers the table does not hold, a count
// histogram and a bitmap of where the absent k-mers end.  Read-only on the table the polish kernels probe (YakDev).
// Bases, k-mers and hashes are np2_kcount_core.hpp's, counts and layouts np2_qv_core.hpp's (both also one-lane host
// programs).
//
// Input as in k_kcount: a block brings HALO + QV_TILE bytes into LDS with contiguous 16-byte loads, a lane rolls its words
// over the 32 bytes before its stretch and owns the k-mers that END inside it.  Every sequence starts at a tile boundary
// of the stream, so a tile belongs to one sequence; a sequence's first tile reads what lies before it as separators.
//
// Probes: k_kcount walks one dependent CAS chain per k-mer; this kernel only reads.  A lane hashes QV_GROUP k-mers, issues
// their first-slot loads back to back and only then looks at the words; the k-mers whose first slot held another key go
// on together, one more slot each per round, until every one met its key or an EMPTY slot.  Random 8-byte reads of a
// table of up to 1e9 words are bounded by latency: what counts is the number of independent loads in flight (8 per lane
// next to the other wavefronts of the CU), not the arithmetic.  Every probe loop is bounded by the sub-table's capacity.
//
// Counters: n_kmers / n_absent live in registers, the histogram in LDS; they reach global memory once per block and
// sequence change (one pair of atomics) and once per block and bin at the end.  The bitmap needs no atomics: a group of 8
// bases is one byte, a lane's stretch one 32-bit word, stored by the lane that owns it.
#include <hip/hip_runtime.h>

#include "np2_qv.hpp"

namespace np2 {
using namespace np2kc;
using namespace np2qv;

namespace {

static constexpr uint32_t QV_CHUNKS = (HALO + QV_TILE) / 16 + 1; // 16-byte pieces of a tile's window (+ 1: a source that is not 16-byte aligned)
static constexpr uint32_t PAD4 = 0x0A0A0A0Au;

// the block's k-mer counters of sequence `seq` -> global memory: wavefront sums, an LDS pair, one pair of atomics
__device__ __forceinline__ void qv_flush(uint32_t &n_kmers, uint32_t &n_absent, uint32_t *s_cnt, unsigned long long *stats, uint32_t seq) {
    uint32_t a = n_kmers, b = n_absent;
    for (int o = 32; o > 0; o >>= 1) {
        a += (uint32_t)__shfl_down((int)a, o);
        b += (uint32_t)__shfl_down((int)b, o);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (a) atomicAdd(&s_cnt[0], a);
        if (b) atomicAdd(&s_cnt[1], b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_cnt[0]) atomicAdd(&stats[2 * (uint64_t)seq], (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&stats[2 * (uint64_t)seq + 1], (unsigned long long)s_cnt[1]);
        s_cnt[0] = s_cnt[1] = 0;
    }
    __syncthreads();
    n_kmers = n_absent = 0;
}

} // namespace

__global__ __launch_bounds__(QV_BLOCK) void k_qv_scan(YakDev y, QvScan q) {
    __shared__ uint4 tile[QV_CHUNKS];
    __shared__ uint32_t s_hist[QV_HIST_BINS];
    __shared__ uint32_t s_cnt[2];
    const uint32_t tid = threadIdx.x;
    if (q.hist)
        for (uint32_t i = tid; i < QV_HIST_BINS; i += QV_BLOCK) s_hist[i] = 0;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();

    const uint32_t k = y.k;
    const uint64_t mask = kmer_mask(k);
    const uint64_t capm = (1ULL << y.cap_log2) - 1;
    // the source's misalignment is the same for every tile (HALO and QV_TILE are multiples of 16): the window in LDS starts
    // `shift` bytes early and a lane reads its dwords across two LDS words
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(q.src) & 15u);
    const uint32_t *lds = reinterpret_cast<const uint32_t *>(tile) + tid * (QV_STRETCH / 4) + (shift >> 2);
    const uint32_t bsh = (shift & 3u) * 8u;
    uint32_t cur = ~0u, n_kmers = 0, n_absent = 0;

    for (uint32_t t = blockIdx.x; t < q.n_tiles; t += gridDim.x) {
        const uint32_t d = q.desc ? q.desc[t] : 0u;
        const uint32_t seq = d & ~QV_FIRST;
        if (seq != cur) { // (the same for every lane of the block: a tile belongs to one sequence)
            if (cur != ~0u) qv_flush(n_kmers, n_absent, s_cnt, q.stats, cur);
            cur = seq;
        }
        const int64_t t0 = (int64_t)t * QV_TILE;
        const int64_t lo = (d & QV_FIRST) && t0 > q.lo ? t0 : q.lo;
        const int64_t w0 = t0 - (int64_t)HALO - (int64_t)shift; // stream offset of the window's first (aligned) 16 bytes
        for (uint32_t i = tid; i < QV_CHUNKS; i += QV_BLOCK) {
            const int64_t c0 = w0 + 16 * (int64_t)i;
            uint32_t w[4] = {PAD4, PAD4, PAD4, PAD4};
            if (c0 + 16 > lo && c0 < q.hi) { // holds a byte that may be read: the aligned 16 bytes around it are mapped
                const uint4 v = *reinterpret_cast<const uint4 *>(q.src + c0);
                w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
                if (c0 < lo || c0 + 16 > q.hi) { // the first / last load of a sequence: what lies outside is a separator
#pragma unroll
                    for (uint32_t b = 0; b < 16; ++b)
                        if (c0 + (int64_t)b < lo || c0 + (int64_t)b >= q.hi)
                            w[b >> 2] = (w[b >> 2] & ~(0xFFu << (8 * (b & 3)))) | ((uint32_t)QV_PAD << (8 * (b & 3)));
                }
            }
            tile[i] = make_uint4(w[0], w[1], w[2], w[3]);
        }
        __syncthreads();

        auto dword = [&](uint32_t i) { return (uint32_t)((((uint64_t)lds[i + 1] << 32) | lds[i]) >> bsh); };
        Roll r;
        uint64_t hh = 0;
#pragma unroll 1
        for (uint32_t i = 0; i < HALO / 4; ++i) {
            const uint32_t w = dword(i);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) (void)push(r, (uint8_t)(w >> (8 * j)), k, mask, &hh);
        }
        uint32_t lane_bits = 0;
#pragma unroll 1
        for (uint32_t g = 0; g < QV_STRETCH / QV_GROUP; ++g) {
            const uint32_t wa = dword(HALO / 4 + 2 * g), wb = dword(HALO / 4 + 2 * g + 1);
            uint64_t h[QV_GROUP];
            uint32_t cnt[QV_GROUP];
            uint32_t valid = 0;
#pragma unroll
            for (uint32_t j = 0; j < QV_GROUP; ++j) {
                h[j] = 0; // (a base no k-mer ends at probes slot 0 of sub-table 0: a valid address, its word is ignored)
                cnt[j] = 0;
                const bool ok = push(r, (uint8_t)((j < 4 ? wa : wb) >> (8 * (j & 3))), k, mask, &h[j]);
                if (!ok) h[j] = 0;
                valid |= (ok ? 1u : 0u) << j;
            }
            if (y.ord) { // a table that repeats keys (yak writes none): the whole probe cluster per k-mer
#pragma unroll
                for (uint32_t j = 0; j < QV_GROUP; ++j)
                    if ((valid >> j) & 1u) cnt[j] = qv_get_bounded(y, h[j], q.min_count);
            } else {
                // round 0: every first-slot load is issued before any word is looked at
                // (the scheduling barriers keep the compiler from sinking a word's use between the loads: without them it
                // issued 2, 1, 1 and 4 loads with a wait after each lot)
                uint64_t w[QV_GROUP];
                uint32_t s[QV_GROUP];
                const uint64_t *at[QV_GROUP];
#pragma unroll
                for (uint32_t j = 0; j < QV_GROUP; ++j) {
                    s[j] = (uint32_t)(key_of(h[j]) & capm);
                    at[j] = y.table + (((uint64_t)bucket_of(h[j]) << y.cap_log2) + s[j]);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (uint32_t j = 0; j < QV_GROUP; ++j) w[j] = *at[j];
                __builtin_amdgcn_sched_barrier(0);
                uint32_t pend = 0;
#pragma unroll
                for (uint32_t j = 0; j < QV_GROUP; ++j) {
                    const bool hit = (w[j] >> COUNT_BITS) == key_of(h[j]); // (EMPTY >> 10 is no key: a hash has 62 bits at most)
                    if (hit) cnt[j] = passing((uint32_t)(w[j] & COUNT_MAX), q.min_count);
                    pend |= (((valid >> j) & 1u) && !hit && w[j] != YAK_EMPTY ? 1u : 0u) << j;
                }
                // the k-mers whose slot held another key: one more slot each per round, again loaded together (a settled k-mer
                // loads its last slot again, a cache hit: eight unconditional loads are issued back to back, loads under a
                // lane's own condition were compiled into a load and a wait each)
                for (uint64_t probe = 1; pend && probe <= capm; ++probe) {
#pragma unroll
                    for (uint32_t j = 0; j < QV_GROUP; ++j) {
                        s[j] = (uint32_t)((s[j] + ((pend >> j) & 1u)) & capm);
                        w[j] = y.table[((uint64_t)bucket_of(h[j]) << y.cap_log2) + s[j]];
                    }
#pragma unroll
                    for (uint32_t j = 0; j < QV_GROUP; ++j)
                        if ((pend >> j) & 1u) {
                            const bool hit = (w[j] >> COUNT_BITS) == key_of(h[j]);
                            if (hit) cnt[j] = passing((uint32_t)(w[j] & COUNT_MAX), q.min_count);
                            if (hit || w[j] == YAK_EMPTY) pend &= ~(1u << j);
                        }
                }
            }
            uint32_t byte = 0;
#pragma unroll
            for (uint32_t j = 0; j < QV_GROUP; ++j) {
                tally((valid >> j) & 1u, cnt[j], j, n_kmers, n_absent, byte);
                if (q.hist && ((valid >> j) & 1u)) atomicAdd(&s_hist[cnt[j]], 1u);
            }
            lane_bits |= byte << (8 * g);
        }
        if (q.bits) q.bits[(uint64_t)t * QV_BLOCK + tid] = lane_bits;
        __syncthreads(); // (the next tile overwrites the window)
    }
    if (cur != ~0u) qv_flush(n_kmers, n_absent, s_cnt, q.stats, cur);
    if (q.hist) {
        __syncthreads();
        for (uint32_t i = tid; i < QV_HIST_BINS; i += QV_BLOCK) {
            const uint32_t v = s_hist[i];
            if (v) atomicAdd(&q.hist[i], (unsigned long long)v);
        }
    }
}

void launch_qv_scan(hipStream_t s, const YakDev &y, const QvScan &q, uint32_t blocks) {
    if (q.n_tiles == 0) return;
    hipLaunchKernelGGL(k_qv_scan, dim3(blocks < q.n_tiles ? (blocks ? blocks : 1u) : q.n_tiles), dim3(QV_BLOCK), 0, s, y, q);
}

} // namespace np2
