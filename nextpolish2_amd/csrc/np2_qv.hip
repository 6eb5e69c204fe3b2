// K-mer QV scan: an assembly's bytes -> per sequence the number of k-mers and of k-mers the table does not hold, a count
// histogram and a bitmap of where the absent k-mers end.  Read-only on the table the polish kernels probe (YakDev).
// Bases, k-mers and hashes are np2_kcount_core.hpp's, counts and layouts np2_qv_core.hpp's (both also one-lane host
// programs).
//
// Input and probes: the staging and probe contracts of np2_kmerscan.hpp.  stage_any brings a tile's window into LDS;
// every sequence starts at a tile boundary of the stream, so a tile belongs to one sequence, and a sequence's first tile
// reads what lies before it as separators.  A lane hashes QV_GROUP k-mers, issues their first-slot loads back to back and
// only then looks at the words (k_kcount walks one dependent CAS chain per k-mer; this kernel only reads).
//
// Counters: n_kmers / n_absent live in registers, the histogram in LDS; they reach global memory once per block and
// sequence change (one pair of atomics) and once per block and bin at the end.  The bitmap needs no atomics: a group of 8
// bases is one byte, a lane's stretch one 32-bit word, stored by the lane that owns it.
#include <hip/hip_runtime.h>

#include "np2_kmerscan.hpp"
#include "np2_qv.hpp"

namespace np2 {
using namespace np2kc;
using namespace np2qv;

namespace {

static constexpr uint32_t QV_CHUNKS = (HALO + QV_TILE) / 16 + 1; // 16-byte pieces of a tile's window (+ 1: a source that is not 16-byte aligned)
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
    const auto dword = lane_dwords<QV_STRETCH>(tile, q.in.src);
    uint32_t cur = ~0u, n[2] = {0, 0}; // k-mers and absent k-mers of sequence `cur`
    auto flush = [&] {
        block_flush<2>(true, n, s_cnt, q.stats + 2 * (uint64_t)cur);
        n[0] = n[1] = 0;
    };

    for (uint32_t t = blockIdx.x; t < q.in.n_tiles; t += gridDim.x) {
        const uint32_t d = q.in.desc ? q.in.desc[t] : 0u;
        const uint32_t seq = d & ~QV_FIRST;
        if (seq != cur) { // (the same for every lane of the block: a tile belongs to one sequence)
            if (cur != ~0u) flush();
            cur = seq;
        }
        stage_any<QV_BLOCK, QV_CHUNKS>(tile, q.in, (int64_t)t * QV_TILE, (d & QV_FIRST) != 0u);
        __syncthreads();

        Roll r;
        warm_halo(r, dword, k, mask);
        uint32_t lane_bits = 0;
#pragma unroll 1
        for (uint32_t g = 0; g < QV_STRETCH / QV_GROUP; ++g) {
            const uint32_t wa = dword(HALO / 4 + 2 * g), wb = dword(HALO / 4 + 2 * g + 1);
            uint64_t h[QV_GROUP];
            uint32_t cnt[QV_GROUP];
            const uint32_t valid = hash_group(r, wa, wb, k, mask, h);
            if (y.ord) { // a table that repeats keys (yak writes none): the whole probe cluster per k-mer
#pragma unroll
                for (uint32_t j = 0; j < QV_GROUP; ++j) cnt[j] = ((valid >> j) & 1u) ? qv_get_bounded(y, h[j], q.min_count) : 0u;
            } else {
                // round 0: every first-slot load is issued before any word is looked at
                // (the scheduling barriers keep the compiler from sinking a word's use between the loads: without them it
                // issued 2, 1, 1 and 4 loads with a wait after each lot)
                uint64_t w[QV_GROUP];
                __builtin_amdgcn_sched_barrier(0);
                probe_issue(y.table, y.cap_log2, h, w);
                __builtin_amdgcn_sched_barrier(0);
                probe_settle(y.table, y.cap_log2, h, valid, w, cnt);
#pragma unroll
                for (uint32_t j = 0; j < QV_GROUP; ++j) cnt[j] = passing(cnt[j], q.min_count);
            }
            uint32_t byte = 0;
#pragma unroll
            for (uint32_t j = 0; j < QV_GROUP; ++j) {
                tally((valid >> j) & 1u, cnt[j], j, n[0], n[1], byte);
                if (q.hist && ((valid >> j) & 1u)) atomicAdd(&s_hist[cnt[j]], 1u);
            }
            lane_bits |= byte << (8 * g);
        }
        if (q.bits) q.bits[(uint64_t)t * QV_BLOCK + tid] = lane_bits;
        __syncthreads(); // (the next tile overwrites the window)
    }
    if (cur != ~0u) flush();
    if (q.hist) {
        __syncthreads();
        for (uint32_t i = tid; i < QV_HIST_BINS; i += QV_BLOCK) {
            const uint32_t v = s_hist[i];
            if (v) atomicAdd(&q.hist[i], (unsigned long long)v);
        }
    }
}

void launch_qv_scan(hipStream_t s, const YakDev &y, const QvScan &q, uint32_t blocks) {
    if (q.in.n_tiles == 0) return;
    hipLaunchKernelGGL(k_qv_scan, dim3(blocks < q.in.n_tiles ? (blocks ? blocks : 1u) : q.in.n_tiles), dim3(QV_BLOCK), 0, s, y, q);
}

} // namespace np2
