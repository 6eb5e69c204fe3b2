// The repetitive k-mer list on the device (the rule: include/np2_io.h; meryl count + meryl print greater-than distinct=):
// a direct-addressed uint32 counter per 2k-bit word (4^k of them, 4 GiB at k = 15), an exact selection of the threshold
// over the counters without sorting them, and an ordered compaction of the counters above it.  The per-lane arithmetic
// is np2_rep_core.hpp (also a one-lane host program).
//
// Bounds.  k_rep_count: an index is min(fw, rv) <= 4^k - 1 (np2rep::push), the table has 4^k counters; the tile is read
// as k_kcount reads it.  A counter cannot wrap: the host refuses a stream that could hold more than 2^32 - 1 k-mers.
// k_rep_hist / k_rep_sizes / k_rep_emit read the table as uint4: 4^k is a multiple of 4 for k >= 1, every load is guarded by
// the number of uint4s.  Histogram bins are c >> 16 and c & 65535, both below REP_HALF; the LDS bins are guarded by
// REP_LO_LDS.  k_rep_emit writes at off[chunk] + rank with rank below the chunk's own count, which k_rep_sizes took with the
// same predicate from the same table: below off[chunk + 1], and the arrays hold off[chunks] entries.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "np2_blockscan.hpp"
#include "np2_kcount.hpp"
#include "np2_kmerscan.hpp"
#include "np2_rep.hpp"
#include "np2_rep_core.hpp"

namespace np2 {
using np2kc::HALO;

// The tiling of k_kcount (the staging contract of np2_kmerscan.hpp, stage_aligned): a lane counts the k-mers that END inside
// its 32 bytes.  The update is one atomicAdd (no return value) on the k-mer's counter.  A homopolymer or a satellite sends
// every k-mer of a stretch to one or two addresses, so with COLLAPSE a lane keeps (index, run length) and adds once when
// the index changes: a 300 000-base homopolymer costs 9 400 adds on its counter instead of 300 000.
template <bool COLLAPSE>
__global__ __launch_bounds__(KC_BLOCK) void k_rep_count(const uint8_t *__restrict__ in, uint64_t n, uint32_t k, uint32_t *__restrict__ count) {
    __shared__ uint4 tile[(HALO + KC_TILE) / 16];
    // `in` offset of the tile's halo = piece offset of its first byte (the host pads the buffer with '\n' to a multiple of 16)
    stage_aligned<KC_BLOCK, (HALO + KC_TILE) / 16>(tile, in, (int64_t)blockIdx.x * KC_TILE, (int64_t)(HALO + n));
    __syncthreads();
    const uint32_t *lw = reinterpret_cast<const uint32_t *>(tile) + threadIdx.x * (KC_STRETCH / 4);
    const uint64_t mask = np2kc::kmer_mask(k);
    np2kc::Roll r;
    uint32_t v = 0;
    warm_halo(r, [&](uint32_t d) { return lw[d]; }, k, mask);
    uint32_t run_v = 0, run_n = 0;
#pragma unroll 1
    for (uint32_t d = 0; d < KC_STRETCH / 4; ++d) {
        const uint32_t w = lw[HALO / 4 + d];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            if (!np2rep::push(r, (uint8_t)(w >> (8 * j)), k, mask, &v)) continue;
            if (!COLLAPSE) {
                atomicAdd(&count[v], 1u);
            } else if (run_n && v == run_v) {
                ++run_n;
            } else {
                if (run_n) atomicAdd(&count[run_v], run_n);
                run_v = v, run_n = 1;
            }
        }
    }
    if (COLLAPSE && run_n) atomicAdd(&count[run_v], run_n);
}

// The selection's pass over the table, a grid-stride loop of uint4 loads.  Almost every counter is 0 or small, so what is
// common never reaches a global atomic: the high-half bin 0, the counters above 0, their sum and maximum are per-lane
// registers, summed per wavefront, one atomic per wavefront at the end; low halves 1, 2, 3 are registers too, the other low
// halves below REP_LO_LDS an LDS histogram the block adds to the global one once.  Only a counter of 65 536 and more (high
// half) or a low half of 4096 and more goes to memory directly.
__global__ __launch_bounds__(REP_BLOCK) void k_rep_hist(const uint32_t *__restrict__ count, uint64_t n4, uint32_t bin, uint32_t first,
                                                        uint32_t *__restrict__ hist_hi, uint32_t *__restrict__ hist_lo,
                                                        unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t lo[REP_LO_LDS];
    for (uint32_t i = threadIdx.x; i < REP_LO_LDS; i += REP_BLOCK) lo[i] = 0;
    __syncthreads();
    uint32_t distinct = 0, hi0 = 0, mx = 0, n1 = 0, n2 = 0, n3 = 0;
    unsigned long long sum = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * REP_BLOCK + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * REP_BLOCK) {
        const uint4 q = reinterpret_cast<const uint4 *>(count)[i];
        const uint32_t c4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t c = c4[j];
            if (c == 0) continue;
            const uint32_t hi = c >> 16, l = c & (REP_HALF - 1);
            ++distinct, sum += c, mx = max(mx, c);
            if (hi == 0) ++hi0;
            else if (first) atomicAdd(&hist_hi[hi], 1u);
            if (hi != bin) continue;
            if (l == 1) ++n1;
            else if (l == 2) ++n2;
            else if (l == 3) ++n3;
            else if (l < REP_LO_LDS) atomicAdd(&lo[l], 1u);
            else atomicAdd(&hist_lo[l], 1u);
        }
    }
    n1 = wave_sum(n1), n2 = wave_sum(n2), n3 = wave_sum(n3);
    if (__lane_id() == 0) {
        if (n1) atomicAdd(&lo[1], n1);
        if (n2) atomicAdd(&lo[2], n2);
        if (n3) atomicAdd(&lo[3], n3);
    }
    if (first) { // (uniform)
        distinct = wave_sum(distinct), hi0 = wave_sum(hi0);
        for (int o = 32; o > 0; o >>= 1) {
            sum += __shfl_down(sum, o);
            mx = max(mx, (uint32_t)__shfl_down((int)mx, o));
        }
        if (__lane_id() == 0 && distinct) {
            atomicAdd(&ctr[REP_DISTINCT], (unsigned long long)distinct);
            atomicAdd(&ctr[REP_TOTAL], sum);
            atomicMax(&ctr[REP_MAX], (unsigned long long)mx);
            if (hi0) atomicAdd(&hist_hi[0], hi0);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < REP_LO_LDS; i += REP_BLOCK)
        if (lo[i]) atomicAdd(&hist_lo[i], lo[i]);
}

// a lane's uint4 of slab s of chunk `chunk` (zeros beyond the table) and the index of its first counter
__device__ __forceinline__ uint4 rep_slab(const uint32_t *__restrict__ count, uint64_t n4, uint32_t chunk, uint32_t s, uint64_t *first) {
    const uint64_t i4 = (uint64_t)chunk * (REP_CHUNK / 4) + s * REP_BLOCK + threadIdx.x;
    *first = i4 * 4;
    return i4 < n4 ? reinterpret_cast<const uint4 *>(count)[i4] : make_uint4(0, 0, 0, 0);
}

// one block per chunk of REP_CHUNK counters: those above the threshold
__global__ __launch_bounds__(REP_BLOCK) void k_rep_sizes(const uint32_t *__restrict__ count, uint64_t n4, uint32_t threshold,
                                                         uint32_t *__restrict__ sizes) {
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    uint32_t c = 0;
#pragma unroll
    for (uint32_t s = 0; s < REP_CHUNK / REP_SLAB; ++s) {
        uint64_t at;
        const uint4 q = rep_slab(count, n4, blockIdx.x, s, &at);
        c += (q.x > threshold) + (q.y > threshold) + (q.z > threshold) + (q.w > threshold);
    }
    c = wave_sum(c);
    if (__lane_id() == 0 && c) atomicAdd(&total, c);
    __syncthreads();
    if (threadIdx.x == 0) sizes[blockIdx.x] = total;
}

// Ordered compaction, one block per chunk.  A chunk that holds nothing above the threshold (off[chunk] == off[chunk + 1]:
// all but a few at distinct = 0.9998) returns before it reads a counter.  Otherwise slab by slab: a lane's uint4 is four
// consecutive indices, the lanes' counts are scanned across the block (np2_blockscan.hpp), so places ascend with the index.
__global__ __launch_bounds__(REP_BLOCK) void k_rep_emit(const uint32_t *__restrict__ count, uint64_t n4, uint32_t threshold,
                                                        const uint32_t *__restrict__ off, uint32_t *__restrict__ index,
                                                        uint32_t *__restrict__ counts) {
    __shared__ uint32_t sh[REP_BLOCK / 64];
    uint32_t base = off[blockIdx.x];
    const uint32_t end = off[blockIdx.x + 1];
    if (base == end) return; // (uniform: before any barrier)
#pragma unroll 1
    for (uint32_t s = 0; s < REP_CHUNK / REP_SLAB; ++s) {
        uint64_t at;
        const uint4 q = rep_slab(count, n4, blockIdx.x, s, &at);
        const uint32_t c4[4] = {q.x, q.y, q.z, q.w};
        uint32_t mine = 0, slab_total = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) mine += c4[j] > threshold ? 1u : 0u;
        uint32_t place = base + block_excl_scan<OpAdd, REP_BLOCK / 64>(mine, sh, slab_total);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (c4[j] > threshold) {
                if (place < end) index[place] = (uint32_t)(at + j), counts[place] = c4[j];
                ++place;
            }
        base += slab_total;
    }
}

void launch_rep_count(hipStream_t s, const uint8_t *in, uint64_t n, uint32_t k, uint32_t *count, bool collapse) {
    if (n == 0) return;
    const dim3 grid((uint32_t)((n + KC_TILE - 1) / KC_TILE));
    if (collapse) hipLaunchKernelGGL(k_rep_count<true>, grid, dim3(KC_BLOCK), 0, s, in, n, k, count);
    else hipLaunchKernelGGL(k_rep_count<false>, grid, dim3(KC_BLOCK), 0, s, in, n, k, count);
}
void launch_rep_hist(hipStream_t s, const uint32_t *count, uint64_t table, uint32_t bin, bool first, uint32_t *hist_hi,
                     uint32_t *hist_lo, unsigned long long *ctr, uint32_t blocks) {
    const uint64_t n4 = table / 4;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (n4 + REP_BLOCK - 1) / REP_BLOCK));
    hipLaunchKernelGGL(k_rep_hist, dim3(grid), dim3(REP_BLOCK), 0, s, count, n4, bin, first ? 1u : 0u, hist_hi, hist_lo, ctr);
}
void launch_rep_sizes(hipStream_t s, const uint32_t *count, uint64_t table, uint32_t threshold, uint32_t *sizes) {
    hipLaunchKernelGGL(k_rep_sizes, dim3((uint32_t)rep_chunks(table)), dim3(REP_BLOCK), 0, s, count, table / 4, threshold, sizes);
}
void launch_rep_emit(hipStream_t s, const uint32_t *count, uint64_t table, uint32_t threshold, const uint32_t *off,
                     uint32_t *index, uint32_t *counts) {
    hipLaunchKernelGGL(k_rep_emit, dim3((uint32_t)rep_chunks(table)), dim3(REP_BLOCK), 0, s, count, table / 4, threshold, off, index, counts);
}

} // namespace np2
