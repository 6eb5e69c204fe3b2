// K-mer counting on the device: a separator stream of read bytes -> the HBM table the polish kernels probe (YakDev:
// 1024 sub-tables by hash & 1023, linear probing on hash >> 10, slot = file word (hash >> 10) << 10 | count, EMPTY = ~0).
// The per-lane arithmetic is np2_kcount_core.hpp (also a one-lane host program); this file adds the table update.
//
// How a slot is updated, and why it is exact under races:
//   * an EMPTY slot is claimed by atomicCAS(EMPTY -> key | add); exactly one lane wins, the others see the winner's word;
//   * a slot never changes its key once claimed, so a lane that found its key increments the count with a CAS LOOP ON THE
//     WORD (old -> old with count = min(1023, count + add)): the count saturates at 1023 and can never carry into the key
//     bits; a failed CAS means another lane's succeeded, so the loop ends after at most 1023 failures;
//   * a slot whose count is already 1023 is left alone after a plain load: a hot k-mer (homopolymer, satellite) costs no
//     atomic from then on;
//   * every probe loop is bounded by the sub-table's capacity.  A lane that probed a whole sub-table without finding its
//     key or an EMPTY slot appends its hash to the spill list (one atomicAdd per wavefront for the places); the host grows
//     the table and replays the list through the same insert (k_kcount_insert_hashes) before the next piece.
// Newly claimed slots and hashed k-mers are summed per wavefront and added with one atomicAdd each per wavefront.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "np2_kcount.hpp"
#include "np2_kcount_core.hpp"
#include "np2_kmerscan.hpp"

namespace np2 {
using namespace np2kc;

namespace {

enum : uint32_t { KC_COUNTED = 0, KC_NEW = 1, KC_FULL = 2 };

__device__ __forceinline__ uint32_t kc_add(const KcTable &t, uint64_t h, uint32_t add) {
    const uint64_t capm = (1ULL << t.cap_log2) - 1;
    unsigned long long *tb = (unsigned long long *)t.table + ((uint64_t)(bucket_of(h) - t.bucket_lo) << t.cap_log2);
    const uint64_t key = key_of(h);
    uint64_t s = key & capm;
    for (uint64_t probe = 0; probe <= capm; ++probe, s = (s + 1) & capm) {
        unsigned long long w = __hip_atomic_load(&tb[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (w == EMPTY) {
            w = atomicCAS(&tb[s], (unsigned long long)EMPTY, (unsigned long long)(key << COUNT_BITS | add));
            if (w == EMPTY) return KC_NEW;
        }
        if ((w >> COUNT_BITS) != key) continue;
        for (;;) {
            const uint32_t c = (uint32_t)(w & COUNT_MAX);
            if (c >= COUNT_MAX) return KC_COUNTED;
            const unsigned long long nw = (w & ~(unsigned long long)COUNT_MAX) | sat_add(c, add);
            const unsigned long long old = atomicCAS(&tb[s], w, nw);
            if (old == w) return KC_COUNTED;
            w = old;
        }
    }
    return KC_FULL;
}

// every lane of the wavefront calls it (converged); lanes with `full` set get a place in the spill list
__device__ __forceinline__ void kc_spill(bool full, uint64_t h, uint64_t *ctr, uint64_t *spill) {
    const uint64_t m = __ballot(full);
    if (m == 0) return;
    const uint32_t lane = __lane_id();
    const uint32_t leader = (uint32_t)__ffsll((unsigned long long)m) - 1u;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd((unsigned long long *)&ctr[KC_SPILLED], (unsigned long long)__popcll(m));
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)base, (int)leader);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), (int)leader);
    if (full) spill[((uint64_t)hi << 32 | lo) + (uint64_t)__popcll(m & ((1ULL << lane) - 1ULL))] = h;
}

__device__ __forceinline__ void kc_wave_add(uint32_t v, uint64_t *dst) {
    v = wave_sum(v);
    if (__lane_id() == 0 && v) atomicAdd((unsigned long long *)dst, (unsigned long long)v);
}

} // namespace

// One block owns KC_TILE bytes of the piece (the staging contract of np2_kmerscan.hpp, stage_aligned) and counts the
// k-mers that END inside it.
__global__ __launch_bounds__(KC_BLOCK) void k_kcount(const uint8_t *__restrict__ in, uint64_t n, uint32_t k, KcTable t,
                                                     uint64_t *__restrict__ ctr, uint64_t *__restrict__ spill) {
    __shared__ uint4 tile[(HALO + KC_TILE) / 16];
    // `in` offset of the tile's halo = piece offset of its first byte (the host pads the buffer with '\n' to a multiple of 16)
    stage_aligned<KC_BLOCK, (HALO + KC_TILE) / 16>(tile, in, (int64_t)blockIdx.x * KC_TILE, (int64_t)(HALO + n));
    __syncthreads();
    const uint32_t *lw = reinterpret_cast<const uint32_t *>(tile) + threadIdx.x * (KC_STRETCH / 4);
    const uint64_t mask = kmer_mask(k);
    Roll r;
    uint64_t h = 0;
    warm_halo(r, [&](uint32_t d) { return lw[d]; }, k, mask);
    uint32_t claimed = 0, kmers = 0;
#pragma unroll 1
    for (uint32_t d = 0; d < KC_STRETCH / 4; ++d) {
        const uint32_t w = lw[HALO / 4 + d];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            bool ok = push(r, (uint8_t)(w >> (8 * j)), k, mask, &h);
            ok = ok && bucket_of(h) >= t.bucket_lo && bucket_of(h) < t.bucket_hi;
            uint32_t res = KC_COUNTED;
            if (ok) res = kc_add(t, h, 1u);
            kmers += ok ? 1u : 0u;
            claimed += res == KC_NEW ? 1u : 0u;
            kc_spill(res == KC_FULL, h, ctr, spill);
        }
    }
    kc_wave_add(claimed, &ctr[KC_CLAIMED]);
    kc_wave_add(kmers, &ctr[KC_KMERS]);
}

// the spill list of a piece, after the table grew: the same insert, one hash a lane
__global__ __launch_bounds__(KC_BLOCK) void k_kcount_insert_hashes(const uint64_t *__restrict__ hashes, uint64_t n, KcTable t,
                                                                   uint64_t *__restrict__ ctr, uint64_t *__restrict__ spill) {
    uint32_t claimed = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * KC_BLOCK; base < n; base += (uint64_t)gridDim.x * KC_BLOCK) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t h = i < n ? hashes[i] : 0;
        uint32_t res = KC_COUNTED;
        if (i < n) res = kc_add(t, h, 1u);
        claimed += res == KC_NEW ? 1u : 0u;
        kc_spill(res == KC_FULL, h, ctr, spill);
    }
    kc_wave_add(claimed, &ctr[KC_CLAIMED]);
}

// every word of `from` into `to` (twice the capacity or more), counts kept; a word that finds its sub-table of `to` full
// is counted in ctr[KC_REHASH_FAIL] (the host then takes a larger `to` and starts over from `from`)
__global__ __launch_bounds__(KC_BLOCK) void k_kcount_rehash(KcTable from, KcTable to, uint64_t *__restrict__ ctr) {
    const uint64_t slots = (uint64_t)(from.bucket_hi - from.bucket_lo) << from.cap_log2;
    for (uint64_t i = (uint64_t)blockIdx.x * KC_BLOCK + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * KC_BLOCK) {
        const uint64_t w = from.table[i];
        if (w == EMPTY) continue;
        const uint64_t h = (w >> COUNT_BITS) << PRE | (uint64_t)(from.bucket_lo + (uint32_t)(i >> from.cap_log2));
        if (kc_add(to, h, (uint32_t)(w & COUNT_MAX)) == KC_FULL) atomicAdd((unsigned long long *)&ctr[KC_REHASH_FAIL], 1ULL);
    }
}

// one block per sub-table: its slots with count >= min_count
__global__ __launch_bounds__(KC_BLOCK) void k_kcount_bucket_sizes(KcTable t, uint32_t min_count, uint32_t *__restrict__ sizes) {
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const uint64_t *tb = t.table + ((uint64_t)blockIdx.x << t.cap_log2);
    uint32_t c = 0;
    for (uint64_t i = threadIdx.x; i < (1ULL << t.cap_log2); i += KC_BLOCK) {
        const uint64_t w = tb[i];
        c += (w != EMPTY && (uint32_t)(w & COUNT_MAX) >= min_count) ? 1u : 0u;
    }
    c = wave_sum(c);
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&total, c);
    __syncthreads();
    if (threadIdx.x == 0) sizes[blockIdx.x] = total;
}

// Compaction, one block per sub-table: the surviving slots of sub-table b as (bucket << 52 | slot key, count) pairs at
// off[b] .. off[b + 1] (the prefix sums of k_kcount_bucket_sizes' counts), places inside the bucket taken per wavefront from a
// counter in LDS — no global atomic (a first version took its places from one device counter: 131 k same-address atomics
// made it as slow as the count kernel itself on the test reads).  The order inside a bucket is whatever the atomics gave;
// the sort that follows (ascending word order inside every bucket) makes the output canonical.
__global__ __launch_bounds__(KC_BLOCK) void k_kcount_emit(KcTable t, uint32_t min_count, const uint64_t *__restrict__ off,
                                                          uint64_t *__restrict__ keys, uint32_t *__restrict__ counts) {
    __shared__ uint32_t taken;
    if (threadIdx.x == 0) taken = 0;
    __syncthreads();
    const uint32_t b = blockIdx.x;
    const uint64_t *tb = t.table + ((uint64_t)b << t.cap_log2);
    const uint64_t o0 = off[b], room = off[b + 1] - o0;
    for (uint64_t base = 0; base < (1ULL << t.cap_log2); base += KC_BLOCK) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t w = i < (1ULL << t.cap_log2) ? tb[i] : EMPTY;
        const bool keep = w != EMPTY && (uint32_t)(w & COUNT_MAX) >= min_count;
        const uint64_t m = __ballot(keep);
        if (m == 0) continue;
        const uint32_t lane = __lane_id();
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)m) - 1u;
        uint32_t at = 0;
        if (lane == leader) at = atomicAdd(&taken, (uint32_t)__popcll(m));
        at = (uint32_t)__shfl((int)at, (int)leader) + (uint32_t)__popcll(m & ((1ULL << lane) - 1ULL));
        if (keep && at < room) { // (at < room always: the same predicate over the same table gave the sizes)
            keys[o0 + at] = (uint64_t)(t.bucket_lo + b) << 52 | (w >> COUNT_BITS);
            counts[o0 + at] = (uint32_t)(w & COUNT_MAX);
        }
    }
}

__global__ __launch_bounds__(KC_BLOCK) void k_kcount_words(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ counts,
                                                           uint64_t n, uint64_t *__restrict__ words) {
    for (uint64_t i = (uint64_t)blockIdx.x * KC_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * KC_BLOCK)
        words[i] = (keys[i] & ((1ULL << 52) - 1ULL)) << COUNT_BITS | (uint64_t)counts[i];
}

namespace {
uint32_t kc_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>((items + KC_BLOCK - 1) / KC_BLOCK, 1u << 16); }
} // namespace

void launch_kcount(hipStream_t s, const uint8_t *in, uint64_t n, uint32_t k, const KcTable &t, uint64_t *ctr, uint64_t *spill) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_kcount, dim3((uint32_t)((n + KC_TILE - 1) / KC_TILE)), dim3(KC_BLOCK), 0, s, in, n, k, t, ctr, spill);
}
void launch_kcount_insert_hashes(hipStream_t s, const uint64_t *hashes, uint64_t n, const KcTable &t, uint64_t *ctr, uint64_t *spill) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_kcount_insert_hashes, dim3(kc_grid(n)), dim3(KC_BLOCK), 0, s, hashes, n, t, ctr, spill);
}
void launch_kcount_rehash(hipStream_t s, const KcTable &from, const KcTable &to, uint64_t *ctr) {
    const uint64_t slots = (uint64_t)(from.bucket_hi - from.bucket_lo) << from.cap_log2;
    hipLaunchKernelGGL(k_kcount_rehash, dim3(kc_grid(slots)), dim3(KC_BLOCK), 0, s, from, to, ctr);
}
void launch_kcount_bucket_sizes(hipStream_t s, const KcTable &t, uint32_t min_count, uint32_t *sizes) {
    hipLaunchKernelGGL(k_kcount_bucket_sizes, dim3(t.bucket_hi - t.bucket_lo), dim3(KC_BLOCK), 0, s, t, min_count, sizes);
}
void launch_kcount_emit(hipStream_t s, const KcTable &t, uint32_t min_count, const uint64_t *off, uint64_t *keys, uint32_t *counts) {
    hipLaunchKernelGGL(k_kcount_emit, dim3(t.bucket_hi - t.bucket_lo), dim3(KC_BLOCK), 0, s, t, min_count, off, keys, counts);
}
void launch_kcount_words(hipStream_t s, const uint64_t *keys, const uint32_t *counts, uint64_t n, uint64_t *words) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_kcount_words, dim3(kc_grid(n)), dim3(KC_BLOCK), 0, s, keys, counts, n, words);
}

} // namespace np2
