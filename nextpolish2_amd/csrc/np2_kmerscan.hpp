// Device toolbox of the k-mer scans (np2_qv.hip, np2_trio.hip, np2_bin.hip, np2_cmp.hip, np2_kcount.hip, np2_rep.hip,
// np2_edits.hip): the window stagers, the halo warm-up, the group hasher, the grouped table probe, the bounded single
// lookup and the counter flushes.  Plain inline functions; every kernel keeps its own tile loop, counters and order logic.
//
// Staging contract.  A block brings HALO + TILE bytes of a stream into LDS with aligned 16-byte loads (TILE = THREADS *
// STRETCH); a lane rolls its words over the HALO bytes before its stretch (the window of a k-mer is the last k <= 32 bytes,
// so rolling more of them changes nothing) and owns the k-mers that END inside its stretch.  Bytes that are not the
// stream's read as the separator '\n', which resets the k-mer run like any non-base.
//   stage_any      a source of any alignment with nothing readable promised around [lo, hi): only the aligned 16 bytes
//                  that hold a byte of [lo, hi) are loaded, the first and last load are masked.  The window in LDS starts
//                  `shift` = src & 15 bytes early (the same for every tile: HALO and TILE are multiples of 16, hence CHUNKS
//                  = (HALO + TILE) / 16 + 1) and a lane reads its dwords across two LDS words: lane_dwords.
//   stage_aligned  a 16-byte aligned source whose halo is always there: CHUNKS = (HALO + TILE) / 16, loads at or beyond
//                  `hi` are skipped, the last one is masked, a lane reads its words as they lie.
//
// Probe contract (yak_get's rule, np2_kernels.hpp: sub-table hash & 1023, start at (hash >> 10) & capm, linear, wrapping
// inside the sub-table, stop at the key or at EMPTY).  A lane has G k-mers in flight: probe_issue loads their first slots
// back to back, probe_settle looks at the words; the k-mers whose slot held another key go on together, one more slot each
// per round, again loaded back to back.  Random 8-byte reads of a table beyond the caches are bounded by latency: what
// counts is the number of independent loads in flight, not the arithmetic.  A k-mer that is not valid has hash 0 and
// probes slot 0 of sub-table 0: a valid address, its word is ignored.  Every probe loop is bounded by the sub-table's
// capacity (a counting table's sub-table may be full).  The callers put their scheduling barriers around probe_issue.
#pragma once
#include <hip/hip_runtime.h>

#include "np2_qv.hpp"

namespace np2 {

static constexpr uint32_t PAD4 = 0x0A0A0A0Au; // QV_PAD four times

// of the 16 bytes at stream offset c0: those outside [lo, hi) become separators
__device__ __forceinline__ void pad_outside(uint32_t (&w)[4], int64_t c0, int64_t lo, int64_t hi) {
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b)
        if (c0 + (int64_t)b < lo || c0 + (int64_t)b >= hi)
            w[b >> 2] = (w[b >> 2] & ~(0xFFu << (8 * (b & 3)))) | ((uint32_t)np2qv::QV_PAD << (8 * (b & 3)));
}

// the window of the tile at stream offset t0; `first`: the tile starts a sequence, what lies before it is another one's
template <uint32_t THREADS, uint32_t CHUNKS>
__device__ __forceinline__ void stage_any(uint4 *tile, const ScanStream &in, int64_t t0, bool first) {
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(in.src) & 15u);
    const int64_t lo = first && t0 > in.lo ? t0 : in.lo;
    const int64_t w0 = t0 - (int64_t)np2kc::HALO - (int64_t)shift; // stream offset of the window's first (aligned) 16 bytes
    for (uint32_t i = threadIdx.x; i < CHUNKS; i += THREADS) {
        const int64_t c0 = w0 + 16 * (int64_t)i;
        uint32_t w[4] = {PAD4, PAD4, PAD4, PAD4};
        if (c0 + 16 > lo && c0 < in.hi) { // holds a byte that may be read: the aligned 16 bytes around it are mapped
            const uint4 v = *reinterpret_cast<const uint4 *>(in.src + c0);
            w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
            if (c0 < lo || c0 + 16 > in.hi) pad_outside(w, c0, lo, in.hi); // the first / last load of a sequence
        }
        tile[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// dword i of this lane's HALO + STRETCH bytes in a window staged by stage_any from `src`
template <uint32_t STRETCH> __device__ __forceinline__ auto lane_dwords(const uint4 *tile, const uint8_t *src) {
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u);
    const uint32_t *lds = reinterpret_cast<const uint32_t *>(tile) + threadIdx.x * (STRETCH / 4) + (shift >> 2);
    const uint32_t bsh = (shift & 3u) * 8u;
    return [=](uint32_t i) { return (uint32_t)((((uint64_t)lds[i + 1] << 32) | lds[i]) >> bsh); };
}

// the window whose first 16 bytes are src + w0 (aligned); offsets at or beyond `hi` are separators
template <uint32_t THREADS, uint32_t CHUNKS>
__device__ __forceinline__ void stage_aligned(uint4 *tile, const uint8_t *src, int64_t w0, int64_t hi) {
    for (uint32_t i = threadIdx.x; i < CHUNKS; i += THREADS) {
        const int64_t c0 = w0 + 16 * (int64_t)i;
        uint32_t w[4] = {PAD4, PAD4, PAD4, PAD4};
        if (c0 < hi) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + c0);
            w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
            if (c0 + 16 > hi) pad_outside(w, c0, INT64_MIN, hi); // the stream's last load
        }
        tile[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// a lane's words over the HALO bytes before its stretch.  (np2_rep.hip uses it too: np2rep::push rolls the same words,
// only what it reports of a whole k-mer differs, and nothing is reported here.)
template <class Dword> __device__ __forceinline__ void warm_halo(np2kc::Roll &r, Dword dword, uint32_t k, uint64_t mask) {
    uint64_t h = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < np2kc::HALO / 4; ++i) {
        const uint32_t w = dword(i);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) (void)np2kc::push(r, (uint8_t)(w >> (8 * j)), k, mask, &h);
    }
}

// the next eight bytes (wa, then wb) -> h[j]: the hash of the k-mer that ends at byte j, 0 where none does; bit j of the
// result says which
__device__ __forceinline__ uint32_t hash_group(np2kc::Roll &r, uint32_t wa, uint32_t wb, uint32_t k, uint64_t mask, uint64_t (&h)[8]) {
    uint32_t valid = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        h[j] = 0;
        const bool ok = np2kc::push(r, (uint8_t)((j < 4 ? wa : wb) >> (8 * (j & 3))), k, mask, &h[j]);
        if (!ok) h[j] = 0;
        valid |= (ok ? 1u : 0u) << j;
    }
    return valid;
}

// round 0 of one table: the first-slot words of a lane's group
template <uint32_t G>
__device__ __forceinline__ void probe_issue(const uint64_t *table, uint32_t cap_log2, const uint64_t (&h)[G], uint64_t (&w)[G]) {
    const uint64_t capm = (1ULL << cap_log2) - 1;
#pragma unroll
    for (uint32_t j = 0; j < G; ++j) w[j] = table[((uint64_t)np2kc::bucket_of(h[j]) << cap_log2) + (np2kc::key_of(h[j]) & capm)];
}

// one table's stored counts (0: not there) from the first-slot words `w`, and the collision rounds.  A settled k-mer loads
// its first slot again, a cache hit: unconditional loads are issued back to back (loads under a lane's own condition were
// compiled into a load and a wait each), and the slot is the round's number, no index to keep per k-mer.
template <uint32_t G>
__device__ __forceinline__ void probe_settle(const uint64_t *table, uint32_t cap_log2, const uint64_t (&h)[G], uint32_t valid,
                                             uint64_t (&w)[G], uint32_t (&cnt)[G]) {
    const uint64_t capm = (1ULL << cap_log2) - 1;
    uint32_t pend = 0;
#pragma unroll
    for (uint32_t j = 0; j < G; ++j) {
        const bool hit = (w[j] >> np2kc::COUNT_BITS) == np2kc::key_of(h[j]); // (EMPTY >> 10 is no key: a hash has 62 bits at most)
        cnt[j] = hit ? (uint32_t)(w[j] & np2kc::COUNT_MAX) : 0u;
        pend |= (((valid >> j) & 1u) && !hit && w[j] != YAK_EMPTY ? 1u : 0u) << j;
    }
    for (uint64_t probe = 1; pend && probe <= capm; ++probe) {
#pragma unroll
        for (uint32_t j = 0; j < G; ++j)
            w[j] = table[((uint64_t)np2kc::bucket_of(h[j]) << cap_log2) + ((np2kc::key_of(h[j]) + (((pend >> j) & 1u) ? probe : 0u)) & capm)];
#pragma unroll
        for (uint32_t j = 0; j < G; ++j)
            if ((pend >> j) & 1u) {
                const bool hit = (w[j] >> np2kc::COUNT_BITS) == np2kc::key_of(h[j]);
                if (hit) cnt[j] = (uint32_t)(w[j] & np2kc::COUNT_MAX);
                if (hit || w[j] == YAK_EMPTY) pend &= ~(1u << j);
            }
    }
}

// count(k-mer) of one k-mer (np2_qv_core.hpp), one lane on its own; a table that repeats keys answers with its last
// passing word in file order (qv_get_bounded)
__device__ __forceinline__ uint32_t get_bounded(const YakDev &y, uint64_t x, uint32_t min_count) {
    if (y.ord) return qv_get_bounded(y, x, min_count);
    const uint64_t capm = (1ULL << y.cap_log2) - 1;
    const uint64_t *tb = y.table + ((uint64_t)np2kc::bucket_of(x) << y.cap_log2);
    uint64_t s = np2kc::key_of(x) & capm;
    for (uint64_t probe = 0; probe <= capm; ++probe, s = (s + 1) & capm) {
        const uint64_t w = tb[s];
        if (w == YAK_EMPTY) break;
        if ((w >> np2kc::COUNT_BITS) == np2kc::key_of(x)) return np2qv::passing((uint32_t)(w & np2kc::COUNT_MAX), min_count);
    }
    return 0u;
}

// the wavefront's sum, in lane 0
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_down((int)v, o);
    return v;
}

// the block's N counters (lanes with `mine` contribute) added to dst[0 .. N): wavefront sums, s_cnt (zero before and
// after), one atomic per non-zero counter.  Every lane of the block calls it.
template <uint32_t N, class T>
__device__ __forceinline__ void block_flush(bool mine, const uint32_t (&v)[N], uint32_t *s_cnt, T *dst) {
#pragma unroll
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t a = wave_sum(mine ? v[i] : 0u);
        if ((threadIdx.x & 63u) == 0 && a) atomicAdd(&s_cnt[i], a);
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const uint32_t c = s_cnt[threadIdx.x];
        if (c) atomicAdd(&dst[threadIdx.x], (T)c);
        s_cnt[threadIdx.x] = 0;
    }
    __syncthreads();
}

} // namespace np2
