// Device helpers shared by the scans that probe a paternal and a maternal table (np2_trio.hip, np2_bin.hip): the scan
// operators of np2_trio_core.hpp's carry algebra and the two-table probe of a lane's group of QV_GROUP k-mers.
#pragma once
#include <hip/hip_runtime.h>

#include "np2_qv.hpp"
#include "np2_trio_core.hpp"

namespace np2 {
using namespace np2kc;
using namespace np2qv;
using namespace np2trio;

struct OpRight {
    static __device__ __forceinline__ uint32_t ident() { return 0u; }
    static __device__ __forceinline__ uint32_t apply(uint32_t a, uint32_t b) { return right(a, b); }
};
struct OpSegRight {
    static __device__ __forceinline__ uint32_t ident() { return 0u; }
    static __device__ __forceinline__ uint32_t apply(uint32_t a, uint32_t b) { return seg_right(a, b); }
};

// the stored count of one k-mer, probe loops bounded by the sub-table's capacity; a table that repeats keys answers with
// its last word in file order (qv_get_bounded)
__device__ __forceinline__ uint32_t trio_get_bounded(const YakDev &y, uint64_t x) {
    if (y.ord) return qv_get_bounded(y, x, 1u);
    const uint64_t capm = (1ULL << y.cap_log2) - 1;
    const uint64_t *tb = y.table + ((uint64_t)bucket_of(x) << y.cap_log2);
    uint64_t s = key_of(x) & capm;
    for (uint64_t probe = 0; probe <= capm; ++probe, s = (s + 1) & capm) {
        const uint64_t w = tb[s];
        if (w == YAK_EMPTY) break;
        if ((w >> COUNT_BITS) == key_of(x)) return (uint32_t)(w & COUNT_MAX);
    }
    return 0u;
}

// one table's answers from the first-slot words `w` of a lane's group: a hit gives the stored count; the k-mers whose
// slot held another key go on together, one more slot each per round, again loaded back to back (a settled k-mer loads its
// first slot again, a cache hit: unconditional loads, as in k_qv_scan, and no slot index to keep per k-mer)
__device__ __forceinline__ void trio_settle(const YakDev &y, const uint64_t (&h)[QV_GROUP], uint32_t valid, uint64_t (&w)[QV_GROUP],
                                            uint32_t (&cnt)[QV_GROUP]) {
    const uint64_t capm = (1ULL << y.cap_log2) - 1;
    uint32_t pend = 0;
#pragma unroll
    for (uint32_t j = 0; j < QV_GROUP; ++j) {
        const bool hit = (w[j] >> COUNT_BITS) == key_of(h[j]); // (EMPTY >> 10 is no key: a hash has 62 bits at most)
        cnt[j] = hit ? (uint32_t)(w[j] & COUNT_MAX) : 0u;
        pend |= (((valid >> j) & 1u) && !hit && w[j] != YAK_EMPTY ? 1u : 0u) << j;
    }
    for (uint64_t probe = 1; pend && probe <= capm; ++probe) {
#pragma unroll
        for (uint32_t j = 0; j < QV_GROUP; ++j)
            w[j] = y.table[((uint64_t)bucket_of(h[j]) << y.cap_log2) + ((key_of(h[j]) + (((pend >> j) & 1u) ? probe : 0u)) & capm)];
#pragma unroll
        for (uint32_t j = 0; j < QV_GROUP; ++j)
            if ((pend >> j) & 1u) {
                const bool hit = (w[j] >> COUNT_BITS) == key_of(h[j]);
                if (hit) cnt[j] = (uint32_t)(w[j] & COUNT_MAX);
                if (hit || w[j] == YAK_EMPTY) pend &= ~(1u << j);
            }
    }
}

} // namespace np2
