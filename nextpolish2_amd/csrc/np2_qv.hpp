// Launcher of the k-mer QV scan (np2_qv.hip) for its host driver (np2_qv_host.cpp).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "np2_kernels.hpp"
#include "np2_qv_core.hpp"

namespace np2 {

// The stream of one scan (QvScan, TrioScan): tiles [0, n_tiles) of a stream whose offset 0 is `src` (any alignment).  Only
// offsets in [lo, hi) are read as bases, everything else as separators; the 16-byte loads are aligned and those that
// straddle lo or hi are masked (stage_any, np2_kmerscan.hpp).  Every sequence starts at a tile boundary.
struct ScanStream {
    const uint8_t *src;
    int64_t lo, hi;
    const uint32_t *desc; // per tile: sequence index | QV_FIRST; nullptr: one sequence (index 0) starting at offset 0
    uint32_t n_tiles;
};
struct QvScan {
    ScanStream in;
    uint32_t min_count;
    unsigned long long *stats; // per sequence: n_kmers, n_absent (added to)
    unsigned long long *hist;  // QV_HIST_BINS counters (added to), or nullptr
    uint32_t *bits;            // n_tiles * QV_BLOCK words: a lane's 32 bitmap bits, or nullptr
};
// `blocks`: the grid (sized to the device by the caller); blocks stride over the tiles
void launch_qv_scan(hipStream_t s, const YakDev &y, const QvScan &q, uint32_t blocks);

#if defined(__HIPCC__)
// yak_get (np2_kernels.hpp) with its probe loops bounded by the sub-table's capacity: the lookup of a table that repeats
// keys (`ord`: the last passing word in file order wins), one k-mer at a time
__device__ __forceinline__ uint32_t qv_get_bounded(const YakDev &y, uint64_t x, uint32_t min_count) {
    const uint64_t capm = (1ULL << y.cap_log2) - 1;
    const uint64_t *tb = y.table + ((uint64_t)np2kc::bucket_of(x) << y.cap_log2);
    const uint32_t *ob = y.ord + ((uint64_t)np2kc::bucket_of(x) << y.cap_log2);
    const uint64_t key = np2kc::key_of(x);
    uint64_t s = key & capm;
    uint32_t c = 0;
    int64_t at = -1;
    for (uint64_t probe = 0; probe <= capm; ++probe, s = (s + 1) & capm) {
        const uint64_t w = tb[s];
        if (w == YAK_EMPTY) break;
        if ((w >> np2kc::COUNT_BITS) == key && (uint32_t)(w & np2kc::COUNT_MAX) >= min_count && (int64_t)ob[s] > at) at = ob[s], c = (uint32_t)(w & np2kc::COUNT_MAX);
    }
    return c;
}
#endif

} // namespace np2
