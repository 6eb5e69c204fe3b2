// Launcher of the k-mer QV scan (np2_qv.hip) for its host driver (np2_qv_host.cpp).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "np2_kernels.hpp"
#include "np2_qv_core.hpp"

namespace np2 {

// One scan: tiles [0, n_tiles) of a stream whose offset 0 is `src` (any alignment).  Only offsets in [lo, hi) are read as
// bases, everything else as separators; the 16-byte loads are aligned and those that straddle lo or hi are masked.
struct QvScan {
    const uint8_t *src;
    int64_t lo, hi;
    const uint32_t *desc;      // per tile: sequence index | QV_FIRST; nullptr: one sequence (index 0) starting at offset 0
    uint32_t n_tiles;
    uint32_t min_count;
    unsigned long long *stats; // per sequence: n_kmers, n_absent (added to)
    unsigned long long *hist;  // QV_HIST_BINS counters (added to), or nullptr
    uint32_t *bits;            // n_tiles * QV_BLOCK words: a lane's 32 bitmap bits, or nullptr
};
// `blocks`: the grid (sized to the device by the caller); blocks stride over the tiles
void launch_qv_scan(hipStream_t s, const YakDev &y, const QvScan &q, uint32_t blocks);

} // namespace np2
