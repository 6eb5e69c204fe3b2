// Launchers of the mapping-depth kernels (np2_depth.hip) and the driver both C entry points share (np2_depth_host.cpp).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "../../include/np2_io.h"
#include "np2_depth_core.hpp"
#include "np2_lookback.hpp"

namespace np2 {

static constexpr uint32_t DEPTH_THREADS = 1024, DEPTH_ITEMS = 8;       // a thread owns 8 consecutive positions (or runs)
static constexpr uint32_t DEPTH_TILE = DEPTH_THREADS * DEPTH_ITEMS;    // of its block's 8192
static constexpr uint32_t DEPTH_MAX_L = 0xFFFF0000u;                    // position arithmetic is 32-bit up to a tile beyond L

// counters of one call, zeroed by the caller before the first launch
struct DepthDev {
    unsigned long long sum_depth, bases_kept;
    uint32_t max_depth, bases_ok, n_runs, n_kept, n_seen, n_counted;
    uint32_t err, pad; // LB_ERR: a look-back wait gave up
};
struct DepthRule {
    double min_aligned_fra;
    uint32_t min_depth, min_len, exclude_flags, min_mapq;
};

inline uint32_t depth_blocks(uint64_t n) { return (uint32_t)((n + DEPTH_TILE - 1) / DEPTH_TILE); }

// +1 / -1 of every counted record into diff (L + 1 zeroed words: word L takes the ends at or beyond the contig's end)
void launch_depth_events(hipStream_t s, const np2_bamrec_t *recs, const uint32_t *cigar, uint32_t n_recs, uint32_t L, DepthRule rule,
                         uint32_t *diff, DepthDev *ctr);
// inclusive sums of diff[0, L) in place (the depth), with sum_depth, max_depth and bases_ok; lb: depth_blocks(L) blocks
void launch_depth_scan(hipStream_t s, const Lookback &lb, uint32_t *depth, uint32_t L, uint32_t min_depth, DepthDev *ctr);
// starts[r], ends[r] of the r-th run of depth >= min_depth (room for (L + 1) / 2 each), ctr->n_runs; lb: depth_blocks(L) blocks
void launch_depth_runs(hipStream_t s, const Lookback &lb, const uint32_t *depth, uint32_t L, uint32_t min_depth, uint32_t *starts,
                       uint32_t *ends, DepthDev *ctr);
// the runs of at least min_len positions, in order, into kept_s / kept_e; ctr->n_kept, ctr->bases_kept.  The number of runs
// is read on the device (ctr->n_runs <= max_runs); lb: depth_blocks(max_runs) blocks
void launch_depth_keep(hipStream_t s, const Lookback &lb, const uint32_t *starts, const uint32_t *ends, uint32_t max_runs,
                       uint32_t min_len, uint32_t *kept_s, uint32_t *kept_e, DepthDev *ctr);

} // namespace np2

struct np2_ctx;
namespace np2h {
// opts as the C ABI takes them -> the kernels' rule; throws NP2_E_ARG (nothing is launched before it)
np2::DepthRule depth_rule(const np2_depth_opts_t *opts);
// The three steps over records and CIGAR words that are on ctx's device already; results as np2_depth_from_records returns
// them (pinned blocks, released with np2_free).
void depth_device(np2_ctx *cx, uint32_t L, const np2_bamrec_t *d_recs, uint32_t n_recs, const uint32_t *d_cigar,
                  const np2::DepthRule &rule, uint32_t **starts, uint32_t **ends, uint32_t *n_runs, uint32_t *depth_out,
                  np2_depth_stats_t *stats);
} // namespace np2h
