// Launchers of the repetitive k-mer kernels (np2_rep.hip) for the host driver (np2_rep_host.cpp).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace np2 {

// device counters of the selection pass (unsigned long long each)
enum : uint32_t { REP_DISTINCT = 0, REP_TOTAL = 1, REP_MAX = 2, REP_N_CTR = 4 };

static constexpr uint32_t REP_HALF = 1u << 16;               // bins of either level of the selection
static constexpr uint32_t REP_LO_LDS = 4096;                 // low-half bins a block keeps in LDS
static constexpr uint32_t REP_BLOCK = 256;                   // lanes of a selection / compaction block
static constexpr uint32_t REP_SLAB = REP_BLOCK * 4;          // counters a block reads at a time: one uint4 a lane
static constexpr uint32_t REP_CHUNK = REP_SLAB * 4;          // counters a compaction block owns
inline uint64_t rep_chunks(uint64_t table) { return (table + REP_CHUNK - 1) / REP_CHUNK; }

// `in` as launch_kcount takes it (HALO bytes, the piece's n bytes, '\n' up to a multiple of 16; 16-byte aligned); count:
// 4^k counters.  collapse: a lane adds a run of equal consecutive indices once (false: one add per k-mer, the probe's A/B).
void launch_rep_count(hipStream_t s, const uint8_t *in, uint64_t n, uint32_t k, uint32_t *count, bool collapse);
// One pass over the `table` counters (a multiple of 4).  With `first`: ctr += (counters above 0, their sum, their maximum)
// and hist_hi[c >> 16] += 1 for every counter c above 0.  Always: hist_lo[c & 65535] += 1 for those with c >> 16 == bin.
// Both histograms have REP_HALF bins and are zeroed by the caller.
void launch_rep_hist(hipStream_t s, const uint32_t *count, uint64_t table, uint32_t bin, bool first, uint32_t *hist_hi,
                     uint32_t *hist_lo, unsigned long long *ctr, uint32_t blocks);
// sizes[c] = counters above `threshold` in chunk c, rep_chunks(table) of them
void launch_rep_sizes(hipStream_t s, const uint32_t *count, uint64_t table, uint32_t threshold, uint32_t *sizes);
// off: the exclusive sums of sizes, off[rep_chunks(table)] the total; the counters above `threshold` as (index, count) at
// off[c] .. off[c + 1], in ascending index
void launch_rep_emit(hipStream_t s, const uint32_t *count, uint64_t table, uint32_t threshold, const uint32_t *off,
                     uint32_t *index, uint32_t *counts);

} // namespace np2
