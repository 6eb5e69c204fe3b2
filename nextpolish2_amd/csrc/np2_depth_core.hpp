// Per-record arithmetic of the mapping-depth report (np2_depth.hip), as plain arithmetic without HIP types: what a CIGAR
// measures, which records are counted, and which runs are kept.  The same text is the event kernel's lane code, the host
// side's argument check and a stand-alone host program (tests/tools/depth_core_test.cpp).
//
// Definitions (one alignment record, CIGAR operations (op, len) in BAM encoding: len << 4 | op, ops MIDNSHP=X = 0..8):
//   span      sum of len over M D N = X: reference bases the record covers; a counted record whose sum is 0 covers 1
//   aligned   sum of len over M I = X: query bases inside the alignment (soft clips excluded)
//   read_len  sum of len over M I S H = X: the read as sequenced (hard clips count)
//   counted   (flag & exclude_flags) == 0, mapq >= min_mapq, n_cigar > 0, read_len > 0 and
//             not (double)aligned / (double)read_len < min_aligned_fra
//   depth[i]  counted records with pos <= i < min(pos + span, L); records with pos < 0 or pos >= L are ignored
//   run       a maximal [s, e] (inclusive) with depth >= min_depth throughout; kept iff e - s + 1 >= min_len
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NP2_DEPTH_HD __host__ __device__ __forceinline__
#else
#define NP2_DEPTH_HD inline
#endif

namespace np2depth {

static constexpr uint32_t DEFAULT_MIN_DEPTH = 3, DEFAULT_MIN_LEN = 1000;
static constexpr uint16_t DEFAULT_EXCLUDE_FLAGS = 0x4;

// the three sums of a CIGAR, or of a part of one (64-bit: 65 535 operations of 2^28 - 1 bases each fit)
struct Measure {
    uint64_t span = 0, aligned = 0, read_len = 0;
};
// bit `op` set: the operation counts in that sum (ops above 8 count in none)
static constexpr uint32_t OPS_SPAN = 1u << 0 | 1u << 2 | 1u << 3 | 1u << 7 | 1u << 8;                // M D N = X
static constexpr uint32_t OPS_ALIGNED = 1u << 0 | 1u << 1 | 1u << 7 | 1u << 8;                       // M I = X
static constexpr uint32_t OPS_READ = 1u << 0 | 1u << 1 | 1u << 4 | 1u << 5 | 1u << 7 | 1u << 8;      // M I S H = X

NP2_DEPTH_HD void add_op(Measure &m, uint32_t word) {
    const uint32_t op = word & 15u;
    const uint64_t len = word >> 4;
    m.span += ((OPS_SPAN >> op) & 1u) ? len : 0;
    m.aligned += ((OPS_ALIGNED >> op) & 1u) ? len : 0;
    m.read_len += ((OPS_READ >> op) & 1u) ? len : 0;
}
NP2_DEPTH_HD void add(Measure &a, const Measure &b) { a.span += b.span, a.aligned += b.aligned, a.read_len += b.read_len; }

// the aligned fraction is too small: IEEE double division and comparison, the one place where it is evaluated
NP2_DEPTH_HD bool fra_below(uint64_t aligned, uint64_t read_len, double min_aligned_fra) {
    return (double)aligned / (double)read_len < min_aligned_fra;
}
// min_aligned_fra is a number in [0, 1] (a NaN fails both comparisons)
NP2_DEPTH_HD bool fra_ok(double min_aligned_fra) { return min_aligned_fra >= 0.0 && min_aligned_fra <= 1.0; }

NP2_DEPTH_HD bool counted(uint32_t flag, uint32_t mapq, uint32_t n_cigar, const Measure &m, uint32_t exclude_flags, uint32_t min_mapq,
                          double min_aligned_fra) {
    if ((flag & exclude_flags) != 0 || mapq < min_mapq) return false;
    if (n_cigar == 0 || m.read_len == 0) return false;
    return !fra_below(m.aligned, m.read_len, min_aligned_fra);
}
// the half-open interval [lo, hi) of a counted record inside a contig of L positions; false: it covers nothing of it
NP2_DEPTH_HD bool cover(int32_t pos, uint64_t span, uint32_t L, uint32_t &lo, uint32_t &hi) {
    if (pos < 0 || (uint32_t)pos >= L) return false;
    const uint64_t end = (uint64_t)(uint32_t)pos + (span ? span : 1u);
    lo = (uint32_t)pos;
    hi = end < (uint64_t)L ? (uint32_t)end : L;
    return true;
}

NP2_DEPTH_HD bool depth_ok(uint32_t depth, uint32_t min_depth) { return depth >= min_depth; }
NP2_DEPTH_HD bool run_kept(uint32_t s, uint32_t e, uint32_t min_len) { return (uint64_t)e - s + 1 >= (uint64_t)min_len; }

} // namespace np2depth
