// Per-lane arithmetic of the trio scan (np2_trio.hip), as plain integer arithmetic without HIP types: what makes a k-mer a
// parental marker, how a lane tallies the markers of its stretch in order, and how two neighbouring stretches are joined.
// The same text is the scan kernel's inner step and a one-lane host program (tests/tools/trio_core_test.cpp, which looks
// its hashes up by binary search in two dumps on a machine without a GPU).  Bases, k-mers and hashes are
// np2_kcount_core.hpp's; tiles, descriptors and bitmap layout are np2_qv_core.hpp's.
//
// Definitions (tables P and M of the same k; c_P, c_M = the stored counts, 0 for a k-mer a table does not hold; where a
// table repeats keys the last word in file order):
//   paternal marker = c_P >= mid_count and c_M < min_count;   maternal marker = c_M >= mid_count and c_P < min_count
//                     (1 <= min_count <= mid_count <= 1023: no k-mer is both);
//   per sequence, its markers in ascending end position e: n_pat, n_mat, and pairs[pp, pm, mp, mm] of consecutive markers
//   as (earlier, later): n_pat + n_mat - 1 pairs when there is a marker.  A non-base byte breaks k-mers, not adjacency;
//   no pair spans two sequences;
//   switch = pm + mp over all pairs; hamming = min(n_pat, n_mat) over n_pat + n_mat;
//   marker bitmaps = one per parent, laid out like the QV scan's absent bitmap: bit e = the k-mer ending at e is that
//   parent's marker.
//
// Order: a stretch of consecutive positions is summed up as Run (class of its first and of its last marker, 0 = none) and
// the pairs inside it.  Stretches a, b in this order join to Run{a.first ? a.first : b.first, right(a.last, b.last)} plus
// one pair (a.last, b.first) when both are markers; with a marker-free stretch in between, right() carries a.last over
// it.  right() is associative with identity 0, so an exclusive scan of the stretches' `last` under it gives every stretch
// the class of the marker before it, whatever the stretches are: lanes of a block, tiles of a sequence, staging pieces.
#pragma once
#include <cstdint>

#include "np2_qv_core.hpp"

namespace np2trio {

static constexpr uint32_t NONE = 0, PAT = 1, MAT = 2; // marker classes
static constexpr uint32_t TRIO_STATS = 7;             // counters per sequence: n_kmers, n_pat, n_mat, pp, pm, mp, mm
static constexpr uint32_t COUNT_LIMIT = np2kc::COUNT_MAX;

NP2_KC_HD bool thresholds_ok(uint32_t min_count, uint32_t mid_count) {
    return 1u <= min_count && min_count <= mid_count && mid_count <= COUNT_LIMIT;
}

NP2_KC_HD uint32_t classify(uint32_t c_pat, uint32_t c_mat, uint32_t min_count, uint32_t mid_count) {
    if (c_pat >= mid_count && c_mat < min_count) return PAT;
    if (c_mat >= mid_count && c_pat < min_count) return MAT;
    return NONE;
}

// rightmost non-zero: the class of the last marker of two stretches in this order
NP2_KC_HD uint32_t right(uint32_t a, uint32_t b) { return b ? b : a; }

struct Tally {
    uint32_t n_kmers = 0, n_pat = 0, n_mat = 0, pp = 0, pm = 0, mp = 0, mm = 0;
};
struct Run {
    uint32_t first = NONE, last = NONE;
};

// the pair (earlier, later); nothing when either is no marker
NP2_KC_HD void add_pair(Tally &t, uint32_t earlier, uint32_t later) {
    t.pp += (earlier == PAT && later == PAT) ? 1u : 0u;
    t.pm += (earlier == PAT && later == MAT) ? 1u : 0u;
    t.mp += (earlier == MAT && later == PAT) ? 1u : 0u;
    t.mm += (earlier == MAT && later == MAT) ? 1u : 0u;
}
// index of (earlier, later) in pairs[pp, pm, mp, mm]; both are markers
NP2_KC_HD uint32_t pair_index(uint32_t earlier, uint32_t later) { return 2u * (earlier - 1u) + (later - 1u); }

// one base of a lane's stretch, in ascending order: `valid` = a k-mer ends here, `cls` = its class; j = the base's place
// in its bitmap byte
NP2_KC_HD void step(bool valid, uint32_t cls, uint32_t j, Tally &t, Run &r, uint32_t &pat_bits, uint32_t &mat_bits) {
    if (!valid) cls = NONE;
    t.n_kmers += valid ? 1u : 0u;
    t.n_pat += cls == PAT ? 1u : 0u;
    t.n_mat += cls == MAT ? 1u : 0u;
    pat_bits |= (cls == PAT ? 1u : 0u) << j;
    mat_bits |= (cls == MAT ? 1u : 0u) << j;
    add_pair(t, r.last, cls);
    r.first = r.first ? r.first : cls;
    r.last = right(r.last, cls);
}

// a stretch that follows a marker of class `before` (0: none): the pair across its front edge
NP2_KC_HD void join(Tally &t, uint32_t before, const Run &r) { add_pair(t, before, r.first); }

// Tile summaries (one word per tile, written by the scan, read by the join over a sequence's tiles) and the elements of
// that join's SEGMENTED scan: bits 0-1 a class, TILE_RESET = this tile starts a sequence, nothing before it counts.
static constexpr uint32_t TILE_RESET = 4u;
NP2_KC_HD uint32_t tile_word(const Run &r) { return r.first | r.last << 2; }
NP2_KC_HD uint32_t tile_first(uint32_t w) { return w & 3u; }
NP2_KC_HD uint32_t tile_last(uint32_t w) { return (w >> 2) & 3u; }
NP2_KC_HD uint32_t seg_right(uint32_t a, uint32_t b) { // associative, identity 0
    if (b & TILE_RESET) return b;
    return (a & TILE_RESET) | right(a & 3u, b & 3u);
}

} // namespace np2trio
