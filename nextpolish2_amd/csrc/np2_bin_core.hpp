// Per-lane arithmetic of the read binner (np2_bin.hip), as plain integer arithmetic without HIP types: how a stretch of a
// PACKED separator stream (reads back to back, one '\n' after each) is walked when it may hold any number of read
// boundaries, how the pieces of one read are joined, and what class a read's tallies give it.  The same text is the scan
// kernel's inner step and a one-lane host program (tests/tools/bin_core_test.cpp).  Markers, Tally, Run and the carry
// algebra (right, seg_right) are np2_trio_core.hpp's, unchanged.
//
// Definitions (tables P and M of the same k, thresholds as np2trio::classify):
//   per read   (n_kmers, n_pat, n_mat, pairs[pp, pm, mp, mm]): what np2_trio_strings returns for the read as a sequence
//              of its own;
//   scores     s_pat = pp, s_mat = mm: a marker counts when it directly follows a marker of the same parent, an isolated
//              marker scores nothing;
//   class      '0' when s_pat < min_score and s_mat < min_score; otherwise with L = max, S = min of the two scores 'a'
//              (ambiguous) when s_pat == s_mat or S * 1000 > L * minor_permille; otherwise 'p' or 'm', the larger score;
//   bins       paternal = p, a, 0; maternal = m, a, 0 (`yak triobin`'s recipe; the semantics are this project's own, yak's
//              report is not reproduced byte for byte).
//
// Order: a stretch with B boundaries is B + 1 segments.  The first belongs to the read that is open where the stretch
// begins (`head`), the last to the read that is open where it ends (`tail`), the B - 1 between them are whole reads.  Only
// head and tail have neighbours: stretches are joined by a SEGMENTED exclusive scan under np2trio::seg_right whose element
// is seg_word(): the class of the tail's last marker, with TILE_RESET when the stretch holds a boundary ("a read starts in
// this stretch").  The prefix & 3 is then the class of the last marker of the head's read before the stretch.
#pragma once
#include <cstdint>

#include "np2_trio_core.hpp"

namespace np2bin {

using np2trio::Run;
using np2trio::Tally;

static constexpr uint8_t SEP = (uint8_t)'\n';
static constexpr uint32_t BIN_STATS = np2trio::TRIO_STATS; // counters per read, uint32 each
static constexpr uint64_t MAX_READ = 0xFFFFFFFEull;        // a read of 2^32 - 1 bytes or more is refused: uint32 counters
static constexpr uint32_t PERMILLE = 1000;
static constexpr uint32_t DEFAULT_MIN_SCORE = 2, DEFAULT_MINOR_PERMILLE = 330;

NP2_KC_HD bool opts_ok(uint32_t minor_permille) { return minor_permille <= PERMILLE; }

// the class byte of one read from its scores; 64-bit integer arithmetic only
NP2_KC_HD uint8_t read_class(uint32_t s_pat, uint32_t s_mat, uint32_t min_score, uint32_t minor_permille) {
    if (s_pat < min_score && s_mat < min_score) return (uint8_t)'0';
    const uint64_t L = s_pat > s_mat ? s_pat : s_mat, S = s_pat > s_mat ? s_mat : s_pat;
    if (s_pat == s_mat || S * (uint64_t)PERMILLE > L * (uint64_t)minor_permille) return (uint8_t)'a';
    return s_pat > s_mat ? (uint8_t)'p' : (uint8_t)'m';
}
NP2_KC_HD uint8_t class_of(const Tally &t, uint32_t min_score, uint32_t minor_permille) {
    return read_class(t.pp, t.mm, min_score, minor_permille);
}
NP2_KC_HD bool keep_pat(uint8_t cls) { return cls != (uint8_t)'m'; }
NP2_KC_HD bool keep_mat(uint8_t cls) { return cls != (uint8_t)'p'; }

NP2_KC_HD void add(Tally &a, const Tally &b) {
    a.n_kmers += b.n_kmers, a.n_pat += b.n_pat, a.n_mat += b.n_mat;
    a.pp += b.pp, a.pm += b.pm, a.mp += b.mp, a.mm += b.mm;
}

// dst = src where `c` holds, field by field (plain selects: nothing here is addressed through a pointer chosen at run time)
NP2_KC_HD void put_if(Tally &dst, bool c, const Tally &src) {
    dst.n_kmers = c ? src.n_kmers : dst.n_kmers, dst.n_pat = c ? src.n_pat : dst.n_pat, dst.n_mat = c ? src.n_mat : dst.n_mat;
    dst.pp = c ? src.pp : dst.pp, dst.pm = c ? src.pm : dst.pm, dst.mp = c ? src.mp : dst.mp, dst.mm = c ? src.mm : dst.mm;
}
NP2_KC_HD void put_if(Run &dst, bool c, const Run &src) {
    dst.first = c ? src.first : dst.first, dst.last = c ? src.last : dst.last;
}

// What a walk leaves of its stretch.  With n_bounds == 0 the whole stretch is `head` (and `tail` is empty); whole reads
// between the first and the last boundary are handed to the walk's `closed` callback and leave nothing here.
struct Stretch {
    Tally head, tail;
    Run head_run, tail_run;
    uint32_t n_bounds = 0;
};

// One byte of a stretch, in ascending order: `valid` / `cls` as np2trio::step, `boundary` = this byte is the separator that
// ends a read (a separator is no base: valid is false there).  closed(i, tally): the i-th read (counted from the stretch's
// head = 0) that lies wholly inside the stretch, i >= 1.
template <class Closed>
NP2_KC_HD void walk(Stretch &s, Tally &t, Run &r, bool valid, uint32_t cls, bool boundary, Closed &&closed) {
    uint32_t pb = 0, mb = 0; // (no bitmaps here)
    np2trio::step(valid, cls, 0, t, r, pb, mb);
    if (boundary) {
        const bool first = s.n_bounds == 0;
        put_if(s.head, first, t), put_if(s.head_run, first, r);
        if (!first) closed(s.n_bounds, t);
        ++s.n_bounds;
        t = Tally{};
        r = Run{};
    }
}
// after the last byte
NP2_KC_HD void walk_end(Stretch &s, const Tally &t, const Run &r) {
    const bool none = s.n_bounds == 0;
    put_if(s.head, none, t), put_if(s.head_run, none, r);
    put_if(s.tail, !none, t), put_if(s.tail_run, !none, r);
}

// the stretch's element of the segmented scan
NP2_KC_HD uint32_t seg_word(const Stretch &s) {
    return s.n_bounds ? (s.tail_run.last | np2trio::TILE_RESET) : s.head_run.last;
}
// the head joined to what the scan found before the stretch
NP2_KC_HD void join_head(Stretch &s, uint32_t prefix) { np2trio::join(s.head, prefix & 3u, s.head_run); }

// Tile summaries (one word per tile, written by the scan, read by the join): bits 0-1 the class of the first marker before
// the tile's first boundary, bits 2-3 the class of the last marker after its last boundary, TILE_HAS_BOUND when the tile
// holds a boundary.  The join's scan element is tile_elem(): np2trio's `last` with TILE_RESET.
static constexpr uint32_t TILE_HAS_BOUND = 1u << 4;
NP2_KC_HD uint32_t tile_word(uint32_t first, uint32_t scan_total) {
    return first | (scan_total & 3u) << 2 | ((scan_total & np2trio::TILE_RESET) ? TILE_HAS_BOUND : 0u);
}
NP2_KC_HD uint32_t tile_elem(uint32_t w) { return np2trio::tile_last(w) | ((w & TILE_HAS_BOUND) ? np2trio::TILE_RESET : 0u); }

} // namespace np2bin
