// Per-lane arithmetic and layouts of the k-mer QV scan (np2_qv.hip), as plain integer arithmetic without HIP types: what a
// count means once the threshold is applied, how one base's k-mer is tallied, and where a sequence's tiles and bitmap
// bytes lie.  The same text is the scan kernel's inner step and a one-lane host program (tests/tools/qv_core_test.cpp,
// which looks its hashes up by binary search in a dump's buckets on a machine without a GPU).  Bases, k-mers and hashes
// are np2_kcount_core.hpp's.
//
// Definitions:
//   count(k-mer)  = KmerInfo::get after retrieve_kmers(min_count): the stored count if it is >= min_count, else 0
//                   (min_count 0 and 1 both mean "present at all": a stored count is never 0);
//   absent        = count == 0;
//   histogram     = hist[c]: k-mers (with multiplicity) whose count is c, c in [0, 1023];
//   absent bitmap = per sequence, least significant bit first: bit e is set exactly when the k-mer ENDING at base e (bases
//                   e - k + 1 .. e) is valid and absent; sequence i starts at byte sum over j < i of ceil(len_j / 8).
//
// Staging layout of the scan: every sequence starts at a tile boundary of the stream and is padded with '\n' to the next
// one, so that a tile belongs to one sequence (an empty sequence has no tile).  A tile's descriptor is its sequence's
// index in the piece, with QV_FIRST set on the sequence's first tile: the bytes in front of such a tile belong to another
// sequence and are read as separators.
#pragma once
#include <cstdint>

#include "np2_kcount_core.hpp"

namespace np2qv {

static constexpr uint32_t QV_BLOCK = 256;                  // lanes of a block
static constexpr uint32_t QV_STRETCH = 32;                 // bytes a lane owns
static constexpr uint32_t QV_GROUP = 8;                    // k-mers a lane has in flight: one bitmap byte
static constexpr uint32_t QV_TILE = QV_BLOCK * QV_STRETCH; // bytes a block brings into LDS per turn
static constexpr uint32_t QV_TILE_BITS = QV_TILE / 8;      // bitmap bytes of a tile
static constexpr uint32_t QV_HIST_BINS = np2kc::COUNT_MAX + 1;
static constexpr uint32_t QV_FIRST = 1u << 31;             // descriptor flag: first tile of its sequence
static constexpr uint8_t QV_PAD = (uint8_t)'\n';

NP2_KC_HD uint64_t tiles_of(uint64_t len) { return (len + QV_TILE - 1) / QV_TILE; }
NP2_KC_HD uint64_t bits_bytes(uint64_t len) { return (len + 7) / 8; }

// the stored count of a found word -> count(k-mer)
NP2_KC_HD uint32_t passing(uint32_t stored, uint32_t min_count) { return stored >= min_count ? stored : 0u; }

// one base of a lane's group: `valid` = a k-mer ends here, `count` = count(k-mer); j = the base's place in its bitmap byte
NP2_KC_HD void tally(bool valid, uint32_t count, uint32_t j, uint32_t &n_kmers, uint32_t &n_absent, uint32_t &bits) {
    const bool miss = valid && count == 0u;
    n_kmers += valid ? 1u : 0u;
    n_absent += miss ? 1u : 0u;
    bits |= (miss ? 1u : 0u) << j;
}

} // namespace np2qv
