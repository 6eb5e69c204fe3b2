// Launchers of the read binner (np2_bin.hip) for its host driver (np2_bin_host.cpp).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "np2_bin_core.hpp"
#include "np2_kernels.hpp"

namespace np2 {

// One piece of a packed separator stream: offset 0 is `src` (16-byte aligned, HALO readable bytes in front of it: the
// stream's own bytes, separators in front of the first piece), offsets [0, n_bytes) are the piece.  Reads lie back to
// back, each followed by one '\n'; `ends` are the offsets of those separators in the piece, ascending.  The reads of the
// piece are numbered from 0: read r ends at ends[r], read n_ends is the one that goes on in the next piece.
struct BinScan {
    const uint8_t *src;
    uint32_t n_bytes, n_tiles; // n_tiles = tiles_of(n_bytes); the buffer holds whole tiles
    const uint32_t *ends;
    uint32_t n_ends;
    uint32_t min_count, mid_count, min_score, minor_permille;
    uint32_t *owner;           // n_tiles words (written by the owner kernel): the read that owns the tile's first byte
    uint32_t *tiles;           // n_tiles words (written by the scan): np2bin::tile_word of every tile
    uint32_t *tallies;         // (n_ends + 1) * BIN_STATS counters, zero before the scan: n_kmers, n_pat, n_mat, pp, pm, mp, mm
    uint32_t *carry;           // one word: class of the last marker of the read that goes on in the next piece (read, written)
    const uint32_t *tally_in;  // BIN_STATS counters: what the pieces before hold of read 0 (zero when it starts here)
    uint32_t *tally_out;       // BIN_STATS counters: what the pieces so far hold of read n_ends (written; != tally_in)
    uint8_t *cls;              // n_ends class bytes (written)
};
// owner -> scan -> join -> classify on one stream.  `blocks`: the scan's grid; blocks stride over the tiles
void launch_bin_piece(hipStream_t s, const YakDev &pat, const YakDev &mat, const BinScan &q, uint32_t blocks);

} // namespace np2
