// Launchers of the trio scan (np2_trio.hip) for its host driver (np2_trio_host.cpp).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>
#include <string>

#include "np2_qv.hpp"
#include "np2_trio_core.hpp"

namespace np2 {

// One scan of a stream laid out and masked as the QV scan's (ScanStream, np2_qv.hpp).
struct TrioScan {
    ScanStream in;
    uint32_t min_count, mid_count;
    unsigned long long *stats; // per sequence TRIO_STATS counters (added to): n_kmers, n_pat, n_mat, pp, pm, mp, mm
    uint32_t *tiles;           // n_tiles words: np2trio::tile_word of every tile (written)
    uint32_t *pat_bits;        // n_tiles * QV_BLOCK words each: a lane's 32 bitmap bits, or nullptr
    uint32_t *mat_bits;
    uint32_t *carry;           // one word: class of the last marker of the sequence that goes on in the next piece; read
                               // as what lies before tile 0 when that tile does not start a sequence, written at the end
};
// k_trio_scan: everything inside a tile.  `blocks`: the grid; blocks stride over the tiles
void launch_trio_scan(hipStream_t s, const YakDev &pat, const YakDev &mat, const TrioScan &q, uint32_t blocks);
// k_trio_join: the pairs across tile boundaries, one block over all tiles (a segmented scan of q.tiles); after the scan
void launch_trio_join(hipStream_t s, const TrioScan &q);

#if defined(__HIPCC__)
// the scan operators of np2_trio_core.hpp's carry algebra (np2_blockscan.hpp), for np2_trio.hip and np2_bin.hip
struct OpRight {
    static __device__ __forceinline__ uint32_t ident() { return 0u; }
    static __device__ __forceinline__ uint32_t apply(uint32_t a, uint32_t b) { return np2trio::right(a, b); }
};
struct OpSegRight {
    static __device__ __forceinline__ uint32_t ident() { return 0u; }
    static __device__ __forceinline__ uint32_t apply(uint32_t a, uint32_t b) { return np2trio::seg_right(a, b); }
};
#endif

} // namespace np2

struct np2_ctx;
namespace np2 {
// np2_trio_host.cpp: everything about the two tables and the thresholds, before anything is launched (NP2_E_ARG, the
// message begins with `who`)
void trio_check_tables(np2_ctx *cx, int pat_idx, int mat_idx, uint16_t min_count, uint16_t mid_count, const std::string &who);
} // namespace np2
