// Trio scan: an assembly's bytes against a paternal and a maternal k-mer table -> per sequence the number of k-mers, of
// paternal and of maternal markers, the four kinds of consecutive marker pairs (switch error = pm + mp over all pairs,
// Hamming error = min(n_pat, n_mat) over all markers) and one bitmap per parent of where the markers end.  Read-only on
// the tables (YakDev).  Definitions and the per-lane arithmetic are np2_trio_core.hpp's (also a one-lane host program).
//
// Input: k_qv_scan's (np2_qv.hip; the staging contract of np2_kmerscan.hpp): stage_any, every sequence from a tile
// boundary, a lane owns the k-mers that END in its 32 bytes.
//
// Probes (the probe contract of np2_kmerscan.hpp): a lane hashes QV_GROUP k-mers and issues their first-slot loads of BOTH
// tables, sixteen independent 8-byte reads, back to back before it looks at any word; then one table after the other
// settles its collisions.
//
// Order: pairs are a relation between consecutive markers, across lanes, wavefronts, tiles, blocks of the grid and staging
// pieces.  Every level sums a stretch up as (first, last, pairs inside) and joins neighbours under np2trio::right
// (rightmost non-zero, associative), so that every counter stays a sum of integers:
//   lane   its 32 positions in order (np2trio::step);
//   block  an exclusive scan of the lanes' `last` under right() (DPP wave scan + 4 wave totals through LDS) gives a lane
//          the class of the marker before its stretch: one pair more; the tile's (first, last) goes to q.tiles[t];
//   tiles  k_trio_join, one block: a segmented exclusive scan of the tiles' `last` (segments = sequences) gives a tile the
//          class of the last marker before it, however many marker-free tiles lie between: one pair more per tile;
//   pieces the join starts from q.carry and leaves there what the piece ends with.
// Which block scans which tile, and where a piece ends, changes no sum.
#include <hip/hip_runtime.h>

#include "np2_blockscan.hpp"
#include "np2_kmerscan.hpp"
#include "np2_trio.hpp"

namespace np2 {
using namespace np2kc;
using namespace np2qv;
using namespace np2trio;

namespace {

static constexpr uint32_t TRIO_CHUNKS = (HALO + QV_TILE) / 16 + 1; // 16-byte pieces of a tile's window (+ 1: a source that is not 16-byte aligned)
static constexpr uint32_t TRIO_WAVES = QV_BLOCK / 64;

} // namespace

__global__ __launch_bounds__(QV_BLOCK) void k_trio_scan(YakDev yp, YakDev ym, TrioScan q) {
    __shared__ uint4 tile[TRIO_CHUNKS];
    __shared__ uint32_t s_cnt[TRIO_STATS];
    __shared__ uint32_t s_scan[TRIO_WAVES];
    __shared__ uint32_t s_first;
    const uint32_t tid = threadIdx.x;
    if (tid < TRIO_STATS) s_cnt[tid] = 0;
    if (tid == 0) s_first = NONE;
    __syncthreads();

    const uint32_t k = yp.k; // (== ym.k: the host driver refuses anything else)
    const uint64_t mask = kmer_mask(k);
    const auto dword = lane_dwords<QV_STRETCH>(tile, q.in.src);
    const bool whole_cluster = yp.ord || ym.ord; // a table that repeats keys (yak writes none)
    uint32_t cur = ~0u;
    Tally tally;
    auto flush = [&] { // the block's counters of sequence `cur` -> global memory
        const uint32_t v[TRIO_STATS] = {tally.n_kmers, tally.n_pat, tally.n_mat, tally.pp, tally.pm, tally.mp, tally.mm};
        block_flush<TRIO_STATS>(true, v, s_cnt, q.stats + TRIO_STATS * (uint64_t)cur);
        tally = Tally{};
    };

    for (uint32_t t = blockIdx.x; t < q.in.n_tiles; t += gridDim.x) {
        const uint32_t d = q.in.desc ? q.in.desc[t] : 0u;
        const uint32_t seq = d & ~QV_FIRST;
        if (seq != cur) { // (the same for every lane of the block: a tile belongs to one sequence)
            if (cur != ~0u) flush();
            cur = seq;
        }
        stage_any<QV_BLOCK, TRIO_CHUNKS>(tile, q.in, (int64_t)t * QV_TILE, (d & QV_FIRST) != 0u);
        __syncthreads();

        Roll r;
        warm_halo(r, dword, k, mask);
        uint32_t lane_pat = 0, lane_mat = 0;
        Run run;
#pragma unroll 1
        for (uint32_t g = 0; g < QV_STRETCH / QV_GROUP; ++g) {
            const uint32_t wa = dword(HALO / 4 + 2 * g), wb = dword(HALO / 4 + 2 * g + 1);
            uint64_t h[QV_GROUP];
            uint32_t cp[QV_GROUP], cm[QV_GROUP];
            const uint32_t valid = hash_group(r, wa, wb, k, mask, h);
            if (whole_cluster) {
#pragma unroll
                for (uint32_t j = 0; j < QV_GROUP; ++j) {
                    cp[j] = cm[j] = 0;
                    if ((valid >> j) & 1u) cp[j] = get_bounded(yp, h[j], 1u), cm[j] = get_bounded(ym, h[j], 1u);
                }
            } else {
                // round 0 of both tables: sixteen first-slot loads are issued before any word is looked at (the scheduling
                // barrier keeps the compiler from sinking a word's use between the loads)
                uint64_t wp[QV_GROUP], wm[QV_GROUP];
                probe_issue(yp.table, yp.cap_log2, h, wp);
                probe_issue(ym.table, ym.cap_log2, h, wm);
                __builtin_amdgcn_sched_barrier(0);
                probe_settle(yp.table, yp.cap_log2, h, valid, wp, cp);
                probe_settle(ym.table, ym.cap_log2, h, valid, wm, cm);
            }
            uint32_t pat_byte = 0, mat_byte = 0;
#pragma unroll
            for (uint32_t j = 0; j < QV_GROUP; ++j)
                step((valid >> j) & 1u, classify(cp[j], cm[j], q.min_count, q.mid_count), j, tally, run, pat_byte, mat_byte);
            lane_pat |= pat_byte << (8 * g);
            lane_mat |= mat_byte << (8 * g);
        }
        if (q.pat_bits) q.pat_bits[(uint64_t)t * QV_BLOCK + tid] = lane_pat;
        if (q.mat_bits) q.mat_bits[(uint64_t)t * QV_BLOCK + tid] = lane_mat;

        // the marker before this lane's stretch inside the tile, and the tile's own (first, last)
        uint32_t tile_last_cls;
        const uint32_t before = block_excl_scan<OpRight, TRIO_WAVES>(run.last, s_scan, tile_last_cls);
        join(tally, before, run);
        if (run.first && !before) s_first = run.first; // (one lane at most: the one that holds the tile's first marker)
        __syncthreads(); // (and the next tile overwrites the window)
        if (tid == 0) {
            q.tiles[t] = tile_word(Run{s_first, tile_last_cls});
            s_first = NONE;
        }
    }
    if (cur != ~0u) flush();
}

// The pairs across tile boundaries.  Element of tile t: its last marker's class, with TILE_RESET where t starts a sequence;
// the exclusive prefix under seg_right, started from the carry of the piece before, is the class of the last marker of
// the same sequence before tile t (0: none).  One block scans all tiles (block_scan_array: loads of 32 K tiles in flight,
// then the block-wide scans), so a marker-free stretch of any number of tiles costs nothing extra.
__global__ __launch_bounds__(BS_THREADS) void k_trio_join(TrioScan q) {
    __shared__ uint32_t sh[16];
    const uint32_t carry_in = *q.carry & 3u;
    __syncthreads(); // (the carry is read by everyone before thread 0 writes it)
    auto first_of_seq = [&](uint32_t t) { return q.in.desc ? (q.in.desc[t] & QV_FIRST) != 0u : false; };
    const uint32_t total = block_scan_array<OpSegRight>(
        q.in.n_tiles, sh, [&](uint32_t t) { return tile_last(q.tiles[t]) | (first_of_seq(t) ? TILE_RESET : 0u); },
        [&](uint32_t t, uint32_t prefix, uint32_t) {
            if (first_of_seq(t)) return;
            const uint32_t before = seg_right(carry_in, prefix) & 3u, first = tile_first(q.tiles[t]);
            if (before && first) {
                const uint32_t seq = q.in.desc ? q.in.desc[t] & ~QV_FIRST : 0u;
                atomicAdd(&q.stats[TRIO_STATS * (uint64_t)seq + 3u + pair_index(before, first)], 1ull);
            }
        });
    if (threadIdx.x == 0) *q.carry = seg_right(carry_in, total) & 3u;
}

void launch_trio_scan(hipStream_t s, const YakDev &pat, const YakDev &mat, const TrioScan &q, uint32_t blocks) {
    if (q.in.n_tiles == 0) return;
    hipLaunchKernelGGL(k_trio_scan, dim3(blocks < q.in.n_tiles ? (blocks ? blocks : 1u) : q.in.n_tiles), dim3(QV_BLOCK), 0, s, pat, mat, q);
}

void launch_trio_join(hipStream_t s, const TrioScan &q) {
    if (q.in.n_tiles == 0) return;
    hipLaunchKernelGGL(k_trio_join, dim3(1), dim3(BS_THREADS), 0, s, q);
}

} // namespace np2
