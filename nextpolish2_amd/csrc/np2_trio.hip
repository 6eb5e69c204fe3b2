// Trio scan: an assembly's bytes against a paternal and a maternal k-mer table -> per sequence the number of k-mers, of
// paternal and of maternal markers, the four kinds of consecutive marker pairs (switch error = pm + mp over all pairs,
// Hamming error = min(n_pat, n_mat) over all markers) and one bitmap per parent of where the markers end.  Read-only on
// the tables (YakDev).  Definitions and the per-lane arithmetic are np2_trio_core.hpp's (also a one-lane host program).
//
// Input: k_qv_scan's staging contract to the letter (np2_qv.hip): HALO + QV_TILE bytes through LDS with aligned 16-byte
// loads, a source of any alignment, [lo, hi) masking, every sequence from a tile boundary, a lane owns the k-mers that END
// in its 32 bytes.
//
// Probes: a lane hashes QV_GROUP k-mers and issues their first-slot loads of BOTH tables, sixteen independent 8-byte
// reads, back to back before it looks at any word; per table the k-mers whose first slot held another key then go on
// together, one more slot each per round.  Every probe loop is bounded by the sub-table's capacity.
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
#include "np2_qv.hpp"
#include "np2_trio.hpp"
#include "np2_trio_probe.hpp"

namespace np2 {
using namespace np2kc;
using namespace np2qv;
using namespace np2trio;

namespace {

static constexpr uint32_t TRIO_CHUNKS = (HALO + QV_TILE) / 16 + 1; // 16-byte pieces of a tile's window (+ 1: a source that is not 16-byte aligned)
static constexpr uint32_t PAD4 = 0x0A0A0A0Au;
static constexpr uint32_t TRIO_WAVES = QV_BLOCK / 64;

// the block's counters of sequence `seq` -> global memory: wavefront sums, LDS, one atomic per non-zero counter
__device__ __forceinline__ void trio_flush(Tally &t, uint32_t *s_cnt, unsigned long long *stats, uint32_t seq) {
    uint32_t v[TRIO_STATS] = {t.n_kmers, t.n_pat, t.n_mat, t.pp, t.pm, t.mp, t.mm};
#pragma unroll
    for (uint32_t i = 0; i < TRIO_STATS; ++i) {
        for (int o = 32; o > 0; o >>= 1) v[i] += (uint32_t)__shfl_down((int)v[i], o);
        if ((threadIdx.x & 63u) == 0 && v[i]) atomicAdd(&s_cnt[i], v[i]);
    }
    __syncthreads();
    if (threadIdx.x < TRIO_STATS) {
        const uint32_t c = s_cnt[threadIdx.x];
        if (c) atomicAdd(&stats[TRIO_STATS * (uint64_t)seq + threadIdx.x], (unsigned long long)c);
        s_cnt[threadIdx.x] = 0;
    }
    __syncthreads();
    t = Tally{};
}

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
    const uint64_t capm_p = (1ULL << yp.cap_log2) - 1, capm_m = (1ULL << ym.cap_log2) - 1;
    // the source's misalignment is the same for every tile (HALO and QV_TILE are multiples of 16): the window in LDS starts
    // `shift` bytes early and a lane reads its dwords across two LDS words
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(q.src) & 15u);
    const uint32_t *lds = reinterpret_cast<const uint32_t *>(tile) + tid * (QV_STRETCH / 4) + (shift >> 2);
    const uint32_t bsh = (shift & 3u) * 8u;
    const bool whole_cluster = yp.ord || ym.ord; // a table that repeats keys (yak writes none)
    uint32_t cur = ~0u;
    Tally tally;

    for (uint32_t t = blockIdx.x; t < q.n_tiles; t += gridDim.x) {
        const uint32_t d = q.desc ? q.desc[t] : 0u;
        const uint32_t seq = d & ~QV_FIRST;
        if (seq != cur) { // (the same for every lane of the block: a tile belongs to one sequence)
            if (cur != ~0u) trio_flush(tally, s_cnt, q.stats, cur);
            cur = seq;
        }
        const int64_t t0 = (int64_t)t * QV_TILE;
        const int64_t lo = (d & QV_FIRST) && t0 > q.lo ? t0 : q.lo;
        const int64_t w0 = t0 - (int64_t)HALO - (int64_t)shift; // stream offset of the window's first (aligned) 16 bytes
        for (uint32_t i = tid; i < TRIO_CHUNKS; i += QV_BLOCK) {
            const int64_t c0 = w0 + 16 * (int64_t)i;
            uint32_t w[4] = {PAD4, PAD4, PAD4, PAD4};
            if (c0 + 16 > lo && c0 < q.hi) { // holds a byte that may be read: the aligned 16 bytes around it are mapped
                const uint4 v = *reinterpret_cast<const uint4 *>(q.src + c0);
                w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
                if (c0 < lo || c0 + 16 > q.hi) { // the first / last load of a sequence: what lies outside is a separator
#pragma unroll
                    for (uint32_t b = 0; b < 16; ++b)
                        if (c0 + (int64_t)b < lo || c0 + (int64_t)b >= q.hi)
                            w[b >> 2] = (w[b >> 2] & ~(0xFFu << (8 * (b & 3)))) | ((uint32_t)QV_PAD << (8 * (b & 3)));
                }
            }
            tile[i] = make_uint4(w[0], w[1], w[2], w[3]);
        }
        __syncthreads();

        auto dword = [&](uint32_t i) { return (uint32_t)((((uint64_t)lds[i + 1] << 32) | lds[i]) >> bsh); };
        Roll r;
        uint64_t hh = 0;
#pragma unroll 1
        for (uint32_t i = 0; i < HALO / 4; ++i) {
            const uint32_t w = dword(i);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) (void)push(r, (uint8_t)(w >> (8 * j)), k, mask, &hh);
        }
        uint32_t lane_pat = 0, lane_mat = 0;
        Run run;
#pragma unroll 1
        for (uint32_t g = 0; g < QV_STRETCH / QV_GROUP; ++g) {
            const uint32_t wa = dword(HALO / 4 + 2 * g), wb = dword(HALO / 4 + 2 * g + 1);
            uint64_t h[QV_GROUP];
            uint32_t cp[QV_GROUP], cm[QV_GROUP];
            uint32_t valid = 0;
#pragma unroll
            for (uint32_t j = 0; j < QV_GROUP; ++j) {
                h[j] = 0; // (a base no k-mer ends at probes slot 0 of sub-table 0: a valid address, its word is ignored)
                const bool ok = push(r, (uint8_t)((j < 4 ? wa : wb) >> (8 * (j & 3))), k, mask, &h[j]);
                if (!ok) h[j] = 0;
                valid |= (ok ? 1u : 0u) << j;
            }
            if (whole_cluster) {
#pragma unroll
                for (uint32_t j = 0; j < QV_GROUP; ++j) {
                    cp[j] = cm[j] = 0;
                    if ((valid >> j) & 1u) cp[j] = trio_get_bounded(yp, h[j]), cm[j] = trio_get_bounded(ym, h[j]);
                }
            } else {
                // round 0 of both tables: sixteen first-slot loads are issued before any word is looked at (the scheduling
                // barrier keeps the compiler from sinking a word's use between the loads)
                uint64_t wp[QV_GROUP], wm[QV_GROUP];
#pragma unroll
                for (uint32_t j = 0; j < QV_GROUP; ++j) wp[j] = yp.table[((uint64_t)bucket_of(h[j]) << yp.cap_log2) + (key_of(h[j]) & capm_p)];
#pragma unroll
                for (uint32_t j = 0; j < QV_GROUP; ++j) wm[j] = ym.table[((uint64_t)bucket_of(h[j]) << ym.cap_log2) + (key_of(h[j]) & capm_m)];
                __builtin_amdgcn_sched_barrier(0);
                trio_settle(yp, h, valid, wp, cp);
                trio_settle(ym, h, valid, wm, cm);
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
    if (cur != ~0u) trio_flush(tally, s_cnt, q.stats, cur);
}

// The pairs across tile boundaries.  Element of tile t: its last marker's class, with TILE_RESET where t starts a sequence;
// the exclusive prefix under seg_right, started from the carry of the piece before, is the class of the last marker of
// the same sequence before tile t (0: none).  One block scans all tiles (block_scan_array: loads of 32 K tiles in flight,
// then the block-wide scans), so a marker-free stretch of any number of tiles costs nothing extra.
__global__ __launch_bounds__(BS_THREADS) void k_trio_join(TrioScan q) {
    __shared__ uint32_t sh[16];
    const uint32_t carry_in = *q.carry & 3u;
    __syncthreads(); // (the carry is read by everyone before thread 0 writes it)
    auto first_of_seq = [&](uint32_t t) { return q.desc ? (q.desc[t] & QV_FIRST) != 0u : false; };
    const uint32_t total = block_scan_array<OpSegRight>(
        q.n_tiles, sh, [&](uint32_t t) { return tile_last(q.tiles[t]) | (first_of_seq(t) ? TILE_RESET : 0u); },
        [&](uint32_t t, uint32_t prefix, uint32_t) {
            if (first_of_seq(t)) return;
            const uint32_t before = seg_right(carry_in, prefix) & 3u, first = tile_first(q.tiles[t]);
            if (before && first) {
                const uint32_t seq = q.desc ? q.desc[t] & ~QV_FIRST : 0u;
                atomicAdd(&q.stats[TRIO_STATS * (uint64_t)seq + 3u + pair_index(before, first)], 1ull);
            }
        });
    if (threadIdx.x == 0) *q.carry = seg_right(carry_in, total) & 3u;
}

void launch_trio_scan(hipStream_t s, const YakDev &pat, const YakDev &mat, const TrioScan &q, uint32_t blocks) {
    if (q.n_tiles == 0) return;
    hipLaunchKernelGGL(k_trio_scan, dim3(blocks < q.n_tiles ? (blocks ? blocks : 1u) : q.n_tiles), dim3(QV_BLOCK), 0, s, pat, mat, q);
}

void launch_trio_join(hipStream_t s, const TrioScan &q) {
    if (q.n_tiles == 0) return;
    hipLaunchKernelGGL(k_trio_join, dim3(1), dim3(BS_THREADS), 0, s, q);
}

} // namespace np2
