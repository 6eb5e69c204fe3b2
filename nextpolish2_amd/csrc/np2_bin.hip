// Read binner: a PACKED separator stream of long reads against a paternal and a maternal k-mer table -> per read the
// trio tallies (k-mers, markers of either parent, the four kinds of consecutive marker pairs) and a class byte
// ('p', 'm', 'a', '0': np2_bin_core.hpp).  Read-only on the tables (YakDev).  What np2_trio.hip measures per contig, for a
// read set: no read is aligned to a tile, a tile or a lane's stretch may hold any number of reads.
//
// Input: the counter's separator stream through stage_aligned (the staging contract of np2_kmerscan.hpp); a lane owns
// the k-mers that END in its 32 bytes.  A '\n' resets the k-mer run (np2kc::push), so no k-mer spans two reads; the
// separators below n_bytes are the read boundaries (their offsets, `ends`, give every tile the read that owns its first
// byte: k_bin_owner).
//
// Probes: k_trio_scan's (the probe contract of np2_kmerscan.hpp): sixteen first-slot loads of both tables before a word is
// looked at, the collision rounds together, the whole-cluster lookup for tables that repeat keys.
//
// Order and counters, level by level (np2_bin_core.hpp):
//   lane   walks its 32 bytes; at a boundary it closes the open tally and starts a fresh Run.  What is left: `head` (the
//          read open at the stretch's start), `tail` (the read open at its end); whole reads inside the stretch go to
//          their counters at once (one set of atomics per lane and closed read, zeros skipped);
//   block  an exclusive add-scan of the lanes' boundary counts numbers the reads; a SEGMENTED exclusive scan of
//          seg_word() under seg_right gives a lane the class of the last marker of its head's read before it: one pair
//          more.  Two reads get a block-wide reduction before their atomics: the one open at the tile's start and the one
//          open at its end (a read that spans the tile costs one set of atomics for it); heads and tails of reads that
//          begin and end inside the tile go lane by lane;
//   tiles  k_bin_join, one block: a segmented exclusive scan of the tile words gives a tile the class of the last marker
//          of the read open at its start, however many marker-free tiles of the same read lie between: one pair more;
//   pieces the join starts from q.carry and leaves there what the piece ends with; k_bin_classify adds tally_in to read 0
//          and leaves the open read's tallies in tally_out.
// No atomic per k-mer anywhere; which block scans which tile, where a piece ends and where a read lies change no sum.
#include <hip/hip_runtime.h>

#include "np2_bin.hpp"
#include "np2_blockscan.hpp"
#include "np2_kmerscan.hpp"
#include "np2_trio.hpp"

namespace np2 {
using namespace np2kc;
using namespace np2qv;
using namespace np2trio;
using namespace np2bin;

namespace {

static constexpr uint32_t BIN_CHUNKS = (HALO + QV_TILE) / 16; // 16-byte pieces of a tile's window (the source is aligned)
static constexpr uint32_t BIN_WAVES = QV_BLOCK / 64;

// one read's counters, lane by lane: zeros cost nothing
__device__ __forceinline__ void bin_add(uint32_t *tallies, uint32_t read, const Tally &t) {
    uint32_t *c = tallies + BIN_STATS * (uint64_t)read;
    if (t.n_kmers) atomicAdd(c + 0, t.n_kmers);
    if (t.n_pat) atomicAdd(c + 1, t.n_pat);
    if (t.n_mat) atomicAdd(c + 2, t.n_mat);
    if (t.pp) atomicAdd(c + 3, t.pp);
    if (t.pm) atomicAdd(c + 4, t.pm);
    if (t.mp) atomicAdd(c + 5, t.mp);
    if (t.mm) atomicAdd(c + 6, t.mm);
}

// the block's counters of one read (lanes with `mine` contribute)
__device__ __forceinline__ void bin_flush(bool mine, const Tally &t, uint32_t *s_cnt, uint32_t *tallies, uint32_t read) {
    const uint32_t v[BIN_STATS] = {t.n_kmers, t.n_pat, t.n_mat, t.pp, t.pm, t.mp, t.mm};
    block_flush<BIN_STATS>(mine, v, s_cnt, tallies + BIN_STATS * (uint64_t)read);
}

} // namespace

// the read that owns a tile's first byte: the number of boundaries in front of it (a separator belongs to the read it ends)
__global__ __launch_bounds__(256) void k_bin_owner(BinScan q) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= q.n_tiles) return;
    const uint32_t at = t * QV_TILE; // (a piece is shorter than 2^32 bytes)
    uint32_t lo = 0, hi = q.n_ends;
    while (lo < hi) { // first end >= at
        const uint32_t mid = lo + (hi - lo) / 2;
        if (q.ends[mid] < at) lo = mid + 1;
        else hi = mid;
    }
    q.owner[t] = lo;
}

__global__ __launch_bounds__(QV_BLOCK) void k_bin_scan(YakDev yp, YakDev ym, BinScan q) {
    __shared__ uint4 tile[BIN_CHUNKS];
    __shared__ uint32_t s_cnt[BIN_STATS];
    __shared__ uint32_t s_scan[BIN_WAVES];
    __shared__ uint32_t s_first;
    const uint32_t tid = threadIdx.x;
    if (tid < BIN_STATS) s_cnt[tid] = 0;
    if (tid == 0) s_first = NONE;
    __syncthreads();

    const uint32_t k = yp.k; // (== ym.k: the host driver refuses anything else)
    const uint64_t mask = kmer_mask(k);
    const uint32_t *lds = reinterpret_cast<const uint32_t *>(tile) + tid * (QV_STRETCH / 4);
    const bool whole_cluster = yp.ord || ym.ord; // a table that repeats keys (yak writes none)
    const int64_t hi = (int64_t)q.n_bytes;

    for (uint32_t t = blockIdx.x; t < q.n_tiles; t += gridDim.x) {
        const uint32_t r0 = q.owner[t];
        const int64_t t0 = (int64_t)t * QV_TILE;
        stage_aligned<QV_BLOCK, BIN_CHUNKS>(tile, q.src, t0 - (int64_t)HALO, hi); // (the halo is always there)
        __syncthreads();

        // the boundaries of this lane's stretch: separators below n_bytes (the padding behind the piece is none)
        const int64_t left = hi - (t0 + (int64_t)tid * QV_STRETCH);
        const uint32_t live = left >= (int64_t)QV_STRETCH ? ~0u : left <= 0 ? 0u : (1u << (uint32_t)left) - 1u;
        uint32_t seps = 0;
#pragma unroll
        for (uint32_t i = 0; i < QV_STRETCH / 4; ++i) {
            const uint32_t w = lds[HALO / 4 + i];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) seps |= (((w >> (8 * j)) & 0xFFu) == (uint32_t)SEP ? 1u : 0u) << (4 * i + j);
        }
        seps &= live;
        uint32_t n_bounds_tile;
        const uint32_t bounds_before = block_excl_scan<OpAdd, BIN_WAVES>((uint32_t)__popc(seps), s_scan, n_bounds_tile);
        const uint32_t head_read = min(r0 + bounds_before, q.n_ends); // (never clamped when `ends` are the stream's separators)

        Roll r;
        warm_halo(r, [&](uint32_t i) { return lds[i]; }, k, mask);
        Stretch st;
        Tally tally;
        Run run;
        auto closed = [&](uint32_t i, const Tally &c) { bin_add(q.tallies, min(head_read + i, q.n_ends), c); };
#pragma unroll 1
        for (uint32_t g = 0; g < QV_STRETCH / QV_GROUP; ++g) {
            const uint32_t wa = lds[HALO / 4 + 2 * g], wb = lds[HALO / 4 + 2 * g + 1];
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
                // round 0 of both tables: sixteen first-slot loads are issued before any word is looked at
                uint64_t wp[QV_GROUP], wm[QV_GROUP];
                probe_issue(yp.table, yp.cap_log2, h, wp);
                probe_issue(ym.table, ym.cap_log2, h, wm);
                __builtin_amdgcn_sched_barrier(0);
                probe_settle(yp.table, yp.cap_log2, h, valid, wp, cp);
                probe_settle(ym.table, ym.cap_log2, h, valid, wm, cm);
            }
            const uint32_t sep8 = (seps >> (8 * g)) & 0xFFu;
#pragma unroll
            for (uint32_t j = 0; j < QV_GROUP; ++j)
                walk(st, tally, run, (valid >> j) & 1u, classify(cp[j], cm[j], q.min_count, q.mid_count), (sep8 >> j) & 1u, closed);
        }
        walk_end(st, tally, run);

        // the marker of the head's read before this lane's stretch inside the tile, and the tile's own summary
        uint32_t tile_total;
        const uint32_t before = block_excl_scan<OpSegRight, BIN_WAVES>(seg_word(st), s_scan, tile_total);
        join_head(st, before);
        if (bounds_before == 0 && !(before & 3u) && st.head_run.first) s_first = st.head_run.first; // (one lane at most)

        // the read open at the tile's start: the heads of the lanes in front of the tile's first boundary
        const bool head_opens = bounds_before == 0;
        bin_flush(head_opens, st.head, s_cnt, q.tallies, r0); // (barriers: s_first is written, the window is free)
        if (tid == 0) {
            q.tiles[t] = tile_word(s_first, tile_total);
            s_first = NONE;
        }
        if (n_bounds_tile) { // (uniform)
            // the read open at the tile's end: the tail of the lane that holds the last boundary, the heads behind it
            const bool head_ends = st.n_bounds == 0 && bounds_before == n_bounds_tile;
            const bool tail_ends = st.n_bounds != 0 && bounds_before + st.n_bounds == n_bounds_tile;
            Tally open_end = st.tail; // (a lane without a boundary has an empty tail)
            if (head_ends) open_end = st.head;
            bin_flush(head_ends || tail_ends, open_end, s_cnt, q.tallies, min(r0 + n_bounds_tile, q.n_ends));
            // reads that begin and end inside the tile, across lanes
            if (!head_opens && !head_ends) bin_add(q.tallies, head_read, st.head);
            if (st.n_bounds != 0 && !tail_ends) bin_add(q.tallies, min(head_read + st.n_bounds, q.n_ends), st.tail);
        }
    }
}

// The pairs across tile boundaries.  Element of tile t: the class of the last marker after its last boundary, with
// TILE_RESET where the tile holds a boundary; the exclusive prefix under seg_right, started from the carry of the piece
// before, is the class of the last marker of the read that is open at tile t's start (0: none).  One block scans all
// tiles (block_scan_array), so a run of marker-free tiles inside one long read is looked past by the scan.
__global__ __launch_bounds__(BS_THREADS) void k_bin_join(BinScan q) {
    __shared__ uint32_t sh[16];
    const uint32_t carry_in = *q.carry & 3u;
    __syncthreads(); // (the carry is read by everyone before thread 0 writes it)
    const uint32_t total = block_scan_array<OpSegRight>(
        q.n_tiles, sh, [&](uint32_t t) { return tile_elem(q.tiles[t]); },
        [&](uint32_t t, uint32_t prefix, uint32_t) {
            const uint32_t before = seg_right(carry_in, prefix) & 3u, first = tile_first(q.tiles[t]);
            if (before && first) atomicAdd(&q.tallies[BIN_STATS * (uint64_t)min(q.owner[t], q.n_ends) + 3u + pair_index(before, first)], 1u);
        });
    if (threadIdx.x == 0) *q.carry = seg_right(carry_in, total) & 3u;
}

// after the join, in stream order: read r < n_ends ended in this piece and gets its class; read n_ends goes on
__global__ __launch_bounds__(256) void k_bin_classify(BinScan q) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r > q.n_ends) return;
    uint32_t *c = q.tallies + BIN_STATS * (uint64_t)r;
    uint32_t v[BIN_STATS];
#pragma unroll
    for (uint32_t i = 0; i < BIN_STATS; ++i) v[i] = c[i] + (r == 0 ? q.tally_in[i] : 0u);
    if (r < q.n_ends) {
        if (r == 0) {
#pragma unroll
            for (uint32_t i = 0; i < BIN_STATS; ++i) c[i] = v[i];
        }
        q.cls[r] = read_class(v[3], v[6], q.min_score, q.minor_permille);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < BIN_STATS; ++i) q.tally_out[i] = v[i];
    }
}

void launch_bin_piece(hipStream_t s, const YakDev &pat, const YakDev &mat, const BinScan &q, uint32_t blocks) {
    if (q.n_tiles) {
        hipLaunchKernelGGL(k_bin_owner, dim3((q.n_tiles + 255) / 256), dim3(256), 0, s, q);
        hipLaunchKernelGGL(k_bin_scan, dim3(blocks < q.n_tiles ? (blocks ? blocks : 1u) : q.n_tiles), dim3(QV_BLOCK), 0, s, pat, mat, q);
        hipLaunchKernelGGL(k_bin_join, dim3(1), dim3(BS_THREADS), 0, s, q);
    }
    hipLaunchKernelGGL(k_bin_classify, dim3(q.n_ends / 256 + 1), dim3(256), 0, s, q);
}

} // namespace np2
