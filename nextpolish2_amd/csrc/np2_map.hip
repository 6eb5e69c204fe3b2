// The mapper on the device (the rule: include/np2_io.h, np2_map_*; the arithmetic: np2_map_core.hpp): minimizer sketch of a
// resident separator stream, the lookup of the reads' minimizers in the sorted index, the ordered emission of anchors, the
// chaining recurrence with one wavefront per read, the export of the primary chains and, on request, a read's further chains
// (k_map_chain_more: np2_io.h, "More chains") with their packing and export per unit.  Sorts and scans are rocPRIM's
// (np2_prims.hip); nothing is appended through an atomic counter, every order is part of the rule.
//
// Bounds.
//   k_map_sketch: the tile is staged by stage_aligned from `seq` - MAP_FRONT + tile offset: the driver keeps MAP_FRONT
//     separator bytes in front of the stream and the buffer readable to the next multiple of 16 after n; bytes at or beyond n
//     are masked to separators.  A lane writes words[lane * 16 .. + 16), MAP_WORDS in all.  The minimizer test of an owned
//     position idx < MAP_TILE reads words[MAP_SIDE + idx + d], |d| <= w - 1 <= MAP_SIDE - 1: inside [1, MAP_WORDS - 2].
//     Emit writes at tile_off[tile] + rank with rank below the tile's own count, taken by the count pass with the same test
//     from the same bytes; the arrays hold tile_off[n_tiles] entries.  The sequence of a position is the number of
//     separators before it, below n_ends because the stream ends in a separator.
//     Weighted: a k-mer's canonical index v is masked to 2k bits, v <= M = 4^k - 1, so its bitmap word v >> 6 < 4^k / 64, the
//     words the index handle allocates (k >= 11: 4^k is a multiple of 64); the coarse level's word v >> 12 < 4^k / 4096, its
//     words (1024 bits at k = 11).  The warm-up bytes are pushed without a lookup.
//   k_map_weights_set: entry i < n of the uploaded list; the host has checked idx[i] <= M, so both words are inside their levels.
//   k_map_seed_count: two binary searches over idx_h[0 .. idx_n); lo + occ <= idx_n.
//   k_map_read_ranges: a binary search over mz_x[0 .. n_mz); first[r] <= n_mz, and off has n_mz + 1 entries.
//   k_map_seed_emit: minimizer m writes cnt[m] anchors at off[m] - off[m0], below off[m1] - off[m0], the arrays' size; it reads
//     idx_x[lo[m] .. lo[m] + cnt[m]), inside the index by k_map_seed_count.
//   k_map_chain: read i's anchors are [aoff[r0 + i] - aoff[r0], aoff[r0 + i + 1] - aoff[r0]); candidates j lie in [max(0, i -
//     lookback), i) and their f / keys in the 64-entry rings at j & 63, written for j before anchor j + 1 is scored.
//     p[i] < i, so the walks of finish_read end.  k_map_chain_export writes hit.n entries at coff[i], walking p from chain_end.
//   k_map_chain_more: the same anchor range; every index into f, p, mark and base is below n (an arg-max winner is an
//     anchor a lane saw, a block's lane is live only with b + lane < n, a predecessor is p of such an anchor).  A read makes
//     max_chains - 1 selections at the most, so it writes units 1 .. max_chains - 1 into its max_chains - 1 slots and the
//     family holds 1 + (max_chains - 1) <= MAX_CHAINS parents.  LDS: s_ptr[ptr] with 0 <= ptr = p[i] - b < lane.
//   k_map_units_pack: read i writes uoff[i + 1] - uoff[i] = ucnt[i] <= max_chains entries at uoff[i]; the arrays hold
//     uoff[n_reads].  k_map_units_export: unit i < n_units writes hits[i].n pairs at coff[i], as k_map_chain_export does.
#include <hip/hip_runtime.h>

#include "np2_blockscan.hpp"
#include "np2_kmerscan.hpp"
#include "np2_map.hpp"
#include "np2_map_core.hpp"

namespace np2 {

// WEIGHTED: a k-mer's word carries its ordering key above its hash (np2map::push_w); whether it is listed is a load from the
// index's bitmap (bit v of 4^k, 64 to a word), in the count pass and in the emit pass alike.  With `coarse` (one bit per word of
// the bitmap: 2 MiB at k = 15, which an XCD's L2 holds, where the bitmap's 128 MiB are random loads from beyond it) that bit is
// tested first and the bitmap is read only where a word has a listed k-mer.
template <bool EMIT, bool WEIGHTED>
__global__ __launch_bounds__(MAP_BLOCK) void k_map_sketch(const uint8_t *__restrict__ seq, uint64_t n, uint64_t base, uint64_t len, uint32_t k,
                                                          uint32_t w, uint32_t tile0, uint32_t *__restrict__ tile_cnt,
                                                          const uint32_t *__restrict__ tile_off, const uint32_t *__restrict__ ends,
                                                          uint32_t n_ends, uint64_t *__restrict__ mz_h, uint64_t *__restrict__ mz_x,
                                                          const uint64_t *__restrict__ listed, const uint64_t *__restrict__ coarse) {
    __shared__ uint4 tile[MAP_TILE_BYTES / 16];
    __shared__ uint64_t words[MAP_WORDS];
    __shared__ uint32_t sh[MAP_BLOCK / 64];
    __shared__ uint32_t s_total;
    const uint64_t t0 = base + (uint64_t)blockIdx.x * MAP_TILE; // the tile's first owned position
    stage_aligned<MAP_BLOCK, MAP_TILE_BYTES / 16>(tile, seq, (int64_t)t0 - (int64_t)MAP_FRONT, (int64_t)n);
    if (threadIdx.x == 0) s_total = 0;
    __syncthreads();
    {
        // the lane's MAP_STRETCH words: those of the bytes at t0 - MAP_SIDE + lane * MAP_STRETCH on, after MAP_WARM bytes of warm-up
        const uint32_t *lw = reinterpret_cast<const uint32_t *>(tile) + threadIdx.x * (MAP_STRETCH / 4);
        const uint64_t mask = np2map::kmer_mask(k);
        np2map::Roll r;
#pragma unroll 1
        for (uint32_t d = 0; d < MAP_WARM / 4; ++d) {
            const uint32_t x = lw[d];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) (void)np2map::push(r, (uint8_t)(x >> (8 * j)), k, mask);
        }
#pragma unroll 1
        for (uint32_t d = 0; d < MAP_STRETCH / 4; ++d) {
            const uint32_t x = lw[MAP_WARM / 4 + d];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                uint64_t word;
                if (WEIGHTED)
                    word = np2map::push_w(r, (uint8_t)(x >> (8 * j)), k, mask, [&](uint64_t v) {
                        if (coarse && !((coarse[v >> 12] >> ((v >> 6) & 63u)) & 1u)) return false;
                        return ((listed[v >> 6] >> (v & 63u)) & 1u) != 0;
                    });
                else word = np2map::push(r, (uint8_t)(x >> (8 * j)), k, mask);
                words[threadIdx.x * MAP_STRETCH + d * 4 + j] = word;
            }
        }
    }
    __syncthreads();
    const uint64_t left = base + len - t0; // owned positions of the piece from t0 on (the grid has no tile beyond the piece)
    const uint32_t own = (uint32_t)(left < MAP_TILE ? left : MAP_TILE);
    uint32_t mine = 0;
    uint32_t place0 = EMIT ? tile_off[tile0 + blockIdx.x] : 0u;
#pragma unroll 1
    for (uint32_t round = 0; round < (MAP_TILE + MAP_BLOCK - 1) / MAP_BLOCK; ++round) { // (uniform: the scan below has barriers)
        const uint32_t idx = round * MAP_BLOCK + threadIdx.x;
        bool flag = false;
        if (idx < own) flag = np2map::is_minimizer([&](int32_t d) { return words[(int32_t)(MAP_SIDE + idx) + d]; }, w);
        if (!EMIT) {
            mine += flag ? 1u : 0u;
        } else {
            uint32_t total;
            const uint32_t place = place0 + block_excl_scan<OpAdd, MAP_BLOCK / 64>(flag ? 1u : 0u, sh, total);
            if (flag) {
                const uint64_t pos = t0 + idx, word = words[MAP_SIDE + idx];
                uint32_t a = 0, b = n_ends; // the separators before pos
                while (a < b) {
                    const uint32_t m = a + (b - a) / 2;
                    if ((uint64_t)ends[m] < pos) a = m + 1;
                    else b = m;
                }
                const uint64_t start = a ? (uint64_t)ends[a - 1] + 1 : 0;
                mz_h[place] = WEIGHTED ? np2map::word_hash(word, np2map::kmer_mask(k)) : word >> 1;
                mz_x[place] = np2map::mz_x(a, (uint32_t)(pos - start), (uint32_t)(word & 1u));
            }
            place0 += total;
        }
    }
    if (!EMIT) {
        mine = wave_sum(mine);
        if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(&s_total, mine);
        __syncthreads();
        if (threadIdx.x == 0) tile_cnt[tile0 + blockIdx.x] = s_total;
    }
}

// the listed indices (any order, duplicates allowed) -> their bits in the zeroed bitmap and, with `coarse`, in the zeroed coarse level
__global__ __launch_bounds__(256) void k_map_weights_set(const uint32_t *__restrict__ idx, uint64_t n, unsigned long long *__restrict__ bitmap,
                                                         unsigned long long *__restrict__ coarse) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = idx[i];
    atomicOr(&bitmap[v >> 6], 1ull << (v & 63u));
    if (coarse) atomicOr(&coarse[v >> 12], 1ull << ((v >> 6) & 63u));
}

__global__ __launch_bounds__(256) void k_map_seed_count(const uint64_t *__restrict__ mz_h, uint32_t n_mz, const uint64_t *__restrict__ idx_h,
                                                        uint32_t idx_n, uint32_t max_occ, uint32_t *__restrict__ lo, uint32_t *__restrict__ cnt,
                                                        unsigned long long *__restrict__ ctr) {
    const uint32_t m = blockIdx.x * 256 + threadIdx.x;
    if (m >= n_mz) return;
    const uint64_t h = mz_h[m];
    uint32_t a = 0, b = idx_n;
    while (a < b) { // the first entry >= h
        const uint32_t mid = a + (b - a) / 2;
        if (idx_h[mid] < h) a = mid + 1;
        else b = mid;
    }
    uint32_t c = a, d = idx_n;
    while (c < d) { // the first entry > h
        const uint32_t mid = c + (d - c) / 2;
        if (idx_h[mid] <= h) c = mid + 1;
        else d = mid;
    }
    const uint32_t occ = c - a;
    lo[m] = a;
    cnt[m] = occ >= 1 && occ <= max_occ ? occ : 0u;
    if (occ > max_occ) atomicAdd(&ctr[0], 1ull);
}

__global__ __launch_bounds__(256) void k_map_read_ranges(const uint64_t *__restrict__ mz_x, uint32_t n_mz, const uint64_t *__restrict__ off,
                                                         uint32_t n_reads, uint32_t *__restrict__ first, uint64_t *__restrict__ aoff) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r > n_reads) return;
    const uint64_t key = (uint64_t)r << 32;
    uint32_t a = 0, b = n_mz;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (mz_x[mid] < key) a = mid + 1;
        else b = mid;
    }
    first[r] = a;
    aoff[r] = off[a];
}

__global__ __launch_bounds__(256) void k_map_seed_emit(uint32_t m0, uint32_t m1, const uint64_t *__restrict__ mz_x, const uint32_t *__restrict__ lo,
                                                       const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ off, uint32_t r0,
                                                       const uint32_t *__restrict__ ends, const uint64_t *__restrict__ idx_x, uint32_t k,
                                                       uint64_t *__restrict__ khi, uint64_t *__restrict__ klo) {
    const uint32_t m = m0 + blockIdx.x * 256 + threadIdx.x;
    if (m >= m1) return;
    const uint32_t c = cnt[m];
    if (c == 0) return;
    const uint64_t x = mz_x[m], at = off[m] - off[m0];
    const uint32_t rid = (uint32_t)(x >> 32), end = (uint32_t)(x & 0xFFFFFFFFu) >> 1, strand = (uint32_t)(x & 1u);
    const uint32_t qlen = ends[rid] - (rid ? ends[rid - 1] + 1u : 0u);
    const uint32_t l = lo[m];
    for (uint32_t e = 0; e < c; ++e) np2map::anchor_of(rid - r0, end, strand, qlen, idx_x[l + e], k, &khi[at + e], &klo[at + e]);
}

// One wavefront (a block of 64) per read.  Anchor by anchor: lane d - 1 scores candidate j = i - d from the rings, a wave-wide
// maximum of the packed words picks the best (of equal scores the largest j), lane 0 settles f[i], p[i] and tracks the
// smallest i with the largest f.  Then lane 0 runs the two sweeps (np2map::finish_read), as k_bamin_walk's one lane does.
__global__ __launch_bounds__(64) void k_map_chain(MapChain c) {
    __shared__ uint64_t r_hi[64], r_lo[64];
    __shared__ int32_t r_f[64];
    const uint32_t rd = c.r0 + blockIdx.x, lane = threadIdx.x;
    const uint64_t a0 = c.aoff[rd] - c.aoff[c.r0];
    const uint32_t n = (uint32_t)(c.aoff[rd + 1] - c.aoff[rd]);
    const uint64_t *hi = c.khi + a0, *lo = c.klo + a0;
    int32_t *f = c.f + a0, *p = c.p + a0;
    int32_t best_f = 0;
    uint32_t end = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t hi_i = hi[i], lo_i = lo[i];
        int64_t cand = np2map::NO_CAND;
        if (lane < c.o.lookback && lane < i) {
            const uint32_t j = i - 1u - lane;
            cand = np2map::candidate(hi_i, lo_i, r_hi[j & 63u], r_lo[j & 63u], r_f[j & 63u], j, c.o);
        }
        for (int o = 32; o > 0; o >>= 1) {
            const int64_t other = __shfl_xor(cand, o);
            cand = other > cand ? other : cand;
        }
        int32_t fi, pi;
        np2map::settle(cand, c.o.k, &fi, &pi);
        __syncthreads(); // (every lane has read the rings: slot i & 63 held anchor i - 64)
        if (lane == 0) {
            r_hi[i & 63u] = hi_i, r_lo[i & 63u] = lo_i, r_f[i & 63u] = fi;
            f[i] = fi, p[i] = pi;
            if (fi > best_f) best_f = fi, end = i;
        }
        __syncthreads();
    }
    if (lane == 0) {
        const uint32_t qlen = c.ends[rd] - (rd ? c.ends[rd - 1] + 1u : 0u);
        __threadfence_block();
        c.chain_end[blockIdx.x] = np2map::finish_read(hi, lo, f, p, c.mark + a0, c.base + a0, n, end, qlen, c.o, &c.hits[rd]);
    }
}

__global__ __launch_bounds__(256) void k_map_chain_export(MapChain c, const uint32_t *__restrict__ coff, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n_reads) return;
    int32_t a = c.chain_end[i];
    if (a < 0) return;
    const uint32_t rd = c.r0 + i;
    const uint64_t a0 = c.aoff[rd] - c.aoff[c.r0];
    uint32_t t = c.hits[rd].n;
    const uint32_t at = coff[i];
    for (; a >= 0 && t > 0; a = c.p[a0 + a]) {
        --t;
        const uint64_t l = c.klo[a0 + a];
        out[2 * (uint64_t)(at + t)] = np2map::lo_r(l), out[2 * (uint64_t)(at + t) + 1] = np2map::lo_q(l);
    }
}

// More chains of a read (np2map::select_more is the same steps with one lane): one wavefront per read, on what k_map_chain left.
// Per selection: the arg-max of f[i] - base[i] over the unmarked anchors is a wave reduction over lanes striding the anchors;
// lane 0 follows the chain back, marks it, fills its hit and classes it (the walk is serial, as the primary's is); then base is
// swept again from the chain's first anchor on in blocks of 64 anchors, a lane an anchor.  p[i] lies in [i - lookback, i) with
// lookback <= 64, so a predecessor is in this block or in an earlier one: an earlier block's base is final and read from
// memory, inside the block a lane follows p through LDS by pointer jumping (six rounds at the most).
__global__ __launch_bounds__(64) void k_map_chain_more(MapChain c, MapMore mo) {
    __shared__ np2map::Family fm;
    __shared__ int32_t s_val[64], s_ptr[64];
    __shared__ uint32_t s_first;
    const uint32_t rd = c.r0 + blockIdx.x, lane = threadIdx.x, stride = mo.m.max_chains - 1u;
    if (c.chain_end[blockIdx.x] < 0) { // an unmapped read is its one unit
        if (lane == 0) mo.ucnt[blockIdx.x] = 1;
        return;
    }
    const uint64_t a0 = c.aoff[rd] - c.aoff[c.r0];
    const uint32_t n = (uint32_t)(c.aoff[rd + 1] - c.aoff[rd]);
    const uint64_t *hi = c.khi + a0, *lo = c.klo + a0;
    const int32_t *f = c.f + a0, *p = c.p + a0;
    int32_t *base = c.base + a0;
    uint8_t *mark = c.mark + a0;
    const size_t slot = (size_t)blockIdx.x * stride;
    const uint32_t qlen = c.ends[rd] - (rd ? c.ends[rd - 1] + 1u : 0u);
    np2map::MoreCounts mc{};
    if (lane == 0) np2map::family_begin(fm, c.hits[rd]);
#pragma unroll 1
    for (uint32_t sel = 1; sel < mo.m.max_chains; ++sel) {
        int64_t best = np2map::NO_CAND;
        for (uint32_t i = lane; i < n; i += 64) {
            if (mark[i]) continue;
            const int64_t key = np2map::more_key(f[i] - base[i], i);
            best = key > best ? key : best;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const int64_t other = __shfl_xor(best, o);
            best = other > best ? other : best;
        }
        if (best == np2map::NO_CAND) break;
        int64_t score;
        uint32_t end;
        np2map::more_unkey(best, &score, &end);
        if (score < (int64_t)c.o.min_score) break;
        if (lane == 0) {
            np2map::Hit h;
            s_first = np2map::take_chain(hi, lo, p, mark, end, (uint32_t)score, qlen, c.o, &h);
            np2map::place_chain(fm, h, end, c.o, mo.m, mo.uhits + slot, mo.ucls + slot, mo.upar + slot, mo.uend + slot, &mc);
        }
        __syncthreads(); // (the chain's marks and its first anchor are the wavefront's)
        const uint32_t first = s_first;
        for (uint32_t b = first & ~63u; b < n; b += 64) {
            const uint32_t i = b + lane;
            const bool live = i < n && !mark[i];
            int32_t val = 0, ptr = -1; // ptr >= 0: base[i] is the base of anchor b + ptr, not known yet
            if (live) {
                const int32_t pi = p[i];
                if (pi < 0 || mark[pi] || (uint32_t)pi < b) val = np2map::base_step(pi, mark, f, base);
                else ptr = pi - (int32_t)b;
            }
            while (__any(ptr >= 0)) {
                s_ptr[lane] = ptr, s_val[lane] = val;
                __syncthreads();
                if (ptr >= 0) {
                    const int32_t t = s_ptr[ptr];
                    if (t < 0) val = s_val[ptr], ptr = -1;
                    else ptr = t;
                }
                __syncthreads();
            }
            if (live) base[i] = val;
            __syncthreads(); // (the next block reads this one's base from memory)
        }
    }
    if (lane == 0) {
        np2map::family_end(fm, mo.uhits + slot);
        mo.ucnt[blockIdx.x] = fm.n_units;
        const uint32_t v[5] = {mc.selections, mc.dropped_cnt, mc.dropped_pri, mc.kept_supp, mc.kept_sec};
        for (int t = 0; t < 5; ++t)
            if (v[t]) atomicAdd(&mo.ctr[t], (unsigned long long)v[t]);
    }
}

__global__ __launch_bounds__(256) void k_map_units_pack(MapChain c, MapMore mo, MapUnits u) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n_reads) return;
    const uint32_t at = u.uoff[i], cnt = u.uoff[i + 1] - at;
    const size_t slot = (size_t)i * (mo.m.max_chains - 1u);
    u.hits[at] = c.hits[c.r0 + i], u.cls[at] = (uint8_t)np2map::CLS_PRIMARY, u.parent[at] = 0, u.end[at] = c.chain_end[i], u.read[at] = i;
    for (uint32_t t = 1; t < cnt; ++t) {
        u.hits[at + t] = mo.uhits[slot + t - 1], u.cls[at + t] = (uint8_t)mo.ucls[slot + t - 1], u.parent[at + t] = mo.upar[slot + t - 1];
        u.end[at + t] = mo.uend[slot + t - 1], u.read[at + t] = i;
    }
}

__global__ __launch_bounds__(256) void k_map_units_export(MapChain c, MapUnits u, uint32_t n_units, const uint32_t *__restrict__ coff,
                                                          uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_units) return;
    int32_t a = u.end[i];
    if (a < 0) return;
    const uint32_t rd = c.r0 + u.read[i];
    const uint64_t a0 = c.aoff[rd] - c.aoff[c.r0];
    uint32_t t = u.hits[i].n;
    const uint32_t at = coff[i];
    for (; a >= 0 && t > 0; a = c.p[a0 + a]) {
        --t;
        const uint64_t l = c.klo[a0 + a];
        out[2 * (uint64_t)(at + t)] = np2map::lo_r(l), out[2 * (uint64_t)(at + t) + 1] = np2map::lo_q(l);
    }
}

void launch_map_chain_more(hipStream_t s, const MapChain &c, const MapMore &mo) {
    if (c.n_reads == 0) return;
    hipLaunchKernelGGL(k_map_chain_more, dim3(c.n_reads), dim3(64), 0, s, c, mo);
}
void launch_map_units_pack(hipStream_t s, const MapChain &c, const MapMore &mo, const MapUnits &u) {
    if (c.n_reads == 0) return;
    hipLaunchKernelGGL(k_map_units_pack, dim3((c.n_reads + 255) / 256), dim3(256), 0, s, c, mo, u);
}
void launch_map_units_export(hipStream_t s, const MapChain &c, const MapUnits &u, uint32_t n_units, const uint32_t *coff, uint32_t *out) {
    if (n_units == 0) return;
    hipLaunchKernelGGL(k_map_units_export, dim3((n_units + 255) / 256), dim3(256), 0, s, c, u, n_units, coff, out);
}

void launch_map_sketch_count(hipStream_t s, const uint8_t *seq, uint64_t n, uint64_t base, uint64_t len, uint32_t k, uint32_t w,
                             uint32_t tile0, uint32_t *tile_cnt, const uint64_t *listed, const uint64_t *coarse) {
    if (len == 0) return;
    if (listed)
        hipLaunchKernelGGL((k_map_sketch<false, true>), dim3(map_tiles(len)), dim3(MAP_BLOCK), 0, s, seq, n, base, len, k, w, tile0, tile_cnt,
                           nullptr, nullptr, 0u, nullptr, nullptr, listed, coarse);
    else
        hipLaunchKernelGGL((k_map_sketch<false, false>), dim3(map_tiles(len)), dim3(MAP_BLOCK), 0, s, seq, n, base, len, k, w, tile0, tile_cnt,
                           nullptr, nullptr, 0u, nullptr, nullptr, nullptr, nullptr);
}
void launch_map_sketch_emit(hipStream_t s, const uint8_t *seq, uint64_t n, uint64_t base, uint64_t len, uint32_t k, uint32_t w,
                            uint32_t tile0, const uint32_t *tile_off, const uint32_t *ends, uint32_t n_ends, uint64_t *mz_h, uint64_t *mz_x,
                            const uint64_t *listed, const uint64_t *coarse) {
    if (len == 0) return;
    if (listed)
        hipLaunchKernelGGL((k_map_sketch<true, true>), dim3(map_tiles(len)), dim3(MAP_BLOCK), 0, s, seq, n, base, len, k, w, tile0, nullptr,
                           tile_off, ends, n_ends, mz_h, mz_x, listed, coarse);
    else
        hipLaunchKernelGGL((k_map_sketch<true, false>), dim3(map_tiles(len)), dim3(MAP_BLOCK), 0, s, seq, n, base, len, k, w, tile0, nullptr,
                           tile_off, ends, n_ends, mz_h, mz_x, nullptr, nullptr);
}
void launch_map_weights_set(hipStream_t s, const uint32_t *idx, uint64_t n, uint64_t *bitmap, uint64_t *coarse) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_map_weights_set, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, idx, n, reinterpret_cast<unsigned long long *>(bitmap),
                       reinterpret_cast<unsigned long long *>(coarse));
}
void launch_map_seed_count(hipStream_t s, const uint64_t *mz_h, uint32_t n_mz, const uint64_t *idx_h, uint32_t idx_n, uint32_t max_occ,
                           uint32_t *lo, uint32_t *cnt, unsigned long long *ctr) {
    if (n_mz == 0) return;
    hipLaunchKernelGGL(k_map_seed_count, dim3((n_mz + 255) / 256), dim3(256), 0, s, mz_h, n_mz, idx_h, idx_n, max_occ, lo, cnt, ctr);
}
void launch_map_read_ranges(hipStream_t s, const uint64_t *mz_x, uint32_t n_mz, const uint64_t *off, uint32_t n_reads, uint32_t *first,
                            uint64_t *aoff) {
    hipLaunchKernelGGL(k_map_read_ranges, dim3((n_reads + 1 + 255) / 256), dim3(256), 0, s, mz_x, n_mz, off, n_reads, first, aoff);
}
void launch_map_seed_emit(hipStream_t s, uint32_t m0, uint32_t m1, const uint64_t *mz_x, const uint32_t *lo, const uint32_t *cnt,
                          const uint64_t *off, uint32_t r0, const uint32_t *ends, const uint64_t *idx_x, uint32_t k, uint64_t *khi,
                          uint64_t *klo) {
    if (m1 <= m0) return;
    hipLaunchKernelGGL(k_map_seed_emit, dim3((m1 - m0 + 255) / 256), dim3(256), 0, s, m0, m1, mz_x, lo, cnt, off, r0, ends, idx_x, k, khi, klo);
}
void launch_map_chain(hipStream_t s, const MapChain &c) {
    if (c.n_reads == 0) return;
    hipLaunchKernelGGL(k_map_chain, dim3(c.n_reads), dim3(64), 0, s, c);
}
void launch_map_chain_export(hipStream_t s, const MapChain &c, const uint32_t *coff, uint32_t *out) {
    if (c.n_reads == 0) return;
    hipLaunchKernelGGL(k_map_chain_export, dim3((c.n_reads + 255) / 256), dim3(256), 0, s, c, coff, out);
}

} // namespace np2
