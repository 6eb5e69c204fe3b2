// Launchers of the mapper's kernels (np2_map.hip) and the pair sort they need (np2_prims.hip), for the host driver
// (np2_map_host.cpp).  The rule: include/np2_io.h; its arithmetic: np2_map_core.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "np2_map_core.hpp"

namespace np2 {

// The sketch kernel's tiling.  A block computes the words (np2map::push) of MAP_WORDS consecutive bytes, MAP_STRETCH a lane,
// and owns the MAP_TILE positions in their middle: a minimizer test looks w - 1 <= MAP_SIDE words to either side, and the
// first word needs the k - 1 <= MAP_WARM bytes before it.  So a tile reads MAP_FRONT = MAP_SIDE + MAP_WARM >= k + w - 2 bytes
// before its first position and MAP_SIDE >= w - 1 after its last.  (These are this kernel's own halo constants; the k-mer
// scans keep np2kc::HALO.)
static constexpr uint32_t MAP_BLOCK = 256, MAP_STRETCH = 16, MAP_WORDS = MAP_BLOCK * MAP_STRETCH;
static constexpr uint32_t MAP_SIDE = 64, MAP_WARM = 32, MAP_FRONT = MAP_SIDE + MAP_WARM;
static constexpr uint32_t MAP_TILE = MAP_WORDS - 2 * MAP_SIDE;
static constexpr uint32_t MAP_TILE_BYTES = MAP_WARM + MAP_WORDS;
static_assert(MAP_SIDE >= np2map::W_MAX - 1 && MAP_WARM >= np2map::K_MAX - 1, "the halo covers the largest k and w");
static_assert(MAP_TILE % 16 == 0 && MAP_FRONT % 16 == 0 && MAP_TILE_BYTES % 16 == 0, "tiles are staged with aligned 16-byte loads");

inline uint32_t map_tiles(uint64_t len) { return (uint32_t)((len + MAP_TILE - 1) / MAP_TILE); }

// One piece [base, base + len) of a resident separator stream of n bytes.  `seq` points at the stream's first byte; the
// MAP_FRONT bytes before it are separators, the buffer is readable up to the next multiple of 16 after n, and base is a
// multiple of 16.  counts: per tile (tile0 + block) the minimizers it owns; emit: their (h, x) at tile_off[tile0 + block] on.
// listed: null for the unweighted sketch, otherwise the weight set's bitmap (map_weight_words(k) words, np2map::push_w), and
// coarse: null or its coarse level (map_weight_coarse_words(k) words).
void launch_map_sketch_count(hipStream_t s, const uint8_t *seq, uint64_t n, uint64_t base, uint64_t len, uint32_t k, uint32_t w,
                             uint32_t tile0, uint32_t *tile_cnt, const uint64_t *listed = nullptr, const uint64_t *coarse = nullptr);
void launch_map_sketch_emit(hipStream_t s, const uint8_t *seq, uint64_t n, uint64_t base, uint64_t len, uint32_t k, uint32_t w,
                            uint32_t tile0, const uint32_t *tile_off, const uint32_t *ends, uint32_t n_ends, uint64_t *mz_h, uint64_t *mz_x,
                            const uint64_t *listed = nullptr, const uint64_t *coarse = nullptr);
// The weight set on the device: one bit per canonical k-mer index, 4^k bits as 64-bit words (128 MiB at k = 15, 512 KiB at
// k = 11), and the coarse level: one bit per word of the bitmap, set where the word is not zero (2 MiB at k = 15).  Both are
// zeroed on the stream first; every idx[i] <= 4^k - 1.  coarse may be null.
inline size_t map_weight_words(uint32_t k) { return (size_t)1 << (2u * k - 6u); }
inline size_t map_weight_coarse_words(uint32_t k) { return (size_t)1 << (2u * k - 12u); }
void launch_map_weights_set(hipStream_t s, const uint32_t *idx, uint64_t n, uint64_t *bitmap, uint64_t *coarse);
// per read minimizer: its run [lo, lo + occ) in the index's sorted hashes; cnt = occ when 1 <= occ <= max_occ, else 0;
// ctr[0] += minimizers dropped by occurrence
void launch_map_seed_count(hipStream_t s, const uint64_t *mz_h, uint32_t n_mz, const uint64_t *idx_h, uint32_t idx_n, uint32_t max_occ,
                           uint32_t *lo, uint32_t *cnt, unsigned long long *ctr);
// per read r in [0, n_reads]: first[r] = its first minimizer, aoff[r] = off[first[r]] (off: exclusive sums of cnt, n_mz + 1)
void launch_map_read_ranges(hipStream_t s, const uint64_t *mz_x, uint32_t n_mz, const uint64_t *off, uint32_t n_reads, uint32_t *first,
                            uint64_t *aoff);
// anchors of the minimizers [m0, m1) (reads r0 on), at off[m] - off[m0]
void launch_map_seed_emit(hipStream_t s, uint32_t m0, uint32_t m1, const uint64_t *mz_x, const uint32_t *lo, const uint32_t *cnt,
                          const uint64_t *off, uint32_t r0, const uint32_t *ends, const uint64_t *idx_x, uint32_t k, uint64_t *khi,
                          uint64_t *klo);
// reads [r0, r0 + n_reads) of the batch, one wavefront each, over their sorted anchors (at aoff[r] - aoff[r0])
struct MapChain {
    const uint64_t *khi, *klo, *aoff;
    const uint32_t *ends;
    int32_t *f, *p, *base;
    uint8_t *mark;
    np2map::Hit *hits;  // [r0 + i]
    int32_t *chain_end; // [i]: the primary chain's last anchor (read-local) or -1
    uint32_t r0, n_reads;
    np2map::Opts o;
};
void launch_map_chain(hipStream_t s, const MapChain &c);
// the primary chains' anchors (r, q), first to last, at coff[i] on
void launch_map_chain_export(hipStream_t s, const MapChain &c, const uint32_t *coff, uint32_t *out);

// More chains (np2map::MultiOpts with max_chains > 1), right behind launch_map_chain on the f, p, mark and base it left: one
// wavefront per read makes the further selections.  A read's kept further units go to its max_chains - 1 slots (unit u of
// read i at i * (max_chains - 1) + u - 1), ucnt[i] is its units with the primary (1 for an unmapped read), ctr[0 .. 5) take
// np2map::MoreCounts' sums.
struct MapMore {
    np2map::MultiOpts m;
    np2map::Hit *uhits;
    uint32_t *ucls, *upar;
    int32_t *uend;
    uint32_t *ucnt; // [n_reads]
    unsigned long long *ctr;
};
void launch_map_chain_more(hipStream_t s, const MapChain &c, const MapMore &mo);
// ... and after an exclusive scan of ucnt (uoff[n_reads + 1]): the units in read order, the primary first, then selection
// order: hits, cls, parent, the chain's last anchor (read-local, -1 for an unmapped primary) and the read (group-local)
struct MapUnits {
    const uint32_t *uoff;
    np2map::Hit *hits;
    uint8_t *cls;
    uint32_t *parent, *read;
    int32_t *end;
};
void launch_map_units_pack(hipStream_t s, const MapChain &c, const MapMore &mo, const MapUnits &u);
// the units' chains (r, q), first to last, at coff[unit] on: k_map_chain_export per unit, each chain ending after its own n anchors
void launch_map_units_export(hipStream_t s, const MapChain &c, const MapUnits &u, uint32_t n_units, const uint32_t *coff, uint32_t *out);

// rocPRIM's stable radix sort of (uint64 key, uint64 value) pairs over the key bits [0, end_bit) (np2_prims.hip)
size_t prim_pairs64_temp_bytes(size_t n);
int prim_sort_pairs_u64_u64(hipStream_t s, void *tmp, size_t tmp_bytes, const uint64_t *kin, uint64_t *kout, const uint64_t *vin,
                            uint64_t *vout, size_t n, unsigned end_bit);

} // namespace np2
