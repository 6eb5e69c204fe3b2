// Launchers of the aligner's kernels (np2_align.hip) for the mapper's host driver (np2_map_host.cpp).  The rule:
// include/np2_io.h, np2_map_align_*; its arithmetic: np2_align_core.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "np2_align_core.hpp"

namespace np2 {

// One group of the mapper: reads [r0, r0 + n_reads) of the resident batch, their hits and exported primary chains (or, with
// unit_read, the group's units).
struct AlignJob {
    const uint8_t *asm_seq;   // the index's assembly stream and its separators
    const uint32_t *asm_ends;
    const uint8_t *rd_seq;    // the batch's read stream and its separators
    const uint32_t *rd_ends;
    const np2map::Hit *hits;  // [r0 + i]; with unit_read: [i]
    const uint32_t *coff, *chain; // read i's (r, q) pairs at chain + 2 coff[i]
    uint32_t r0, n_reads, k, max_cells;
    np2aln::Opts o;
    uint8_t *pin;             // per chain anchor
    uint32_t *nslots, *soff;  // per read: pins + 1 (0: unmapped), and their exclusive sums [n_reads + 1]
    np2aln::Slot *slots;
    uint32_t *slot_read;      // per slot: its read (group-local)
    uint32_t *cells;          // per slot [n_slots + 1]
    uint64_t *tb_off;         // their exclusive sums
    uint64_t *read_cells;     // [n_reads + 1]: tb_off at each read's first slot
    np2aln::Res *res;
    uint8_t *tb;
    unsigned long long *ctr;  // np2aln::C_N counters
    uint32_t *nops, *ooff;    // per read: raw ops, and their exclusive sums
    uint32_t *a, *b;          // raw ops at ooff[i] - ooff[g0]; the CIGAR at 2 (ooff[i] - ooff[g0]) + 2 (i - g0)
    np2aln::Rec *recs;        // [i]
    // More chains (np2_io.h, "More chains"): null, or the jobs are units: a read together with one kept chain.  Job i is read
    // r0 + unit_read[i] with the hit hits[i] and its own chain at coff[i]; n_reads counts the units, and every per-read array
    // above is per unit.
    const uint32_t *unit_read;
};

__device__ __forceinline__ const np2map::Hit &hit_of(const AlignJob &c, uint32_t i) { return c.unit_read ? c.hits[i] : c.hits[c.r0 + i]; }

// read i of the group and the contig its hit names (the aligner's kernels and the tag kernels, np2_aligntags.hip)
__device__ __forceinline__ np2aln::Seqs seqs_of(const AlignJob &c, uint32_t i) {
    const uint32_t rd = c.r0 + (c.unit_read ? c.unit_read[i] : i);
    const np2map::Hit &h = hit_of(c, i);
    const uint32_t q_at = rd ? c.rd_ends[rd - 1] + 1u : 0u;
    const uint32_t t_at = h.tid > 0 ? c.asm_ends[h.tid - 1] + 1u : 0u;
    np2aln::Seqs s;
    s.t = c.asm_seq + t_at, s.tlen = c.asm_ends[h.tid] - t_at;
    s.q = c.rd_seq + q_at, s.qlen = h.qlen, s.rev = h.rev;
    return s;
}

// pin flags and slot counts per read
void launch_align_pins(hipStream_t s, const AlignJob &c);
// the slots of every mapped read (head, raw segments, tail) at soff[i]
void launch_align_plan(hipStream_t s, const AlignJob &c);
// one thread per slot: trim, class, band, cells; the counters
void launch_align_classify(hipStream_t s, const AlignJob &c, uint32_t n_slots);
void launch_align_read_cells(hipStream_t s, const AlignJob &c);
// one wavefront per slot of the reads [g0, g1), slots [s0, s1): the banded matrix and its traceback bits at tb + (tb_off - tb_base)
void launch_align_dp(hipStream_t s, const AlignJob &c, uint32_t s0, uint32_t s1, uint64_t tb_base);
// one lane per read of [g0, g1): the number of raw ops; then the ops, the final CIGAR and the record
void launch_align_ops_count(hipStream_t s, const AlignJob &c, uint32_t g0, uint32_t g1, uint64_t tb_base);
void launch_align_ops_emit(hipStream_t s, const AlignJob &c, uint32_t g0, uint32_t g1, uint64_t tb_base);

} // namespace np2
