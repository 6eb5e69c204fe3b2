// Launchers of the kernels that pack the aligner's records into a resident SAM handle's input-order arrays (np2_alnpack.hip)
// for the mapper's host driver (np2_map_host.cpp).  The rule: include/np2_io.h, np2_sam_from_reads; its arithmetic:
// np2_alnpack_core.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "np2_alnpack_core.hpp"

namespace np2 {

// One sub-group of the aligner: reads [g0, g1) of a group whose first read is read r0 of the resident batch, right after
// launch_align_ops_emit on the same stream.
struct AlnPackJob {
    const np2aln::Rec *recs;   // [i], i counted within the group
    const uint8_t *rd_seq;     // the batch's read stream and its separators; readable 8 bytes before and 16 behind
    const uint32_t *rd_ends;   // [r0 + i]
    const uint32_t *b, *ooff;  // read i's CIGAR words at b + 2 ooff[i] + 2 (i - g0)
    uint32_t r0, g0, g1;
    const uint32_t *name_at;   // names: read r0 + i's bytes names_in[name_at[r0 + i] .. name_at[r0 + i + 1] - 1); NULL without
    const uint8_t *names_in;
    // the sizes, [i - g0], g1 - g0 + 1 entries each, and their exclusive sums
    uint32_t *kept, *n_cig, *n_seq, *n_name;
    const uint32_t *kept_off, *cig_off, *seq_off, *name_off;
};
// where the sub-group's kept records go: the input-order arrays of the handle being built
struct AlnPackOut {
    uint64_t rec_base, cig_base, seq_base, name_base; // seq_base, name_base: bytes
    uint32_t tie_by_strand;
    uint32_t *recs;    // REC_WORDS words a record
    int32_t *tids;
    uint64_t *keys;
    uint32_t *cigar;
    uint8_t *seq4;     // 4-byte aligned
    uint8_t *names;
    uint64_t *name_ref;
};

// One lane per read of [g0, g1]: kept (0 / 1), its CIGAR words, its packed SEQ bytes and, with names, the bytes of its name
// (0 for a read that is not kept; entry g1 - g0 of each is set to 0).  A kept read whose name is empty or longer than 254
// bytes: *first_bad = min(*first_bad, r0 + i), its number in the batch.
void launch_alnpack_sizes(hipStream_t s, const AlnPackJob &j, uint32_t *first_bad);
// One wavefront per read, at work for a kept one: its record, tid, key, CIGAR words, packed SEQ and, with names, its name.
void launch_alnpack(hipStream_t s, const AlnPackJob &j, const AlnPackOut &o);

} // namespace np2
