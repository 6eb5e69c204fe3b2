// Launchers of the tag kernels (np2_aligntags.hip): MD, cs and the = / X CIGAR of aligned records.  The rule: include/np2_io.h,
// np2_map_align_*, "Tags"; its arithmetic: np2_aligntags_core.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "np2_align.hpp"
#include "np2_aligntags_core.hpp"

namespace np2 {

// n records from one of two sources.  from_aligner: reads [g0, g0 + n) of an aligner sub-group, as k_align_ops_emit left them
// (c.recs, c.b, c.ooff).  Otherwise a caller's records (np2_align_tags_device): record i's reference columns start at ref +
// t_off[i], its read, already oriented, at reads + q_off[i], its words are cigar[cig_off[i] .. cig_off[i + 1]); the host has
// checked that every column lies inside the two buffers.
struct TagJob {
    AlignJob c;
    uint32_t g0, from_aligner;
    const uint8_t *ref, *reads;
    const uint64_t *t_off, *q_off, *cig_off;
    const uint32_t *cigar;
    uint32_t n, flags;              // np2aln::ALN_MD | ALN_CS | ALN_EQX: an output that is not asked for has size 0
    uint32_t *n_md, *n_cs, *n_eqx;  // [n + 1], the last 0
    const uint64_t *md_off, *cs_off; // their exclusive sums
    const uint32_t *eqx_off;
    char *md, *cs;
    uint32_t *eqx;
};

// one wavefront per record: the sizes of its MD text, cs text and split CIGAR
void launch_align_tags_size(hipStream_t s, const TagJob &j);
// ... and, after the three scans, the texts and the words themselves
void launch_align_tags_emit(hipStream_t s, const TagJob &j);

} // namespace np2
