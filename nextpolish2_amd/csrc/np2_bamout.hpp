// Launchers of the BAM writer's kernels (np2_bamout.hip) for its host driver (np2_bamout_host.cpp).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "np2_bamout_core.hpp"

namespace np2 {

// the resident arrays of a SAM opened with its names, as the kernels read them
struct BamSrc {
    const uint32_t *recs; // SAM_REC_WORDS words a record, sorted order
    const int32_t *tids;
    const uint32_t *cigar;
    const uint8_t *seq4;
    const uint8_t *names;
    const uint64_t *name_ref;
    const uint8_t *tails;     // NP2_SAM_KEEP_ALL: the tails and, per record, offset << 1 | has_qual; both nullptr for the lean stream
    const uint64_t *tail_ref;
    uint32_t n;
};

// A lane per record: sz[i] = its bytes in the stream (sz[n] = 0), be[i] = bin | last window << 16, ref->* = the first record
// of each refusal (set to NONE by the caller), n_intv[tid] = max(n_intv[tid], last window + 1) (zeroed by the caller).
void launch_bam_sizes(hipStream_t s, BamSrc src, uint32_t *sz, uint32_t *be, np2bam::Refusals *ref, uint32_t *n_intv);
// Bytes [b0, b1) of the stream's record part to dst[0, b1 - b0): off[i] (n + 1 entries, the scan of sz) is where record i begins,
// counted from the first record; b0 is a multiple of 4 and dst 4-byte aligned.  A wavefront per record that intersects
// the range writes the record's bytes inside it.
void launch_bam_emit(hipStream_t s, BamSrc src, const uint64_t *off, const uint32_t *be, uint64_t b0, uint64_t b1, uint8_t *dst, uint32_t n_blocks);
// A lane per record: beg[i] and end[i] = V(hdr + off[i]), V(hdr + off[i + 1]) over C, the blocks' file offsets;
// head[i] = 1 where (tid, bin) differs from the record before (head[0] = 1, head[n] = 0)
void launch_bai_voff(hipStream_t s, BamSrc src, const uint64_t *off, const uint32_t *be, uint64_t hdr, const uint64_t *C, uint64_t *beg,
                     uint64_t *end, uint32_t *head);
// run[i] = heads before i (the scan of head).  Per run r: key[r] = tid << 32 | bin, rbeg[r] = beg of its first record,
// rend[r] = end of its last, val[r] = r
void launch_bai_chunks(hipStream_t s, BamSrc src, const uint32_t *be, const uint64_t *beg, const uint64_t *end, const uint32_t *head,
                       const uint32_t *run, uint64_t *key, uint64_t *rbeg, uint64_t *rend, uint32_t *val);
// win[win_off[tid] + w] = min(.., beg[i]) over every window w record i overlaps (win: set to all ones by the caller)
void launch_bai_linear(hipStream_t s, BamSrc src, const uint32_t *be, const uint64_t *beg, const uint32_t *win_off, unsigned long long *win);

} // namespace np2
