// Launchers of the BAM input kernels (np2_bamin.hip) for the host driver (np2_sam_host.cpp); the rule is np2_bamin_core.hpp.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "np2_bamin_core.hpp"
#include "np2_sam.hpp"

namespace np2 {

static constexpr uint32_t BAMIN_PAD = 64;       // bytes behind a piece's inflated stream that may be read (whole words are loaded)
static constexpr uint32_t BAMIN_WALK_SHORT = 1; // the walk's last entry has a block_size below 32: nothing can be found behind it
static constexpr uint32_t BAMIN_WALK_PIECE = 2; // the walk's last entry is a record longer than `limit`
static constexpr uint32_t BAMIN_KEPT = 1u << 8, BAMIN_HAS_QUAL = 1u << 9; // info[i]: the `where` code and these

struct BaminCtr {
    uint32_t count;     // record starts found
    uint32_t flags;     // BAMIN_WALK_*
    uint32_t first_err; // k_bamin_fields: the first refused record of the piece (set to 0xFFFFFFFF by the caller)
    uint32_t tail_at;   // where the walk stopped: n, or the start of a record that the stream does not finish
};

// The record walk: one lane follows the chain of block_size words from `start` through stream[0, n) (n below 2^31).  starts[i]:
// where record i begins (room for n / 36 + 2 entries); every listed record lies wholly in the stream, except a last one
// flagged BAMIN_WALK_SHORT or BAMIN_WALK_PIECE (4 + block_size above `limit`), which ends the walk.
void launch_bamin_walk(hipStream_t s, const uint8_t *stream, uint32_t start, uint32_t n, uint32_t limit, uint32_t *starts, BaminCtr *ctr);
// One wavefront per record: info[i], and for the scans kept[i], n_cig[i], n_seq[i], n_name[i] (with KEEP_NAMES or KEEP_ALL) and
// t_size[i] (with KEEP_ALL: the tail's bytes padded to a word); entry n_recs of each is set to 0.  walk_flags: ctr->flags.
void launch_bamin_fields(hipStream_t s, const uint8_t *stream, const uint32_t *starts, uint32_t n_recs, uint32_t walk_flags, uint32_t n_ref,
                         uint32_t flags, uint32_t *info, uint32_t *kept, uint32_t *n_cig, uint32_t *n_seq, uint32_t *n_name, uint32_t *t_size,
                         BaminCtr *ctr);
// One wavefront per record, at work for a kept one: what k_sam_pack, k_sam_name_copy and k_sam_tail_emit write for a line.
struct BaminOut {
    const uint32_t *kept_off, *cig_off, *seq_off, *name_off, *tail_off;
    uint64_t rec_base, cig_base, seq_base, name_base, tail_base;
    uint32_t *recs;
    int32_t *tids;
    uint64_t *keys;
    uint32_t *cigar;
    uint8_t *seq4, *names;
    uint64_t *name_ref;
    uint8_t *tails;
    uint64_t *tail_ref;
};
void launch_bamin_pack(hipStream_t s, const uint8_t *stream, const uint32_t *starts, const uint32_t *info, uint32_t n_recs, uint32_t n_ref,
                       uint32_t flags, uint32_t tie_by_strand, const BaminOut &out);

} // namespace np2
