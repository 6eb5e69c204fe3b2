// Launchers of the edit kernels (np2_edits.hip) for their host driver (np2_edits_host.cpp).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "np2_edits_core.hpp"
#include "np2_kernels.hpp"

namespace np2 {

// Counters of one call, on the device from the first kernel to the last: nothing of it is read back between stages.
struct EditsDev {
    uint32_t err;                 // np2edits::E_* | LB_ERR
    uint32_t has_span, first, last;
    uint32_t n_raw, n_long, n_edits, same_runs;
    uint32_t n_kind[5];
    uint32_t ref_bytes, alt_bytes, pad;
    unsigned long long bases_inserted, bases_deleted, outside;
};

struct EditsSeq { // the three inputs and what k_edits_heads derives from them
    const uint8_t *ref;
    const uint8_t *out;
    const uint32_t *pos;
    uint32_t L, n;
    uint32_t *gstart, *gend; // [L]
};
struct EditsRuns { // raw runs [0, n_raw), capacity max_runs
    uint32_t max_runs;
    uint32_t *run_s, *run_e;                 // inclusive
    uint32_t *t_s, *t_os, *t_lr, *t_la;      // trimmed
    uint32_t *real;                          // 1: an edit
    uint32_t *long_list;                     // runs left to the wavefront variant
};
struct EditsList { // real edits [0, n_edits)
    uint32_t *s0, *os0, *lr, *la, *sh; // before the shift, and the shift
    np2edits::Edit *rec;               // after it
};
struct EditsTables {
    YakDev y[np2edits::MAX_TABLES];
    uint32_t n;
    uint32_t min_count;
};

void launch_edits_unpack_ref(hipStream_t s, const uint8_t *refnib, uint32_t L, uint8_t *ref);
void launch_edits_heads(hipStream_t s, const EditsSeq &q, EditsDev *ctr);
void launch_edits_flags(hipStream_t s, const EditsSeq &q, EditsDev *ctr, uint32_t *hbits, uint32_t *tbits, uint32_t n_words);
void launch_edits_runs(hipStream_t s, const uint32_t *hbits, const uint32_t *tbits, const uint32_t *hoff, const uint32_t *toff,
                       uint32_t n_words, const EditsRuns &r, EditsDev *ctr);
void launch_edits_trim(hipStream_t s, const EditsSeq &q, const EditsRuns &r, EditsDev *ctr, uint32_t wave_blocks);
void launch_edits_compact(hipStream_t s, const EditsRuns &r, const uint32_t *eidx, const EditsList &e, EditsDev *ctr);
void launch_edits_shift(hipStream_t s, const EditsSeq &q, const EditsList &e, uint32_t max_runs, EditsDev *ctr);
void launch_edits_emit(hipStream_t s, const EditsSeq &q, const EditsList &e, const uint32_t *roff, const uint32_t *aoff, uint32_t max_runs,
                       uint8_t *ref_pool, uint8_t *alt_pool, EditsDev *ctr, uint32_t blocks);
// sup[(edit * n_tables + table) * 4 ..]: n_in, absent_in, n_out, absent_out
void launch_edits_support(hipStream_t s, const EditsSeq &q, const EditsList &e, const EditsTables &t, uint32_t *sup, uint32_t max_runs,
                          const EditsDev *ctr, uint32_t blocks);

} // namespace np2
