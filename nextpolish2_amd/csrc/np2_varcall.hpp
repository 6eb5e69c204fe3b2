// Launchers of the variant caller's kernels (np2_varcall.hip) and the driver its C entry points share (np2_varcall_host.cpp).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "np2_depth.hpp"
#include "np2_varcall_core.hpp"

namespace np2 {

// counters of one call, zeroed by the caller before the first launch
struct VarDev {
    unsigned long long callable, calls[6];
    uint32_t n_seen, n_counted, n_no_seq, n_skipped, n_events, n_alleles, n_calls;
    uint32_t err; // LB_ERR: a look-back wait gave up; VC_ERR_*: below
};
static constexpr uint32_t VC_ERR_SEQ = 1u, VC_ERR_EVENTS = 2u, VC_ERR_CALLS = 4u; // SEQ outside its buffer; more events / calls than room

// A wavefront per record: admission, +1 / -1 into diff (L + 1 zeroed words), mismatches into alt (4 L zeroed words), and the
// keys of its indel events after their left shift into ev_hi / ev_lo (room for ev_cap; ctr->n_events counts them, in no
// particular order).  ref: the contig's L bytes; seq: seq_bytes bytes of 4-bit SEQ.
void launch_varcall_records(hipStream_t s, const np2_bamrec_t *recs, const uint32_t *cigar, const uint8_t *seq, uint64_t seq_bytes, uint32_t n_recs,
                            const uint8_t *ref, uint32_t L, np2vc::Rule rule, uint32_t *diff, uint32_t *alt, uint64_t *ev_hi, uint64_t *ev_lo,
                            uint32_t ev_cap, VarDev *ctr);
// Over the n keys in ascending (hi, lo): ctr->n_alleles, and per (anchor, kind) the allele of the greatest count (the first
// of the greatest in key order): best[2 anchor + kind] = 1 + the index of its first key, best_count[...] = its count.
// best / best_count: 2 L zeroed words each.
void launch_varcall_alleles(hipStream_t s, const uint64_t *ev_hi, const uint64_t *ev_lo, uint32_t n, uint32_t L, uint32_t *best, uint32_t *best_count,
                            VarDev *ctr);
// The calls of every position.  calls == nullptr: they are counted (ctr->n_calls, ctr->calls, ctr->callable) and lb is not
// used; else they are written in order (room for max_calls; lb: depth_blocks(L) blocks) and nothing is counted.
void launch_varcall_calls(hipStream_t s, const Lookback &lb, const uint8_t *ref, uint32_t L, const uint32_t *cov, const uint32_t *alt,
                          const uint32_t *best, const uint32_t *best_count, const uint64_t *ev_hi, const uint64_t *ev_lo, np2vc::Rule rule,
                          np2_varcall_t *calls, uint32_t max_calls, VarDev *ctr);

} // namespace np2

struct np2_ctx;
namespace np2h {
// opts as the C ABI takes them -> the rule; throws NP2_E_ARG (nothing is launched before it)
np2vc::Rule varcall_rule(const np2_varcall_opts_t *opts);
// The caller over records, CIGAR words (n_cig of them) and SEQ that are on ctx's device already; ref is the host's.  Results as
// np2_varcall_from_records returns them (*calls a pinned block, released with np2_free).
void varcall_device(np2_ctx *cx, const uint8_t *ref, uint32_t L, const np2_bamrec_t *d_recs, uint32_t n_recs, const uint32_t *d_cigar,
                    uint64_t n_cig, const uint8_t *d_seq, uint64_t seq_bytes, const np2vc::Rule &rule, np2_varcall_t **calls, uint32_t *n_calls,
                    uint32_t *cov, uint32_t *alt, np2_varcall_stats_t *stats);
// every record's CIGAR inside n_cig words and SEQ inside seq_bytes bytes, or NP2_E_ARG naming `who`
void varcall_check_records(const np2_bamrec_t *recs, uint32_t n_recs, uint64_t n_cig, uint64_t seq_bytes, const char *who);
} // namespace np2h
