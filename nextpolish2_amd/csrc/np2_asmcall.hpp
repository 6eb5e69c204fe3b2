// Launchers of the assembly-to-reference caller's kernels (np2_asmcall.hip); their driver is np2_asmcall_host.cpp.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "np2_asmcall_core.hpp"
#include "np2_depth.hpp"

namespace np2 {

// counters of one call, zeroed by the caller before the first launch
struct AsmDev {
    unsigned long long found[3], kept[3], ins_bases, del_bases;
    uint32_t n_runs, n_kept;
    uint32_t err, pad; // LB_ERR: a look-back wait gave up; AC_ERR_*: below
};
static constexpr uint32_t AC_ERR_RANGE = 1u, AC_ERR_EVENTS = 2u, AC_ERR_RUNS = 4u; // an interval beyond the references; more events / runs than room

// A wavefront per admitted alignment adm[i] (n_adm of them, ascending), 64 CIGAR words a step and 64 columns a step.
// vars == nullptr, the count pass: ev_cnt[i] = its events, +1 / -1 of its covered interval into diff (G + 1 zeroed words, G =
// ref_off[n_refs]), ctr->found.  Else the emit pass: ev_cnt holds the inclusive sums of the counts; the events go to vars / keys
// from ev_cnt[i - 1] on in CIGAR order (room for ev_cap).
void launch_asmcall_walk(hipStream_t s, const np2_asmaln_t *alns, const uint32_t *adm, uint32_t n_adm, const uint32_t *cigar, const uint8_t *query,
                         const uint8_t *refs, const uint64_t *ref_off, uint32_t G, uint32_t *diff, uint32_t *ev_cnt, uint64_t *keys, np2_asmvar_t *vars,
                         uint32_t ev_cap, AsmDev *ctr);
// ones[i] = cov[i] == 1, i < G (scanned afterwards by launch_depth_scan)
void launch_asmcall_ones(hipStream_t s, const uint32_t *cov, uint32_t G, uint32_t *ones);
// the maximal runs of cov == 1 inside each reference, in order (room for max_runs), ctr->n_runs; lb: depth_blocks(G) blocks
void launch_asmcall_runs(hipStream_t s, const Lookback &lb, const uint32_t *cov, uint32_t G, const uint64_t *ref_off, uint32_t n_refs,
                         np2_asmrun_t *runs, uint32_t max_runs, AsmDev *ctr);
// the events whose footprint has cov == 1 throughout, in order: kept_keys[r], kept_idx[r] (the event's index); ctr->n_kept, kept,
// ins_bases, del_bases; lb: depth_blocks(n_ev) blocks
void launch_asmcall_filter(hipStream_t s, const Lookback &lb, const uint64_t *keys, const np2_asmvar_t *vars, uint32_t n_ev, const uint32_t *cov,
                           const uint32_t *ones, const uint64_t *ref_off, uint64_t *kept_keys, uint64_t *kept_idx, AsmDev *ctr);
// out[i] = vars[idx[i]]
void launch_asmcall_gather(hipStream_t s, const np2_asmvar_t *vars, const uint64_t *idx, uint32_t n, np2_asmvar_t *out);

} // namespace np2
