#pragma once
// Internal declarations shared by the units of the polish driver: np2_polish.cpp (the per-pass pipeline of one contig),
// np2_final.cpp (its final pass and the result), np2_vote.cpp (the device half of the phasing vote) and np2_shard.cpp (the
// shards of one contig).  What only one of them uses is defined there.
#include "np2_ctx.hpp"
#include "np2_vote_host.hpp"

#include <functional>
#include <string>
#include <vector>

namespace np2h {

struct PassCounts {
    uint32_t n_reg = 0, NC = 0, SB = 0, M = 0;
    uint32_t grow = 0; // upper bound of the consensus growth of one splice round (sum of the longest kept candidates)
    // NC / SB / grow are produced on the device (scal S_NC / S_SB / S_GROW) and picked up by the next read-back that
    // happens anyway; until then buffers and launches use the bounds below
    bool known = false;
    uint32_t NC_cap = 0; // 60 candidates per region
    uint32_t SB_cap = 0; // candidate strings are disjoint pieces of the reads: at most the pileup's columns
    void resolve(const std::vector<uint32_t> &sc) {
        NC = sc[S_NC], SB = sc[S_SB], grow = sc[S_GROW];
        known = true;
    }
};

inline RegionTables region_tables(np2_ctx *cx, uint32_t n_reg) {
    return RegionTables{cx->cand_off.p, cx->cand_order.p, cx->kscore.p, cx->cand_seq_off.p, cx->cand_seq.p, n_reg};
}

// the final pass ran its splice rounds with a guessed growth allowance that turned out too small (nothing was written
// out of bounds: k_splice_plan): run_final_pass repeats the pass with the exact one
// ... or its recheck rounds went by the region list and a list, job count or string size outgrew its capacity (again
// nothing out of bounds, the round spliced nothing: k_rech_prepare): repeated with the general recheck kernels
struct GrowRetry : Np2Error {
    bool grow, rech_cap;
    GrowRetry(bool g, bool r) : Np2Error(NP2_E_DEVICE, g ? "internal: guessed growth allowance too small" : "internal: recheck region list too small"), grow(g), rech_cap(r) {}
};
void check_region_err(uint32_t e); // the error word of the region kernels (scal S_ERR) -> the exception it stands for

// stage traces (a tracing context): a consensus, the candidate tables as the oracle traces them ("cand" / "hete": every
// candidate; "seed" / "rechN": kept lists)
struct Cns {
    std::vector<uint32_t> pos;
    std::vector<uint8_t> base;
};
void trace_cns(np2_ctx *cx, int pass, const std::string &tag, const Cns &c);
void trace_region_tables(np2_ctx *cx, int pass, const std::string &tag, const PassCounts &pc, bool kept_view);

// consensus double buffer: cns_pos/cns_base (A) <-> cns_pos2/cns_base2 (B).  The length lives on the device
// (M_p); the host only carries an upper bound (M_cap) to size launches and buffers.
struct CnsDev {
    uint32_t *pos;
    uint8_t *base;
    const uint32_t *M_p;
    uint32_t M_cap;
};

struct ResultOut {
    uint8_t *bases = nullptr;
    uint32_t *pos = nullptr;
    uint64_t len = 0;
    bool want_pos = true;
    bool want_bases = true; // false: the sequence stays on the device (np2_last_result_device / np2_result_fetch_begin)
    void release() { // the pinned result blocks go back to the pool (a result that is not handed to the caller)
        if (bases) pinned_pool().put(bases), bases = nullptr;
        if (pos) pinned_pool().put(pos), pos = nullptr;
    }
};

// The per-contig loop (main.rs:1819-1836) as a stepper: begin (dense pass), then for every pass either
// vote_pass + apply_losers (a phasing pass) or final_pass.  np2_polish_resident drives it straight through; the shards
// of one contig (np2_shard_*) stop after vote_pass, exchange their votes, and continue with the contig-wide losers.
struct PolishRun {
    np2_ctx *cx = nullptr;
    np2_contig *c = nullptr;
    np2_opts_t o{};
    uint32_t own_lo = 0, own_hi = 0xFFFFFFFFu; // regions this run votes over (sub-contig coordinates)
    uint32_t T = 0, pass = 0, M = 0, n_reg = 0;
    bool reuse = false;
    bool front_issued = false; // graph, DP, consensus and LQ regions of pass `pass` are already on their way (polish_impl)
    uint32_t grow_prev = 0xFFFFFFFFu; // growth bound of the previous (phasing) pass, read back with its vote for free
    bool wide_votes = false; // the shards of a contig export (a << 32 | b, counts) pairs; the plain pipeline reads the graph's finished rows
    uint64_t key_add = 0;    // ... with the shard's read-number shift added on the device (s << 32 | s)
    PassCounts pc;
    bool final_pass() const { return pass + 1 == o.iter_count; }
};

void run_begin(PolishRun &r);
void run_pass_front(PolishRun &r);
void run_vote_pass(PolishRun &r, VoteData &vd, const std::function<void()> *after_front = nullptr);
void run_apply_losers(PolishRun &r, const std::vector<uint32_t> &losers);
void run_final_pass(PolishRun &r, ResultOut &result, bool exact_grow = false, bool rech_general = false);
// The early start of the next pass and its settlement: see polish_impl (np2_polish.cpp)
size_t run_start_on_flagged(PolishRun &r, const VoteData &vd);
bool run_settle_flagged(PolishRun &r, const std::vector<uint8_t> &flagged, size_t n_flagged, const std::vector<uint32_t> &losers);
void polish_impl(np2_ctx *cx, np2_contig *c, const np2_opts_t *o, ResultOut &result);

// the device half of the vote (np2_vote.cpp)
void vote_collect(np2_ctx *cx, np2_contig *c, PassCounts &pc, bool asref, bool use_all, int pass, uint32_t own_lo,
                  uint32_t own_hi, VoteData &vd, bool wide = false, uint64_t key_add = 0);

} // namespace np2h
