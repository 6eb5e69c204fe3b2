// The final pass of a contig and its result: seed, the splice rounds (update_consensus_with_lqseqs), the recheck rounds per
// k-mer table (reupdate_consensus_with_lqseqs), the read-back of the polished sequence, and the C ABI that hands the
// result out (include/np2.h: np2_result_fetch_*, np2_last_span, np2_last_result_device).
#include "np2_polish.hpp"

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

using namespace np2;

namespace {

static const uint8_t LB_SUCC = 0x80, LB_RECH = 0x20; // main.rs:655-658

// update_consensus_with_lqseqs on the device; returns the new consensus (in the other buffer).  No read-back: the
// new length is chained on the device into cx->mlen[version].
// the buffers of a splice round: the plan of up to n_slots applied regions, the other half of the consensus double buffer
CnsDev splice_buffers(np2_ctx *cx, const CnsDev &in, uint32_t n_slots, uint32_t grow_bound, bool to_b, uint32_t version) {
    cx->sp_idx_s.ensure(n_slots + 2);
    cx->sp_idx_e.ensure(n_slots + 2);
    cx->ap_g.ensure(n_slots + 2);
    cx->ap_s.ensure(n_slots + 2);
    cx->ap_e.ensure(n_slots + 2);
    cx->ap_delta.ensure(n_slots + 2);
    cx->ap_shift.ensure(n_slots + 2);
    cx->mlen.ensure(16);
    const uint32_t out_cap = in.M_cap + grow_bound;
    const size_t cap = (size_t)out_cap + 64;
    uint32_t *opos = to_b ? cx->cns_pos2.ensure(cap) : cx->cns_pos.ensure(cap);
    uint8_t *obase = to_b ? cx->cns_base2.ensure(cap) : cx->cns_base.ensure(cap);
    return CnsDev{opos, obase, cx->mlen.p + version, out_cap};
}
CnsDev splice_gpu(np2_ctx *cx, const CnsDev &in, uint32_t n_reg, uint8_t lable, uint32_t grow_bound, bool to_b,
                  uint32_t version) {
    hipStream_t s = cx->stream;
    EventTimer t(cx, "splice");
    const CnsDev out = splice_buffers(cx, in, n_reg, grow_bound, to_b, version);
    uint32_t *const opos = out.pos;
    uint8_t *const obase = out.base;
    const uint32_t out_cap = out.M_cap;
    // per-round counters (stuck, n_ap) live behind the posted scalar block; run_diff zeroes them once per contig
    uint32_t *const stuck_p = cx->scal.p + S_COUNT + 2 * version, *const nap_p = stuck_p + 1;
    launch_splice_find(s, in.pos, in.M_p, cx->lq_start.p, cx->lq_end.p, cx->reg_lable.p, lable, n_reg, cx->sp_idx_s.p,
                       cx->sp_idx_e.p, stuck_p);
    launch_splice_plan(s, next_lookback(cx, region_lb_blocks(n_reg)), cx->reg_lable.p, lable, n_reg, stuck_p,
                       cx->sp_idx_s.p, cx->sp_idx_e.p, cx->seed_cand.p, cx->cand_seq_off.p, cx->ap_g.p, cx->ap_s.p,
                       cx->ap_e.p, cx->ap_delta.p, cx->ap_shift.p, nap_p, in.M_p, cx->mlen.p + version, out_cap,
                       cx->scal.p + S_ERR);
    launch_splice_write(s, in.pos, in.base, in.M_p, in.M_cap, cx->ap_g.p, cx->ap_s.p, cx->ap_e.p, cx->ap_delta.p,
                        cx->ap_shift.p, nap_p, n_reg, cx->lq_start.p, cx->seed_cand.p, cx->cand_seq_off.p,
                        cx->cand_seq.p, opos, obase);
    return out;
}

Cns fetch_cns_dev(np2_ctx *cx, const CnsDev &c) { // trace only
    Cns r;
    const uint32_t M = d2h(cx, c.M_p, 1)[0];
    r.pos = d2h(cx, c.pos, M);
    r.base = d2h(cx, c.base, M);
    return r;
}

// The recheck rounds of a final pass from the list of its RECH regions (np2_regions.hip: k_rech_prepare): may this
// contig take it?  Decided from what the host knows without a read-back; every contig that takes it issues the same
// five kernels per table, so the batch driver merges them.
bool rech_by_list(const np2_ctx *cx, uint32_t n_reg) {
    return !cx->trace && !cx->hooks.rech_general && n_reg <= RL_NREG_MAX;
}
uint32_t rech_list_cap(const np2_ctx *cx) { return std::min(cx->hooks.rech_cap_list, RL_CAP_LIST); }
// the list round y reads / the one it leaves for round y + 1, and their counts
uint32_t *rech_list_of(np2_ctx *cx, size_t y) { return cx->rl_list.p + (y & 1) * RL_CAP_LIST; }
uint32_t *rech_list_cnt(np2_ctx *cx, size_t y) { return cx->scal.p + S_RL + (y & 1); }

CnsDev recheck_list_gpu(np2_ctx *cx, const CnsDev &in, const PassCounts &pc, int yak_idx, uint16_t min_kmer_count,
                        bool first_yak, bool last_yak, bool to_b, uint32_t version) {
    hipStream_t s = cx->stream;
    EventTimer t(cx, "recheck");
    const uint32_t ksize = cx->yaks[yak_idx].k;
    const uint32_t cap_jobs = std::min(cx->hooks.rech_cap_jobs, RL_CAP_JOBS), cap_blob = std::min(cx->hooks.rech_cap_blob, RL_CAP_BLOB);
    cx->rech.ensure(RL_CAP_LIST + 2);
    cx->rech_groups.ensure((size_t)(RL_CAP_LIST + 2) * rech_group_bytes());
    cx->rech_groups_tmp.ensure((size_t)(RL_CAP_LIST + 2) * rech_group_bytes());
    cx->rech_joboff.ensure(RL_CAP_LIST + 2);
    cx->rl_blob_off.ensure(RL_CAP_LIST + 2);
    cx->rl_glen.ensure(RL_CAP_LIST + 2);
    cx->rl_job_ol.ensure(RL_CAP_JOBS + 2);
    cx->sstr.ensure((size_t)RL_CAP_BLOB + 64);
    cx->sscore.ensure(RL_CAP_JOBS + 2);
    const CnsDev out = splice_buffers(cx, in, std::max(pc.n_reg, RL_CAP_LIST), pc.grow, to_b, version);
    uint32_t *const st = cx->scal.p + S_RL + 2, *const nap_p = cx->scal.p + S_COUNT + 2 * version + 1;
    const RechList rl{rech_list_of(cx, (size_t)yak_idx), rech_list_cnt(cx, (size_t)yak_idx), rech_list_of(cx, (size_t)yak_idx + 1),
                      rech_list_cnt(cx, (size_t)yak_idx + 1), st, cx->rech.p, cx->sp_idx_s.p, cx->sp_idx_e.p, cx->rech_groups.p, cx->rech_groups_tmp.p,
                      cx->rech_joboff.p, cx->rl_blob_off.p, cx->rl_glen.p, cx->rl_job_ol.p, cx->sstr.p,
                      rech_list_cap(cx), cap_jobs, cap_blob};
    launch_rech_prepare(s, rl, in.pos, in.base, in.M_p, cx->lq_start.p, cx->lq_end.p, cx->keep_n.p, ksize, cx->reg_maxlen.p,
                        cx->cand_off.p, cx->keep_list.p, cx->cand_seq_off.p, cx->cand_seq.p, cx->scal.p + S_ERR);
    launch_score_jobs(s, cx->yaks[yak_idx].dev(), cx->sstr.p, cx->rl_job_ol.p, st + RL_NJOBS, min_kmer_count,
                      cx->sscore.p);
    launch_rech_finish(s, rl, cx->sscore.p, cx->keep_ks.p, cx->cand_off.p, cx->keep_n.p, cx->keep_list.p, cx->cand_order.p,
                       first_yak, last_yak, cx->reg_lable.p, cx->seed_cand.p, in.pos, in.M_p, cx->lq_start.p,
                       cx->cand_seq_off.p, cx->ap_g.p, cx->ap_s.p, cx->ap_e.p, cx->ap_delta.p, cx->ap_shift.p, nap_p, cx->mlen.p + version,
                       out.M_cap, cx->scal.p + S_ERR);
    launch_splice_write(s, in.pos, in.base, in.M_p, in.M_cap, cx->ap_g.p, cx->ap_s.p, cx->ap_e.p, cx->ap_delta.p,
                        cx->ap_shift.p, nap_p, RL_CAP_LIST, cx->lq_start.p, cx->seed_cand.p, cx->cand_seq_off.p,
                        cx->cand_seq.p, out.pos, out.base);
    cx->timing.host.push_back({"rech_list", 1.0f}); // (a count, read through np2_last_timings by the tests)
    return out;
}

// reupdate_consensus_with_lqseqs for one yak table, on the device: the general kernels, over all regions
CnsDev recheck_gpu(np2_ctx *cx, const CnsDev &in, const PassCounts &pc, int yak_idx, uint16_t min_kmer_count,
                   bool first_yak, bool to_b, uint32_t version) {
    hipStream_t s = cx->stream;
    const uint32_t n_reg = pc.n_reg, ksize = cx->yaks[yak_idx].k;
    uint32_t n_rech = 0, n_groups = 0, n_jobs = 0;
    uint64_t blob_bound = 0; // upper bound of the recheck strings' bytes (sizes their buffer without a read-back)
    {
        // RECH region list, chain groups and job offsets: two look-back passes, then one read-back
        EventTimer t(cx, "recheck");
        cx->rech.ensure(n_reg + 2);
        cx->rech_groups.ensure((size_t)(n_reg + 2) * rech_group_bytes());
        cx->rech_joboff.ensure(n_reg + 2);
        cx->rech_groups_tmp.ensure((size_t)(n_reg + 2) * rech_group_bytes());
        cx->rech_headjobs.ensure(n_reg + 2);
        launch_rech_list(s, next_lookback(cx, region_lb_blocks(n_reg)), cx->reg_lable.p, n_reg, cx->rech.p, cx->scal.p + S_NRECH,
                         (unsigned long long *)(cx->scal.p + S_M1), cx->scal.p + S_ERR);
        launch_rech_groups(s, next_lookback(cx, region_lb_blocks(n_reg)), cx->rech.p, cx->scal.p + S_NRECH, n_reg, in.pos, in.M_p,
                           cx->lq_start.p, cx->lq_end.p, cx->keep_n.p, ksize, cx->reg_maxlen.p, cx->rech_groups_tmp.p,
                           cx->rech_headjobs.p, cx->rech_groups.p,
                           cx->rech_joboff.p, cx->scal.p + S_NGROUPS,
                           cx->scal.p + S_M0, (unsigned long long *)(cx->scal.p + S_M1), cx->scal.p + S_ERR);
        std::vector<uint32_t> sc = fetch_scal(cx);
        blob_bound = (uint64_t)sc[S_M1] | ((uint64_t)sc[S_M2] << 32);
        check_region_err(sc[S_ERR]);
        n_rech = sc[S_NRECH];
        n_groups = sc[S_NGROUPS];
        n_jobs = sc[S_M0];
        if (cx->hooks.rech_log)
            fprintf(stderr, "np2 recheck, table %d: %u regions, %u RECH, %u groups, %u jobs, %llu string bytes at most\n", yak_idx, n_reg,
                    n_rech, n_groups, n_jobs, (unsigned long long)blob_bound);
    }
    if (n_rech) {
        RechPtrs rp{cx->rech_groups.p, cx->rech_joboff.p, cx->rech.p, cx->cand_off.p, cx->keep_list.p,
                    cx->cand_seq_off.p, cx->cand_seq.p, in.base, n_groups};
        if (n_jobs) {
            EventTimer t(cx, "recheck");
            cx->job_len.ensure(n_jobs + 2);
            cx->job_off32.ensure(n_jobs + 2);
            cx->soff.ensure(n_jobs + 2);
            cx->sscore.ensure(n_jobs + 2);
            cx->tmp.ensure(prim_temp_bytes((size_t)n_jobs + 2));
            launch_rech_job_len(s, rp, n_jobs, cx->job_len.p);
            exclusive_total_n(cx, cx->job_len.p, cx->job_off32.p, n_jobs);
            if (blob_bound >= 0xFFFFFFF0ull) // 32-bit string offsets: let the exact total decide
                blob_bound = fetch_scal(cx, cx->scal.p + S_M0, cx->job_off32.p + n_jobs)[S_M0];
            cx->sstr.ensure((size_t)blob_bound + 64);
            launch_rech_job_build(s, rp, n_jobs, cx->job_off32.p, cx->soff.p, cx->sstr.p);
            launch_score_strings(s, cx->yaks[yak_idx].dev(), cx->sstr.p, cx->soff.p, n_jobs, min_kmer_count,
                                 cx->sscore.p, true);
            launch_rech_apply(s, rp, cx->sscore.p, cx->keep_ks.p);
        }
        EventTimer t(cx, "recheck");
        launch_rech_select(s, cx->rech.p, cx->scal.p + S_NRECH, n_rech, cx->cand_off.p, cx->keep_n.p, cx->keep_list.p,
                           cx->keep_ks.p, cx->cand_order.p, first_yak, cx->reg_lable.p, cx->seed_cand.p);
    }
    CnsDev out = splice_gpu(cx, in, n_reg, LB_RECH, pc.grow, to_b, version);
    launch_rech_relabel(s, cx->reg_lable.p, n_reg);
    return out;
}

// M_cap: what the host knows the length is at most (the device buffers hold that many elements).  The sequence is copied
// out up to that bound in the SAME wait that brings the length back (one device round trip per contig less than
// "length first, then the copy"; the bound exceeds the length by the splice rounds' growth allowance, a few per cent).
void fetch_result(np2_ctx *cx, const uint32_t *dpos, const uint8_t *dbase, const uint32_t *M_p, uint32_t M_cap, ResultOut &r,
                  uint32_t M_likely = 0xFFFFFFFFu) {
    const double t0 = now_ms();
    // final length + the error word of everything that ran without a read-back since the last one
    // (the same post carries the first and the last consensus position: the FASTA header span)
    std::vector<uint32_t> sc;
    // (a second copy of the bases, device to device, at its device-side length: into the caller's sink — np2_batch_set_sink —,
    // done when this call's last wait returns)
    if (cx->sink_dst && cx->sink_cap) launch_copy_len(cx->stream, cx->sink_dst, dbase, M_p, 1, cx->sink_cap);
    if (r.want_bases || r.want_pos) {
        const uint32_t seq = ++cx->mbox_seq;
        launch_post(cx->stream, cx->scal.p, S_COUNT, cx->mbox_dev, seq, cx->scal.p + S_M0, M_p, nullptr, nullptr, nullptr, nullptr,
                    nullptr, nullptr, dpos, cx->scal.p + S_M1);
        if (r.want_bases) r.bases = (uint8_t *)pinned_pool().get((size_t)M_cap + 1);
        if (r.want_pos) r.pos = (uint32_t *)pinned_pool().get(((size_t)M_cap + 1) * 4);
        if ((r.want_bases && !r.bases) || (r.want_pos && !r.pos)) throw Np2Error(NP2_E_NOMEM, "pinned result allocation failed");
        // (M_likely: a tighter guess of the length — every splice round reserves the full growth allowance, a region
        // is spliced in one of them —; should the sequence be longer after all, its rest follows in a second copy)
        // (under the batch driver the copy kernel reads the length on the device and moves exactly that)
        uint32_t first = std::min(M_cap, M_likely);
        const bool exact_b = r.want_bases && op_d2h_len(cx, r.bases, dbase, M_p, 1, M_cap);
        const bool exact_p = r.want_pos && op_d2h_len(cx, r.pos, dpos, M_p, 4, (size_t)M_cap * 4);
        if (r.want_bases && !exact_b) op_d2h(cx, r.bases, dbase, first);
        if (r.want_pos && !exact_p) op_d2h(cx, r.pos, dpos, (size_t)first * 4);
        if ((exact_b || !r.want_bases) && (exact_p || !r.want_pos)) first = M_cap; // (nothing left for a second copy)
        op_sync(cx);
        if (__atomic_load_n(&cx->mbox_host[0], __ATOMIC_ACQUIRE) != seq)
            throw Np2Error(NP2_E_DEVICE, "mailbox not posted after a synchronisation");
        sc.assign(cx->mbox_host + 1, cx->mbox_host + 1 + S_COUNT);
        if (sc[S_M0] > first && sc[S_M0] <= M_cap) {
            const uint32_t rest = sc[S_M0] - first;
            if (r.want_bases) op_d2h(cx, r.bases + first, dbase + first, rest);
            if (r.want_pos) op_d2h(cx, r.pos + first, dpos + first, (size_t)rest * 4);
            op_sync(cx);
        }
    } else {
        sc = fetch_scal(cx, cx->scal.p + S_M0, M_p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, dpos, cx->scal.p + S_M1);
    }
    check_region_err(sc[S_ERR]);
    const uint32_t M = sc[S_M0];
    if (M == 0) throw Np2Error(NP2_E_REFPANIC, "reference would panic: empty consensus");
    if (M > M_cap) throw Np2Error(NP2_E_DEVICE, "internal: consensus longer than its bound");
    r.len = M;
    cx->last_first_pos = sc[S_M1];
    cx->last_last_pos = sc[S_M2];
    cx->last_dbase = dbase;
    cx->last_dpos = dpos;
    cx->last_len = M;
    if (cx->stage_timing) cx->timing.host.push_back({"wall_fetch_result", (float)(now_ms() - t0)});
}


} // namespace

namespace np2h {

void run_final_pass(PolishRun &r, ResultOut &result, bool exact_grow, bool rech_general) {
    np2_ctx *cx = r.cx;
    np2_contig *c = r.c;
    hipStream_t s = cx->stream;
    run_pass_front(r);
    const uint32_t n_reg = r.n_reg;
    if (n_reg == 0) {
        fetch_result(cx, cx->cns_pos.p, cx->cns_base.p, cx->eoff.p + c->L, r.M, result);
        return;
    }
    PassCounts &pc = r.pc;
    WallTimer w(cx, "wall_final");
    RegionTables rt = region_tables(cx, n_reg);
    cx->reg_lable.ensure(n_reg + 2);
    cx->seed_cand.ensure(n_reg + 2);
    cx->keep_n.ensure(n_reg + 2);
    // The splice rounds need an allowance for the consensus' growth (the sum of the regions' longest kept candidates, on
    // the device: S_GROW).  Reading it back is a device round trip of its own; after a phasing pass its value there is
    // known — the final pass has fewer reads and mostly fewer regions — so twice that, guarded on the device, is used
    // instead, and the pass is repeated with the exact figure should a round outgrow it (never observed).
    const bool no_guess = cx->hooks.exact_grow;
    bool guessed = false;
    if (!pc.known) {
        if (r.grow_prev != 0xFFFFFFFFu && !exact_grow && !no_guess && !cx->trace && (uint64_t)r.grow_prev * 2 + 4096 < 0x7FFFFFFFull) {
            pc.grow = r.grow_prev * 2 + 4096;
            if (cx->hooks.has_grow_guess) pc.grow = cx->hooks.grow_guess; // test hook: force the retry
            guessed = true;
        } else {
            pc.resolve(fetch_scal(cx));
        }
    }
    // the recheck rounds go by the list of the RECH regions, which k_seed writes, unless the contig is too large for it, the
    // stage traces want the per-stage tables, or the list overflowed in this pass's first attempt
    const bool by_list = !rech_general && !cx->yaks.empty() && rech_by_list(cx, n_reg);
    try {
        cx->keep_list.ensure((size_t)pc.NC_cap + 2);
        cx->keep_ks.ensure((size_t)pc.NC_cap + 2);
        if (by_list) cx->rl_list.ensure(2 * (size_t)RL_CAP_LIST);
        {
            EventTimer t(cx, "seed");
            // (the first list's count is zero here: run_diff cleared it with the scalar block, k_rech_finish and the retry below
            // leave it cleared)
            launch_seed(s, rt, r.o.max_indel_len, cx->reg_lable.p, cx->seed_cand.p, cx->keep_n.p, cx->keep_list.p,
                        cx->keep_ks.p, cx->scal.p + S_ERR, by_list ? rech_list_of(cx, 0) : nullptr,
                        by_list ? rech_list_cnt(cx, 0) : nullptr, rech_list_cap(cx));
        }
        if (cx->trace) check_region_err(d2h(cx, cx->scal.p + S_ERR, 1)[0]);
        trace_region_tables(cx, (int)r.pass, "seed", pc, true);
        CnsDev cur{cx->cns_pos.p, cx->cns_base.p, cx->eoff.p + c->L, r.M}; // eoff[L] = length of the raw consensus
        bool to_b = true;
        uint32_t version = 0;
        cur = splice_gpu(cx, cur, n_reg, LB_SUCC, pc.grow, to_b, version++);
        to_b = !to_b;
        if (cx->trace) trace_cns(cx, (int)r.pass, "cns_succ", fetch_cns_dev(cx, cur));
        for (size_t y = 0; y < cx->yaks.size(); ++y) {
            cur = by_list ? recheck_list_gpu(cx, cur, pc, (int)y, r.o.min_kmer_count, y == 0, y + 1 == cx->yaks.size(), to_b, version++)
                          : recheck_gpu(cx, cur, pc, (int)y, r.o.min_kmer_count, y == 0, to_b, version++);
            to_b = !to_b;
            trace_region_tables(cx, (int)r.pass, "rech" + std::to_string(y), pc, true);
            if (cx->trace) trace_cns(cx, (int)r.pass, "cns_rech" + std::to_string(y), fetch_cns_dev(cx, cur));
        }
        fetch_result(cx, cur.pos, cur.base, cur.M_p, cur.M_cap, result, guessed ? r.M + r.grow_prev : r.M + pc.grow);
    } catch (const GrowRetry &g) {
        if ((g.grow && !guessed) || (g.rech_cap && !by_list)) throw;
        result.release();
        op_fill(cx, cx->scal.p + S_ERR, 0, 4); // (every other bit of the word would have been reported first)
        // (the rounds' counters and the region lists' start over with the pass)
        op_fill(cx, cx->scal.p + S_COUNT, 0, (size_t)(SCAL_TOTAL - S_COUNT) * 4);
        if (g.rech_cap) cx->timing.host.push_back({"rech_redo", 1.0f}); // (a count, read through np2_last_timings by the tests)
        r.reuse = false;
        run_final_pass(r, result, exact_grow || g.grow, rech_general || g.rech_cap);
    }
}

} // namespace np2h

extern "C" {

int np2_result_fetch_begin(np2_ctx_t *cx) {
    if (!cx || !cx->last_dbase || cx->out_pending) return NP2_E_ARG;
    return abi_guard([&] {
        HIPCHK(hipSetDevice(cx->device));
        const size_t n = cx->last_len;
        cx->out_snap.ensure(n + 1);
        uint8_t *&host = cx->out_host[cx->out_slot];
        if (cx->out_host_cap[cx->out_slot] < n + 1) {
            if (host) pinned_pool().put(host);
            host = nullptr;
            cx->out_host_cap[cx->out_slot] = 0;
            const size_t cap = n + n / 8 + 4096;
            host = (uint8_t *)pinned_pool().get(cap);
            if (!host) throw Np2Error(NP2_E_NOMEM, "pinned result allocation failed");
            cx->out_host_cap[cx->out_slot] = cap;
        }
        // snapshot on the main stream (in order before the next contig overwrites the consensus buffers), host copy on
        // the output stream behind it
        HIPCHK(hipMemcpyAsync(cx->out_snap.p, cx->last_dbase, n, hipMemcpyDeviceToDevice, cx->stream));
        HIPCHK(hipEventRecord(cx->ev_out, cx->stream));
        HIPCHK(hipStreamWaitEvent(cx->stream_out, cx->ev_out, 0));
        HIPCHK(hipMemcpyAsync(host, cx->out_snap.p, n, hipMemcpyDeviceToHost, cx->stream_out));
        cx->out_len = n;
        cx->out_pending = true;
        return NP2_OK;
    }, ctx_sink(cx));
}

int np2_result_fetch_end(np2_ctx_t *cx, const uint8_t **bases, uint64_t *len) {
    if (!cx || !bases || !len || !cx->out_pending) return NP2_E_ARG;
    return abi_guard([&] {
        HIPCHK(hipStreamSynchronize(cx->stream_out));
        *bases = cx->out_host[cx->out_slot];
        *len = cx->out_len;
        cx->out_slot ^= 1;
        cx->out_pending = false;
        return NP2_OK;
    }, ctx_sink(cx));
}

int np2_last_span(np2_ctx_t *cx, uint32_t *first_pos, uint32_t *last_pos) {
    if (!cx || !first_pos || !last_pos) return NP2_E_ARG;
    *first_pos = cx->last_first_pos;
    *last_pos = cx->last_last_pos;
    return NP2_OK;
}

int np2_last_result_device(np2_ctx_t *cx, const uint8_t **dev_bases, uint64_t *len) {
    if (!cx || !dev_bases || !len) return NP2_E_ARG;
    if (!cx->last_dbase) return NP2_E_ARG;
    *dev_bases = cx->last_dbase;
    *len = cx->last_len;
    return NP2_OK;
}

} // extern "C"
