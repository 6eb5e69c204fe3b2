// The per-contig polish pipeline of the MI355X NextPolish2 hot path: the kernel orchestration of a pass up to its
// candidates, the stepper the plain driver and the shards of a contig go through (the final pass: np2_final.cpp), the early
// start of the next pass beside the vote's decision, and the C ABI np2_polish_* (include/np2.h).  Replaces the per-contig
// loop src/main.rs:1819-1836 of the reference.  No CPU fallback: every entry point needs a HIP device.
#include "np2_polish.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <future>
#include <memory>
#include <string>
#include <vector>

using namespace np2;

namespace np2h {
void check_region_err(uint32_t e) {
    if (e & 4u) throw Np2Error(NP2_E_REFPANIC, "reference would panic: seq2 order is equal to 0");
    if (e & 8u) throw Np2Error(NP2_E_REFPANIC, "reference would panic: index out of bounds: lqseq.seqs[max1_p]");
    if (e & 16u) throw Np2Error(NP2_E_REFPANIC, "reference would panic: the first lqseq is not ref.");
    if (e & 32u) throw Np2Error(NP2_E_REFPANIC, "reference would panic: lqseq.seqs[0] after retain_sort_seqs");
    if (e & 64u) throw Np2Error(NP2_E_REFPANIC, "reference would panic: consensus index out of bounds in reupdate");
    if (e & 128u) throw Np2Error(NP2_E_NOMEM, "cartesian product of chained LQ regions is too large");
    if (e & LB_ERR) throw Np2Error(NP2_E_DEVICE, "device-wide scan timed out waiting for a predecessor block");
    if (e & (GROW_ERR | RECH_CAP_ERR)) throw GrowRetry((e & GROW_ERR) != 0, (e & RECH_CAP_ERR) != 0);
    if (e & LQ_LIST_ERR) throw Np2Error(NP2_E_DEVICE, "internal: more low-quality bases than their list was sized for");
}

void trace_cns(np2_ctx *cx, int pass, const std::string &tag, const Cns &c) {
    trace_put(cx, pass, tag + ".pos", c.pos);
    trace_put(cx, pass, tag + ".base", c.base);
}

// candidate tables as the oracle traces them ("cand" / "hete": every candidate; "seed" / "rechN": kept lists)
void trace_region_tables(np2_ctx *cx, int pass, const std::string &tag, const PassCounts &pc, bool kept_view) {
    if (!cx->trace) return;
    const uint32_t n_reg = pc.n_reg;
    auto start = d2h(cx, cx->lq_start.p, n_reg), end = d2h(cx, cx->lq_end.p, n_reg);
    auto coff = d2h(cx, cx->cand_off.p, (size_t)n_reg + 1);
    auto order = d2h(cx, cx->cand_order.p, pc.NC);
    auto ks = d2h(cx, cx->kscore.p, pc.NC);
    auto soff = d2h(cx, cx->cand_seq_off.p, (size_t)pc.NC + 1);
    auto pool = d2h(cx, cx->cand_seq.p, pc.SB);
    std::vector<uint8_t> lable(n_reg, 0);
    std::vector<uint32_t> seedc, keepn, keepl;
    std::vector<uint16_t> keepks;
    if (tag != "cand") lable = d2h(cx, cx->reg_lable.p, n_reg);
    if (kept_view) {
        seedc = d2h(cx, cx->seed_cand.p, n_reg);
        keepn = d2h(cx, cx->keep_n.p, n_reg);
        keepl = d2h(cx, cx->keep_list.p, pc.NC);
        keepks = d2h(cx, cx->keep_ks.p, pc.NC);
    }
    std::vector<uint32_t> o_coff(1, 0), o_order, o_soff(1, 0), sudo_off(1, 0);
    std::vector<uint16_t> o_ks;
    std::vector<uint8_t> o_seq, sudo;
    for (uint32_t g = 0; g < n_reg; ++g) {
        if (kept_view) {
            const uint32_t c = seedc[g];
            if (c != 0xFFFFFFFFu) sudo.insert(sudo.end(), pool.begin() + soff[c], pool.begin() + soff[c + 1]);
            for (uint32_t t = 0; t < keepn[g]; ++t) {
                const uint32_t ci = keepl[coff[g] + t];
                o_order.push_back(order[ci]);
                o_ks.push_back(keepks[coff[g] + t]);
                o_seq.insert(o_seq.end(), pool.begin() + soff[ci], pool.begin() + soff[ci + 1]);
                o_soff.push_back((uint32_t)o_seq.size());
            }
        } else {
            for (uint32_t ci = coff[g]; ci < coff[g + 1]; ++ci) {
                o_order.push_back(order[ci]);
                o_ks.push_back(ks[ci]);
                o_seq.insert(o_seq.end(), pool.begin() + soff[ci], pool.begin() + soff[ci + 1]);
                o_soff.push_back((uint32_t)o_seq.size());
            }
        }
        sudo_off.push_back((uint32_t)sudo.size());
        o_coff.push_back((uint32_t)o_order.size());
    }
    trace_put(cx, pass, tag + ".start", start);
    trace_put(cx, pass, tag + ".end", end);
    trace_put(cx, pass, tag + ".lable", lable);
    trace_put(cx, pass, tag + ".sudo_off", sudo_off);
    trace_put(cx, pass, tag + ".sudo", sudo);
    trace_put(cx, pass, tag + ".cand_off", o_coff);
    trace_put(cx, pass, tag + ".order", o_order);
    trace_put(cx, pass, tag + ".kscore", o_ks);
    trace_put(cx, pass, tag + ".seq_off", o_soff);
    trace_put(cx, pass, tag + ".seq", o_seq);
    if (tag == "cand") trace_put(cx, pass, "cand.kmer", d2h(cx, cx->cand_kmer.p, pc.NC));
}

} // namespace np2h

namespace {

// ------------------------------------------------------------------------------------------
// the per-contig pipeline
// ------------------------------------------------------------------------------------------
// Dense pass + exception sort.  Afterwards the sorted (node key, read) records of contig tile t are
// keys_raw / vals_raw [a, a + tile_n[t]) with a = t * cx->bucket_cap (bucketed layout, the normal case) or
// a = tile_scan[t] when cx->bucket_cap == 0 (compact layout after the device-wide sort).
void run_diff(np2_ctx *cx, np2_contig *c, uint32_t &T) {
    hipStream_t s = cx->stream;
    const uint32_t L = c->L, R = c->R, NCH = c->n_chunks;
    const uint32_t n_tiles = (L + TILE - 1) >> TILE_SHIFT;
    const uint32_t bcap = std::min(cx->tile_cap, c->tile_cap); // (cx: the NP2_TILE_CAP test hook)
    const uint64_t buckets = (uint64_t)n_tiles * bcap;
    uint64_t ovf_cap = std::max<uint64_t>(c->n_cols / 256 + 65536, 1u << 18); // spill area of full buckets
    cx->tmp.ensure(prim_temp_bytes(std::max<size_t>((size_t)NCH + 2, (size_t)L + 2)));
    cx->tile_n.ensure(n_tiles + 2);
    cx->tile_scan.ensure(n_tiles + 2);
    cx->tile_scanb.ensure(n_tiles + 2);
    cx->tile_nn.ensure(n_tiles + 2);
    cx->tile_nr.ensure(n_tiles + 2);
    cx->tile_noff.ensure(n_tiles + 2);
    cx->tile_roff.ensure(n_tiles + 2);
    cx->tile_gain.ensure(n_tiles + 2);
    if (cx->tile_cur.cap < (size_t)n_tiles + 2) { // the cursors are left zeroed by k_tile_layout; clear new storage
        cx->tile_cur.ensure(n_tiles + 2);
        zero32(cx, cx->tile_cur.p, cx->tile_cur.cap);
    }
    if (cx->chunk_st.cap < (size_t)NCH + 2) { // status words carry a launch epoch: cleared once, never again
        cx->chunk_st.ensure(NCH + 2);
        zero32(cx, cx->chunk_st.p, cx->chunk_st.cap, 8);
    }
    // chunk counts ahead of the dense pass (launch_chunk_counts): when this process shares the device with another one
    // (NP2_DENSE_PRECOUNT: set by the host side for ranks rehearsing on one GPU), or once a chunk's wait gave up
    static const bool precount_env = getenv("NP2_DENSE_PRECOUNT") != nullptr;
    bool precount = precount_env;
    for (int attempt = 0; attempt < 4; ++attempt) {
        if (ovf_cap >= 0xFFFFFFF0ull) throw Np2Error(NP2_E_NOMEM, "too many exception nodes");
        cx->keys_raw.ensure(buckets + ovf_cap + 1);
        cx->vals_raw.ensure(buckets + ovf_cap + 1);
        zero32(cx, cx->scal.p, SCAL_TOTAL);
        if (++cx->chunk_epoch == 0) ++cx->chunk_epoch; // 0 = never written
        if (precount) launch_chunk_counts(s, c->descs.p, NCH, c->nib.p, cx->chunk_st.p, cx->chunk_epoch);
        {
            EventTimer t(cx, "diff_reads", true);
            launch_diff_reads(s, c->descs.p, NCH, c->nib.p, (const uint64_t *)c->refnib.p, c->refnib.p, c->refnib.p + c->ref_stride, c->ref_stride, L,
                              cx->keys_raw.p, cx->vals_raw.p, cx->tile_cur.p, n_tiles, bcap, buckets, (uint32_t)ovf_cap,
                              cx->scal.p + S_M3, c->ckpt.p, cx->chunk_st.p, cx->chunk_epoch, cx->scal.p + S_ERR);
        }
        {
            EventTimer t(cx, "sort_exceptions");
            // per-tile counts / layouts + the counters the host needs, all in the mailbox: S_M0 = T, S_M1 = largest
            // tile, S_M2 = records spilled from full buckets
            // (contigs of a few thousand tiles and more: a handful of blocks chained by the look-back)
            const bool wide = n_tiles >= 2048;
            Lookback lb{};
            if (wide) lb = next_lookback(cx, tile_scan_blocks(n_tiles));
            launch_tile_layout(s, cx->tile_cur.p, n_tiles, bcap, cx->tile_n.p, cx->tile_scan.p, cx->tile_scanb.p,
                               cx->scal.p + S_M3, cx->scal.p + S_M0, wide ? &lb : nullptr, cx->scal.p + S_ERR);
        }
        std::vector<uint32_t> sc = fetch_scal(cx);
        // (a wait that gave up — in the dense pass or in k_tile_layout — first: what follows it in the kernel is undefined,
        // the descriptor check included)
        static const bool test_fail = getenv("NP2_TEST_DENSE_LB_FAIL") != nullptr; // (test hook: the first attempt "gave up")
        if (test_fail && attempt == 0 && !precount) sc[S_ERR] |= LB_ERR;
        if ((sc[S_ERR] & LB_ERR) && !precount) { // (cursors, scalars and epoch start over with the next attempt)
            precount = true;
            continue;
        }
        if (sc[S_ERR] & ~2u) check_region_err(sc[S_ERR] & ~2u);
        if (sc[S_ERR] & 2u)
            throw Np2Error(NP2_E_ARG, "packed read inconsistent with its descriptor (n_cols / aln_t_e / terminator)");
        if (sc[S_M2] > ovf_cap) { // the spill area itself overflowed: grow and redo the dense pass
            ovf_cap = (uint64_t)sc[S_M2] * 5 / 4 + 65536;
            continue;
        }
        T = sc[S_M0];
        if (T >= 0xFFFFFFF0u) throw Np2Error(NP2_E_NOMEM, "too many exception nodes");
        cx->tmp.ensure(prim_temp_bytes(std::max<size_t>({(size_t)T + 1, (size_t)L + 2, (size_t)R + 1})));
        EventTimer t(cx, "sort_exceptions");
        if (sc[S_M2] == 0) {
            // raw records -> node keys, sorted by (key, read) inside LDS, tile by tile, in place
            cx->tile_pidx.ensure((size_t)n_tiles * (TILE / 16) + 64);
            launch_tile_sort(s, cx->tile_pidx.p, c->reads.p, c->nib.p, cx->tile_n.p, n_tiles, bcap, sc[S_M1], cx->keys_raw.p,
                             cx->vals_raw.p, cx->scal.p + S_ERR);
            cx->bucket_cap = bcap;
            cx->pidx_valid = true;
        } else {
            // some tile holds more records than a bucket (e.g. a long insertion carried by every read): gather
            // buckets + spill area into one array and sort it device-wide
            cx->keys.ensure((size_t)T + 1);
            cx->vals.ensure((size_t)T + 1);
            const uint32_t nb = T - sc[S_M2];
            launch_gather_buckets(s, c->reads.p, c->nib.p, cx->tile_n.p, cx->tile_scanb.p, n_tiles, bcap, cx->keys_raw.p,
                                  cx->vals_raw.p, cx->keys.p, cx->vals.p);
            launch_gather_spill(s, c->reads.p, c->nib.p, cx->keys_raw.p + buckets, cx->vals_raw.p + buckets, sc[S_M2],
                                cx->keys.p + nb, cx->vals.p + nb);
            unsigned pos_bits = 1;
            while ((1ull << pos_bits) < (uint64_t)L + 1) ++pos_bits;
            prim_op(cx, [=](hipStream_t st) {
                if (prim_sort_pairs_u64_u32(st, cx->tmp.p, cx->tmp.cap, cx->keys.p, cx->keys_raw.p, cx->vals.p, cx->vals_raw.p,
                                            T, 32 + pos_bits))
                    throw Np2Error(NP2_E_DEVICE, "rocprim radix_sort_pairs failed");
            });
            cx->bucket_cap = 0;
            cx->pidx_valid = false;
        }
        return;
    }
    throw Np2Error(NP2_E_NOMEM, "exception buffer kept overflowing");
}

void build_graph(np2_ctx *cx, np2_contig *c, uint32_t T, uint32_t &n_nodes, uint32_t &n_runs) {
    hipStream_t s = cx->stream;
    const uint32_t L = c->L;
    const uint32_t n_tiles = (L + TILE - 1) >> TILE_SHIFT;
    EventTimer t(cx, "build_graph");
    cx->npos.ensure(T + 1);
    cx->nbases.ensure(T + 1);
    cx->ndelta.ensure(T + 1);
    cx->ncount.ensure(T + 1);
    cx->nminr.ensure(T + 1);
    cx->nscore.ensure(T + 1);
    cx->nbesti.ensure(T + 1);
    cx->nrec.ensure((size_t)T + 32); // the DP kernels prefetch a fixed number of records per position
    cx->node_off.ensure(L + 16); // k_dp_bt_short reads fixed windows past a run's start
    cx->cov.ensure(L + 16);
    cx->pflag.ensure((size_t)L + TILE + 16); // (k_tile_write stores four flags at a time, up to the end of the last tile)
    cx->run_start.ensure(L + 2);
    cx->run_end.ensure(L + 2);
    cx->emit.ensure(L + 2);
    NodeArrays nd{cx->npos.p, cx->nbases.p, cx->ndelta.p, cx->ncount.p, cx->nminr.p};
    launch_tile_count(s, cx->keys_raw.p, cx->vals_raw.p, cx->tile_n.p, cx->tile_scan.p, cx->bucket_cap, n_tiles,
                      cx->alive.p, cx->tile_nn.p, cx->tile_nr.p);
    // (also resets the per-pass scalars S_BEST .. S_NLQ)
    {
        const bool wide = n_tiles >= 2048;
        Lookback lb{};
        if (wide) lb = next_lookback(cx, tile_scan_blocks(n_tiles));
        launch_tile_offsets(s, cx->tile_nn.p, cx->tile_nr.p, n_tiles, cx->tile_noff.p, cx->tile_roff.p,
                            cx->scal.p + S_NNODES, cx->scal.p + S_NRUNS, cx->scal.p + S_BEST, S_NLQ + 1 - S_BEST,
                            wide ? &lb : nullptr, cx->scal.p + S_ERR);
    }
    launch_tile_write(s, cx->keys_raw.p, cx->vals_raw.p, cx->tile_n.p, cx->tile_scan.p, cx->bucket_cap, cx->tile_noff.p,
                      cx->tile_roff.p, n_tiles, cx->alive.p, L, nd, cx->nrec.p, cx->node_off.p, cx->run_start.p,
                      c->reads.p, c->tile_rd_off.p, c->tile_rd.p, cx->cov.p, c->refnib.p, cx->emit.p,
                      (long long *)cx->tile_gain.p, cx->scal.p + S_DEEP /* reset by launch_tile_offsets above */, cx->deep_min,
                      cx->pflag.p);
    // no read-back: downstream kernels are launched with the bound below and check the device-side counters
    n_runs = std::min<uint32_t>(T, L);
    n_nodes = T;
    if (cx->trace) n_nodes = d2h(cx, cx->scal.p + S_NNODES, 1)[0];
}

GraphPtrs graph_ptrs(np2_ctx *cx, np2_contig *c) {
    NodeArrays nd{cx->npos.p, cx->nbases.p, cx->ndelta.p, cx->ncount.p, cx->nminr.p};
    return GraphPtrs{c->refnib.p, cx->node_off.p, nd, cx->cov.p, c->L, cx->nrec.p, cx->scal.p + S_DEEP, cx->pflag.p};
}

void trace_graph(np2_ctx *cx, np2_contig *c, int pass, uint32_t n_nodes) {
    if (!cx->trace) return;
    const uint32_t L = c->L;
    auto off = d2h(cx, cx->node_off.p, (size_t)L + 1);
    auto nb = d2h(cx, cx->nbases.p, n_nodes);
    auto ndl = d2h(cx, cx->ndelta.p, n_nodes);
    auto nc = d2h(cx, cx->ncount.p, n_nodes);
    auto cov = d2h(cx, cx->cov.p, (size_t)L);
    auto rn = d2h(cx, c->refnib.p, (size_t)(L + 1) / 2);
    auto code = [&](uint32_t p) -> unsigned { return (rn[p >> 1] >> (4 * (p & 1))) & 7; };
    std::vector<uint32_t> goff(L + 1, 0), gcount;
    std::vector<uint16_t> gbases, gdelta;
    for (uint32_t p = 0; p < L; ++p) {
        uint16_t b, d;
        if (p >= 2)
            b = (uint16_t)((code(p - 2) << 8) | (code(p - 1) << 4) | code(p)), d = 0;
        else if (p == 1)
            b = (uint16_t)(0x0F00 | (code(0) << 4) | code(1)), d = 1;
        else
            b = (uint16_t)(0x4FF0 | code(0)), d = 0;
        uint32_t e0 = 0;
        for (uint32_t i = off[p]; i < off[p + 1]; ++i)
            if (node_delta3(nb[i], ndl[i]) == 0) e0 += nc[i];
        gbases.push_back(b);
        gdelta.push_back(d);
        gcount.push_back((uint32_t)cov[p] - e0);
        for (uint32_t i = off[p]; i < off[p + 1]; ++i) {
            gbases.push_back(nb[i]);
            gdelta.push_back(ndl[i]);
            gcount.push_back(nc[i]);
        }
        goff[p + 1] = (uint32_t)gcount.size();
    }
    trace_put(cx, pass, "graph.off", goff);
    trace_put(cx, pass, "graph.bases", gbases);
    trace_put(cx, pass, "graph.delta", gdelta);
    trace_put(cx, pass, "graph.count", gcount);
}

// DP + backtrack + LQ regions; returns consensus length M and region count
// One read-back at the end: consensus length, region count, error word.  The consensus length stays on the device
// (eoff[L]) while the consensus and the LQ regions are built; launches and buffers are sized by M <= L + T.
struct CnsBounds {
    uint32_t M_cap, lq_cap, n_words;
};
CnsBounds cns_buffers(np2_ctx *cx, np2_contig *c, uint32_t n_nodes, uint32_t n_runs, uint32_t T) {
    const uint32_t L = c->L;
    if ((uint64_t)L + T + 2 >= 0xFFFFFFF0ull) throw Np2Error(NP2_E_NOMEM, "consensus bound exceeds 32 bits");
    const uint32_t M_cap = L + T + 2; // a path node emits at most one base; exception nodes <= T
    cx->eoff.ensure(L + 2);
    cx->cns_pos.ensure(M_cap + 2);
    cx->cns_base.ensure(M_cap + 2);
    cx->cns_cls.ensure(M_cap + 2);
    cx->lq_kind.ensure(M_cap + 2);
    cx->lq_next.ensure(M_cap + 2);
    cx->lq_nothead.ensure(M_cap + 2);
    cx->rflag.ensure(M_cap + 2);
    cx->rstart.ensure(M_cap + 2);
    cx->rend.ensure(M_cap + 2);
    cx->ridx.ensure(M_cap + 2);
    cx->raw_start.ensure(M_cap + 2);
    cx->raw_end.ensure(M_cap + 2);
    cx->headflag.ensure(M_cap + 2);
    cx->hidx.ensure(M_cap + 2);
    cx->lq_start.ensure(M_cap + 2);
    cx->lq_end.ensure(M_cap + 2);
    cx->tmp.ensure(prim_temp_bytes((size_t)M_cap + 2));
    // the low-quality bases (they only come out of dirty runs) as a list of consensus indices; a path through a run has
    // at most one entry per dirty position and per exception node
    const uint32_t lq_cap = (uint32_t)std::min<uint64_t>(2ull * n_nodes + n_runs + 2, M_cap);
    const uint32_t n_words = (M_cap + 31) / 32;
    cx->lq_list.ensure((size_t)lq_cap + 2);
    cx->hbits.ensure((size_t)n_words + 2);
    return CnsBounds{M_cap, lq_cap, n_words};
}
// raw LQ regions from the list of low-quality bases (n_lq of them, a device-side count): chain heads marked in a bitmap
// over the emission indices, heads per word scanned, regions written out in bit order (right -> left, the reference's
// numbering), then merged (main.rs:1613-1615)
void lq_regions_issue(np2_ctx *cx, const CnsBounds &b, const uint32_t *M_p, const uint32_t *n_lq) {
    hipStream_t s = cx->stream;
    EventTimer t(cx, "lq_regions");
    // (the head bitmap is cleared by k_lq_scan, its words counted inside the scan, the merge flags formed inside theirs:
    // three launches less per pass than one kernel per step)
    launch_lq_scan(s, cx->cns_pos.p, cx->cns_base.p, cx->cns_cls.p, M_p, cx->lq_list.p, n_lq, b.lq_cap, cx->lq_kind.p,
                   cx->lq_next.p, cx->lq_nothead.p, cx->hbits.p, b.n_words + 1, cx->rstart.p, cx->rend.p);
    launch_scan_lb_popc(s, next_lookback(cx, scan_lb_blocks((size_t)b.n_words + 1)), cx->hbits.p, cx->ridx.p, b.n_words,
                        cx->scal.p + S_ERR);
    launch_scatter_regions(s, cx->hbits.p, b.n_words, cx->ridx.p, cx->rstart.p, cx->rend.p, cx->raw_start.p,
                           cx->raw_end.p, cx->scal.p + S_NRAW);
    launch_lq_merge_scan_lb(s, next_lookback(cx, lq_merge_lb_blocks()), cx->raw_start.p, cx->raw_end.p, cx->scal.p + S_NRAW, b.M_cap,
                            cx->headflag.p, cx->hidx.p, cx->scal.p + S_ERR);
    // (the merged regions written by the single-block scan kernel itself measured slower: 52 + 15 -> 95 us per step)
    launch_lq_merge_write(s, cx->raw_start.p, cx->raw_end.p, cx->scal.p + S_NRAW, cx->headflag.p, cx->hidx.p,
                          cx->lq_start.p, cx->lq_end.p, cx->scal.p + S_NREG);
}

void consensus_and_regions_issue(np2_ctx *cx, np2_contig *c, uint32_t n_nodes, uint32_t n_runs, uint32_t T) {
    hipStream_t s = cx->stream;
    const uint32_t L = c->L;
    const CnsBounds cb = cns_buffers(cx, c, n_nodes, n_runs, T);
    const uint32_t M_cap = cb.M_cap, lq_cap = cb.lq_cap;
    GraphPtrs gp = graph_ptrs(cx, c);
    cx->n0_besti.ensure(L + 2);
    cx->run_gain.ensure((size_t)n_runs + 2);
    cx->run_flag.ensure((size_t)n_runs + 2);
    cx->emit.ensure(L + 2);
    cx->bt_path.ensure((size_t)M_cap + 2);
    cx->lqc.ensure((size_t)n_runs + 4);
    cx->lqoff.ensure((size_t)n_runs + 4);
    const uint32_t *const n_lq = cx->lqoff.p + n_runs; // total of the scanned per-run counts (n_runs: host-side bound)
    const uint32_t *M_p = cx->eoff.p + L;
    {
        EventTimer t(cx, "dp_backtrack");
        // (scalars were zeroed by build_graph; S_GAIN already holds the clean-position gains)
        // The short kernel goes first and lists the runs it leaves alone, so that the long-run kernels walk that list
        // instead of classifying every run again.
        cx->dp_list.ensure((size_t)n_runs + 2);
        uint32_t *const dp_list = cx->dp_list.p, *const n_dp_list = cx->scal.p + S_NDPLIST; // (zeroed with the per-pass scalars)
        launch_dp_short(s, gp, c->refnib.p, cx->run_start.p, cx->scal.p + S_NRUNS, n_runs, cx->run_end.p, cx->run_gain.p,
                        cx->emit.p, cx->scal.p + S_PATHBEGIN, cx->bt_path.p, dp_list, n_dp_list);
        launch_dp_long(s, gp, cx->run_start.p, n_runs, cx->nrec.p, cx->nscore.p, cx->nbesti.p, cx->n0_besti.p,
                       cx->run_end.p, (int64_t *)(cx->scal.p + S_LAST0), cx->run_gain.p, cx->emit.p,
                       cx->scal.p + S_PATHBEGIN, cx->bt_path.p, cx->run_flag.p, dp_list, n_dp_list);
        launch_dp_finish(s, gp, cx->run_start.p, cx->scal.p + S_NRUNS, cx->nscore.p, cx->nbesti.p, cx->n0_besti.p,
                         (const int64_t *)(cx->scal.p + S_LAST0), (unsigned long long *)(cx->scal.p + S_GAIN0),
                         cx->scal.p + S_DUP /* block counter: reset with the per-pass scalars */, cx->scal.p + S_BEST,
                         cx->run_gain.p, (const long long *)cx->tile_gain.p,
                         (c->L + TILE - 1) >> TILE_SHIFT, cx->emit.p, cx->scal.p + S_PATHBEGIN, cx->bt_path.p);
        exclusive_total(cx, cx->emit.p, cx->eoff.p, (size_t)L + 1);
        launch_bt_write(s, gp, cx->run_start.p, cx->scal.p + S_NRUNS, n_runs, cx->emit.p, cx->eoff.p, cx->bt_path.p,
                        cx->cns_pos.p, cx->cns_base.p, cx->cns_cls.p, cx->lq_nothead.p, cx->lqc.p);
        exclusive_total(cx, cx->lqc.p, cx->lqoff.p, (size_t)n_runs + 1); // (lqc[n_runs] = 0)
        launch_lq_list(s, gp, cx->run_start.p, cx->scal.p + S_NRUNS, n_runs, cx->emit.p, cx->eoff.p, cx->bt_path.p,
                       cx->lqoff.p, lq_cap, cx->lq_list.p, cx->scal.p + S_ERR);
        launch_default_tail(s, gp, cx->scal.p + S_BEST, M_p, cx->cns_base.p, cx->cns_cls.p, cx->lq_list.p,
                            cx->lqoff.p + n_runs, lq_cap, cx->scal.p + S_ERR);
    }
    lq_regions_issue(cx, cb, M_p, n_lq);
}

// The same stage through the fused pass front (np2_passfront.hip): records of a tile -> the tile's piece of the consensus
// in one kernel, one scan over the per-tile counts, one compaction; no graph arrays in memory.  Needs the bucketed record
// layout with k_tile_sort's position index.  A pass the fused kernels cannot hold (PF_REDO) or whose best path score is
// negative is redone by the kernels above (pass_front_finish).
bool front_can_fuse(np2_ctx *cx) {
    return !cx->hooks.front_unfused && cx->bucket_cap != 0 && cx->pidx_valid;
}
void pass_front_fused_issue(np2_ctx *cx, np2_contig *c, uint32_t T) {
    hipStream_t s = cx->stream;
    const uint32_t L = c->L;
    const uint32_t n_tiles = (L + TILE - 1) >> TILE_SHIFT;
    const CnsBounds cb = cns_buffers(cx, c, T, std::min<uint32_t>(T, L), T);
    cx->pf_slots.ensure(pf_slot_entries(n_tiles, T));
    cx->pf_bad.ensure((size_t)n_tiles + 2);
    cx->pf_bad2.ensure((size_t)n_tiles + 2);
    // (test hooks: lower the LDS variants' limits so that small inputs take the big variant / the unfused redo)
    const np2_ctx::Hooks &hk = cx->hooks;
    const uint32_t cap_lim = hk.has_pf_cap ? hk.pf_cap : PF_CAP, cap_big = hk.has_pf_cap_big ? hk.pf_cap_big : PF_CAP_BIG,
                   halo_lim = (hk.has_pf_halo ? hk.pf_halo : PF_HALO) & ~15u, cov_max = hk.has_pf_cov_max ? hk.pf_cov_max : PF_COV_MAX;
    PfTile a{cx->keys_raw.p, cx->vals_raw.p, cx->tile_n.p, cx->tile_scan.p, cx->tile_pidx.p, cx->alive.p, c->reads.p,
             c->tile_rd_off.p, c->tile_rd.p, c->refnib.p, cx->pf_slots.p, cx->tile_nn.p, cx->tile_nr.p,
             (long long *)cx->tile_gain.p, cx->scal.p + S_PF, cx->scal.p + S_NBAD, cx->pf_bad.p, cx->scal.p + S_NBAD2, cx->pf_bad2.p,
             (long long *)(cx->scal.p + S_PFEND0), (unsigned long long *)(cx->scal.p + S_PFGAIN0), nullptr, L, n_tiles, cx->bucket_cap,
             cap_lim, cap_big, halo_lim, std::min(cov_max, cx->deep_min), cx->pf_big ? 1u : 0u};
    uint32_t *const M_p = cx->eoff.p + L;
    uint32_t *const n_lq = cx->scal.p + S_NRUNS;
    const bool prof = cx->hooks.pf_prof && tl_recorder() == nullptr; // (phase timers of the tile kernel: a tool's switch)
    if (prof) {
        cx->pf_prof.ensure((size_t)n_tiles * 8 + 8);
        zero32(cx, cx->pf_prof.p, (size_t)n_tiles * 8, 8);
        a.prof = (unsigned long long *)cx->pf_prof.p;
    }
    {
        EventTimer t(cx, "pass_front");
        launch_pf_tile(s, a);
        if (prof) {
            auto st = d2h(cx, cx->pf_prof.p, (size_t)n_tiles * 8);
            double sum[8] = {0}, mx[8] = {0};
            size_t cnt = 0;
            for (uint32_t t = 0; t < n_tiles; ++t) {
                const uint64_t *q = st.data() + (size_t)t * 8;
                if (!q[7] || !q[0]) continue; // (a tile the small variant did not finish)
                ++cnt;
                for (int i = 1; i < 8; ++i) {
                    const double d = (double)(q[i] - q[i - 1]);
                    sum[i] += d, mx[i] = std::max(mx[i], d);
                }
            }
            {
                auto tn = d2h(cx, cx->tile_n.p, n_tiles);
                uint32_t h[6] = {0};
                for (uint32_t v : tn) ++h[v <= 480 ? 0 : v <= 960 ? 1 : v <= 1440 ? 2 : v <= 1920 ? 3 : v <= 3584 ? 4 : 5];
                fprintf(stderr, "[pf_prof] records per tile <=480 / 960 / 1440 / 1920 / 3584 / more: %u %u %u %u %u %u; ", h[0], h[1], h[2], h[3], h[4], h[5]);
            }
            fprintf(stderr, "listed for the middle / the big variant: %u / %u; ", d2h(cx, cx->scal.p + S_NBAD, 1)[0], d2h(cx, cx->scal.p + S_NBAD2, 1)[0]);
            fprintf(stderr, "tiles %zu of %u; mean / max clocks per phase (loads, cover+nodes, offsets+sort, DP, reduce, count+scan, write):", cnt, n_tiles);
            for (int i = 1; i < 8; ++i) fprintf(stderr, " %.0f/%.0f", cnt ? sum[i] / cnt : 0.0, mx[i]);
            fprintf(stderr, "\n");
        }
        // consensus offset and low-quality offset of every tile, their totals (consensus length -> eoff[L]), the total of the
        // gains; also resets the per-pass scalars S_BEST .. S_NLQ like the unfused build
        const bool wide = n_tiles >= 2048;
        Lookback lb{};
        if (wide) lb = next_lookback(cx, tile_scan_blocks(n_tiles));
        launch_tile_offsets(s, cx->tile_nn.p, cx->tile_nr.p, n_tiles, cx->tile_noff.p, cx->tile_roff.p, M_p, n_lq,
                            cx->scal.p + S_BEST, S_NLQ + 1 - S_BEST, wide ? &lb : nullptr, cx->scal.p + S_ERR,
                            (const long long *)cx->tile_gain.p, (unsigned long long *)(cx->scal.p + S_PFGAIN0));
        launch_pf_compact(s, n_tiles, cx->pf_slots.p, cx->tile_scan.p, cx->tile_nn.p, cx->tile_noff.p, cx->tile_roff.p,
                          cx->cns_pos.p, cx->cns_base.p, cx->cns_cls.p, cx->lq_nothead.p, cx->lq_list.p, cb.lq_cap,
                          cx->scal.p + S_ERR, cx->scal.p + S_PF, cx->scal.p + S_PFOUT, cx->scal.p + S_NBAD, cx->scal.p + S_NBAD2);
    }
    lq_regions_issue(cx, cb, M_p, n_lq);
}

// graph + consensus + LQ regions of a pass, issued (no wait): fused where possible
void pass_front_issue(np2_ctx *cx, np2_contig *c, uint32_t T, int pass, bool force_unfused = false) {
    cx->front_fused = !force_unfused && front_can_fuse(cx);
    if (!cx->front_fused || cx->trace) { // (stage traces of the graph come from the unfused build)
        uint32_t n_nodes = 0, n_runs = 0;
        {
            WallTimer w(cx, "wall_graph");
            build_graph(cx, c, T, n_nodes, n_runs);
        }
        trace_graph(cx, c, pass, n_nodes);
        if (!cx->front_fused) {
            consensus_and_regions_issue(cx, c, n_nodes, n_runs, T);
            return;
        }
    }
    pass_front_fused_issue(cx, c, T);
}
// ... and the read-back that ends the stage: consensus length, region count, the error word
void consensus_and_regions_finish(np2_ctx *cx, np2_contig *c, uint32_t T, int pass, uint32_t &M, uint32_t &n_reg, bool whole_contig = true) {
    const uint32_t *M_p = cx->eoff.p + c->L;
    std::vector<uint32_t> sc = fetch_scal(cx, cx->scal.p + S_M0, M_p);
    if (cx->front_fused) {
        const int64_t total = (int64_t)(((uint64_t)sc[S_PFGAIN1] << 32) | sc[S_PFGAIN0]);
        const int64_t end_rel = (int64_t)(((uint64_t)sc[S_PFEND1] << 32) | sc[S_PFEND0]);
        const bool negative = end_rel <= SCORE_NEG / 2 || total + end_rel < 0; // main.rs:1651,1680: no end node reaches 0
        if (sc[S_PFOUT] & PF_NEED_BIG) cx->pf_big = true; // (sticky: the next fused pass of this context launches it)
        if ((sc[S_PFOUT] & PF_REDO) || negative) {
            ++cx->front_redos;
            cx->timing.host.push_back({"front_redo", 1.0f}); // (a count, read through np2_last_timings by the tests)
            pass_front_issue(cx, c, T, pass, true);
            sc = fetch_scal(cx, cx->scal.p + S_M0, M_p);
        }
    }
    check_region_err(sc[S_ERR]);
    // No end node at score >= 0: k_dp_finish / k_default_tail have walked back from the reference's default node
    // (main.rs:1651,1680).  Whether the score is negative is a property of the WHOLE contig: a shard cannot tell.
    if (!cx->front_fused && sc[S_BEST] == 0xFFFFFFFFu && !whole_contig)
        throw Np2Error(NP2_E_UNSUPPORTED,
                       "best path score is negative at the end of a shard (the reference's default node is chosen by the whole "
                       "contig's score): polish this contig unsharded");
    M = sc[S_M0];
    if (M == 0) throw Np2Error(NP2_E_REFPANIC, "reference would panic: empty consensus");
    n_reg = sc[S_NRAW] ? sc[S_NREG] : 0;
}

// candidate extraction + first-yak scoring; fills the host RegionSet
void extract_candidates(np2_ctx *cx, np2_contig *c, uint32_t n_reg, uint16_t min_kmer_count, int pass,
                        PassCounts &pc) {
    hipStream_t s = cx->stream;
    const uint32_t R = c->R;
    REFPANIC_IF(cx->yaks.empty(), "index out of bounds: opt.yak[0]");
    if ((uint64_t)n_reg * LQSEQ_MAX_CAN_COUNT >= 0xFFFFFFF0ull) throw Np2Error(NP2_E_NOMEM, "too many LQ regions");
    const uint32_t NC_cap = n_reg * LQSEQ_MAX_CAN_COUNT;
    // candidate strings are disjoint pieces of the reads: at most the pileup's columns.  A chromosome-sized contig does not
    // allocate by that bound (7.7 GB for a 248 Mb contig, 1 % of it used: half a second of the context's first polish) but
    // reads the exact byte count back once the offsets are known — a read-back of its own, ~60 us, which a contig that
    // size does not notice and a yeast-sized batch would
    static const uint64_t exact_from = getenv("NP2_CAND_EXACT_FROM") ? strtoull(getenv("NP2_CAND_EXACT_FROM"), nullptr, 10) : (1ull << 28); // (tests lower it)
    const bool exact_bytes = c->n_cols >= exact_from && !cx->trace;
    uint32_t SB_cap = (uint32_t)std::min<uint64_t>(c->n_cols + 64, 0xFFFFFFF0ull);
    cx->mval.ensure(R + 2);
    cx->smin.ensure(R + 2);
    cx->pj.ensure(R + 2);
    cx->pcount.ensure(R + 2);
    cx->rinfo.ensure(R + 2);
    cx->reg_ncand.ensure(n_reg + 2);
    cx->reg_bytes.ensure(n_reg + 2);
    cx->reg_soff.ensure(n_reg + 2);
    cx->reg_maxlen.ensure(n_reg + 2);
    cx->blk_sum.ensure(3 * ((size_t)n_reg / 4 + 2));
    cx->blk_coff.ensure((size_t)n_reg / 4 + 2);
    cx->blk_soff.ensure((size_t)n_reg / 4 + 2);
    cx->cand_off.ensure(n_reg + 2);
    cx->kept_read.ensure((size_t)NC_cap + 2);
    cx->kept_len.ensure((size_t)NC_cap + 2);
    cx->kept_col.ensure((size_t)NC_cap + 2);
    cx->cand_order.ensure((size_t)NC_cap + 2);
    cx->cand_kmer.ensure((size_t)NC_cap + 2);
    cx->cand_seq_off.ensure((size_t)NC_cap + 2);
    if (!exact_bytes) cx->cand_seq.ensure((size_t)SB_cap + 64);
    cx->kscore.ensure((size_t)NC_cap + 2);
    cx->long_list.ensure((size_t)NC_cap + 2);
    CandPtrs cp{c->reads.p,   c->nib.p,   c->ck_off.p,      c->ckpt.p,    cx->lq_start.p, cx->lq_end.p, cx->pj.p,
                cx->pcount.p, cx->alive.p, cx->rinfo.p, c->tile_rd_off.p, c->tile_rd.p, c->n_tiles, cx->yaks[0].k,
                cx->keys_raw.p, cx->vals_raw.p, cx->tile_n.p,
                (cx->pidx_valid && cx->bucket_cap) ? cx->tile_pidx.p : nullptr, cx->bucket_cap,
                (const uint32_t *)c->refnib.p, c->L};
    {
        EventTimer t(cx, "candidates");
        // every live read covers a contiguous interval [pj, pj + pcount) of the region list
        // (both in one single-block kernel measured 58 us against 7.5 + 6: a block's worth of binary searches is a latency chain)
        launch_read_m(s, c->reads.p, R, cx->alive.p, cx->lq_start.p, n_reg, cx->mval.p);
        scan_incl_min(cx, cx->mval.p, cx->smin.p, R);
        launch_pair_count(s, c->reads.p, R, cx->alive.p, cx->lq_start.p, cx->lq_end.p, n_reg, cx->smin.p, cx->pj.p,
                          cx->pcount.p, c->ck_off.p, cx->rinfo.p);
        // one wavefront per region: find its reads, measure the candidates, keep the first 60 non-empty ones
        launch_region_measure(s, cp, n_reg, cx->kept_read.p, cx->kept_len.p, cx->kept_col.p, cx->reg_ncand.p,
                              cx->reg_bytes.p, cx->reg_maxlen.p, cx->blk_sum.p);
        {
            // (the chained variant whenever there is a region at all: a threshold had the contigs of a batch pick different
            // kernels here, and everything up to the vote went out twice, once per half of the batch)
            const bool wide = n_reg > 0;
            Lookback lb{};
            if (wide) lb = next_lookback(cx, cand_offsets_blocks(n_reg));
            launch_cand_offsets(s, cx->blk_sum.p, n_reg, cx->blk_coff.p, cx->blk_soff.p, cx->cand_off.p, cx->reg_soff.p,
                                cx->scal.p + S_NC, cx->scal.p + S_SB, cx->scal.p + S_GROW, wide ? &lb : nullptr,
                                cx->scal.p + S_ERR);
        }
        if (exact_bytes) {
            const std::vector<uint32_t> sc = fetch_scal(cx);
            check_region_err(sc[S_ERR]);
            pc.resolve(sc);
            SB_cap = (uint32_t)std::min<uint64_t>((uint64_t)pc.SB + 64, SB_cap);
            cx->cand_seq.ensure((size_t)SB_cap + 64);
        }
        launch_region_write(s, cp, n_reg, cx->kept_read.p, cx->kept_len.p, cx->kept_col.p, cx->reg_ncand.p,
                            cx->reg_bytes.p, cx->blk_coff.p, cx->blk_soff.p, cx->cand_off.p, cx->reg_soff.p, NC_cap + 1,
                            SB_cap, cx->cand_order.p, cx->cand_kmer.p, cx->cand_seq_off.p, cx->cand_seq.p);
    }
    {
        EventTimer t(cx, "kmer_score");
        launch_cand_score(s, cx->yaks[0].dev(), cx->cand_seq_off.p, cx->cand_seq.p, cx->cand_kmer.p, cx->scal.p + S_NC,
                          NC_cap, min_kmer_count, cx->kscore.p, cx->long_list.p, cx->scal.p + S_NLONG);
    }
    pc.n_reg = n_reg;
    pc.NC_cap = NC_cap;
    pc.SB_cap = SB_cap;
    pc.known = exact_bytes; // (NC / SB / grow read back above)
    if (cx->trace) pc.resolve(fetch_scal(cx));
    trace_region_tables(cx, pass, "cand", pc, false);
}

Cns fetch_cns(np2_ctx *cx, uint32_t M) {
    Cns c;
    c.pos = d2h(cx, cx->cns_pos.p, M);
    c.base = d2h(cx, cx->cns_base.p, M);
    return c;
}

} // namespace

namespace np2h {

// The per-contig loop (main.rs:1819-1836) as a stepper: begin (dense pass), then for every pass either
// vote_pass + apply_losers (a phasing pass) or final_pass.  np2_polish_resident drives it straight through; the shards
// of one contig (np2_shard_*) stop after vote_pass, exchange their votes, and continue with the contig-wide losers.
void run_begin(PolishRun &r) {
    np2_ctx *cx = r.cx;
    if (r.o.iter_count < 1) throw Np2Error(NP2_E_ARG, "iter_count must be >= 1");
    HIPCHK(hipSetDevice(cx->device));
    cx->trace_items.clear();
    cx->last_dbase = nullptr;
    cx->last_dpos = nullptr;
    cx->scal.ensure(SCAL_TOTAL);
    cx->alive.ensure(r.c->R + 2);
    {
        WallTimer w(cx, "wall_diff");
        run_diff(cx, r.c, r.T);
    }
    launch_init_alive(cx->stream, r.c->reads.p, r.c->R, cx->alive.p);
    r.pass = 0;
    r.reuse = false;
}

// graph, consensus, LQ regions and candidates of pass r.pass.  If a phasing pass voted out no read, this pass would
// rebuild a byte-identical graph, consensus, region list and candidate table (they are pure functions of the pileup and
// the live-read set): reuse them.  The reference recomputes (main.rs:1819-1836); the result is identical by construction.
void run_pass_front(PolishRun &r) {
    np2_ctx *cx = r.cx;
    np2_contig *c = r.c;
    if (!r.reuse) {
        {
            WallTimer w(cx, "wall_cns_lq");
            if (!r.front_issued) pass_front_issue(cx, c, r.T, (int)r.pass);
            r.front_issued = false;
            consensus_and_regions_finish(cx, c, r.T, (int)r.pass, r.M, r.n_reg, !r.wide_votes);
        }
        if (cx->trace) {
            trace_cns(cx, (int)r.pass, "cns_raw", fetch_cns(cx, r.M));
            trace_put(cx, (int)r.pass, "lq.start", d2h(cx, cx->lq_start.p, r.n_reg));
            trace_put(cx, (int)r.pass, "lq.end", d2h(cx, cx->lq_end.p, r.n_reg));
        }
    }
    if (r.n_reg == 0) return;
    if (!r.reuse) {
        r.pc = PassCounts();
        r.pc.M = r.M;
        WallTimer w(cx, "wall_extract");
        extract_candidates(cx, c, r.n_reg, r.o.min_kmer_count, (int)r.pass, r.pc);
    } else if (r.pc.NC_cap) { // undo mark_hete's kscore edits of the previous (identical) pass
        op_copy_d2d(cx, cx->kscore.p, cx->kscore_saved.p, (size_t)(r.pc.known ? r.pc.NC : r.pc.NC_cap) * 2);
    }
}

// a phasing pass up to the votes (vd.any == false: nobody votes)
void run_vote_pass(PolishRun &r, VoteData &vd, const std::function<void()> *after_front) {
    np2_ctx *cx = r.cx;
    vd = VoteData();
    vd.R = r.c->R;
    run_pass_front(r);
    if (after_front) (*after_front)(); // (polish_impl: the previous pass's vote is settled before this pass votes)
    if (r.n_reg == 0) return;
    WallTimer w(cx, "wall_vote");
    const bool may_reuse = cx->reuse_identical_pass && !cx->trace;
    if (may_reuse && r.pc.NC_cap) {
        cx->kscore_saved.ensure((size_t)r.pc.NC_cap + 2);
        op_copy_d2d(cx, cx->kscore_saved.p, cx->kscore.p, (size_t)(r.pc.known ? r.pc.NC : r.pc.NC_cap) * 2);
    }
    vote_collect(cx, r.c, r.pc, r.o.model_ref != 0, r.o.use_all_reads != 0, (int)r.pass, r.own_lo, r.own_hi, vd, r.wide_votes, r.key_add);
    if (r.pc.known) r.grow_prev = r.pc.grow;
}

// the reads the vote removed (align_bases = empty, main.rs:1548-1550), then on to the next pass
void run_apply_losers(PolishRun &r, const std::vector<uint32_t> &losers) {
    np2_ctx *cx = r.cx;
    if (r.n_reg) trace_put(cx, (int)r.pass, "invalid_ids", losers); // (a pass without regions never reaches the vote)
    for (uint32_t id : losers) REFPANIC_IF(id >= r.c->R, "index out of bounds: alignseqs[id]");
    const bool may_reuse = cx->reuse_identical_pass && !cx->trace;
    r.reuse = false;
    if (!losers.empty()) {
        cx->kill_ids.ensure(losers.size());
        h2d_staged(cx, cx->kill_ids.p, losers.data(), losers.size() * 4);
        launch_kill_reads(cx->stream, cx->kill_ids.p, (uint32_t)losers.size(), cx->alive.p);
        // (no wait: the ids sit in the pinned staging buffer, guarded by h2d_inflight)
    } else if (may_reuse) {
        r.reuse = true; // (also when the pass had no region at all: no read was voted out)
    }
    ++r.pass;
}

// The early start of the next pass.  Without -r the vote kernel has already flagged the reads that disagree with the contig
// at a marker (main.rs:977: removed whatever else the decision says), so while the vote is still being decided the next
// pass goes out on the flagged reads alone: they are killed where the kernel left the flags, the pass counter advances
// (what run_apply_losers does; the pass cannot be a reuse of the last one: reads are going) and graph, DP, consensus and
// LQ regions are issued.  Only kernels, no read-back.  -> the number of flagged reads; 0: nothing was started (nobody
// votes, every read is used, a tracing context, NP2_NO_SPECULATE, or no read is flagged)
size_t run_start_on_flagged(PolishRun &r, const VoteData &vd) {
    np2_ctx *cx = r.cx;
    if (!vd.any || !vd.d_bad || r.o.use_all_reads || cx->trace || cx->hooks.no_speculate) return 0;
    size_t n_flagged = 0;
    for (uint8_t b : vd.bad) n_flagged += b;
    if (n_flagged == 0) return 0;
    launch_kill_flagged(cx->stream, vd.d_bad, r.c->R, cx->alive.p);
    ++r.pass;
    r.reuse = false;
    pass_front_issue(cx, r.c, r.T, (int)r.pass);
    r.front_issued = true;
    op_submit(cx);
    return n_flagged;
}

// ... and its settlement once the decision stands: `flagged` are the flags the pass went by (local read numbers, n_flagged
// of them set), `losers` the reads the decision removes.  It removes exactly the flagged ones -> true, the pass under way
// is the right one.  It removes others too (a read flagged by the neighbouring shard, a conflicting community) -> they go
// as well; it KEEPS a flagged read (a replayed or custom loser list; the reference's own decision removes every flagged
// read) -> the read was alive before the vote, it comes back; either way -> false: the pass has to be done again
// (run_pass_front starts it, on the right reads: its results are a pure function of the live reads).
bool run_settle_flagged(PolishRun &r, const std::vector<uint8_t> &flagged, size_t n_flagged, const std::vector<uint32_t> &losers) {
    np2_ctx *cx = r.cx;
    const uint32_t R = r.c->R;
    std::vector<uint32_t> extra, spared;
    size_t n_hit = 0;
    for (uint32_t id : losers) {
        REFPANIC_IF(id >= R, "index out of bounds: alignseqs[id]");
        if (flagged[id]) ++n_hit; else extra.push_back(id);
    }
    if (n_hit != n_flagged) {
        std::vector<uint8_t> removed(R, 0);
        for (uint32_t id : losers) removed[id] = 1;
        for (uint32_t id = 0; id < R; ++id)
            if (flagged[id] && !removed[id]) spared.push_back(id);
    }
    if (cx->hooks.shard_spec_log && r.wide_votes) fprintf(stderr, "[np2 shard] apply: %zu removed here, %zu beyond the flagged ones, %zu flagged ones kept\n", losers.size(), extra.size(), spared.size());
    if (extra.empty() && spared.empty() && !cx->hooks.test_misspeculate) return true; // (test hook: the redo branch)
    if (!spared.empty()) {
        cx->kill_ids.ensure(spared.size() + 1);
        h2d_staged(cx, cx->kill_ids.p, spared.data(), spared.size() * 4);
        launch_revive_reads(cx->stream, cx->kill_ids.p, (uint32_t)spared.size(), cx->alive.p);
        op_sync(cx); // (the staging buffer is reused for the other list right away)
    }
    if (!extra.empty()) {
        cx->kill_ids.ensure(extra.size() + 1);
        h2d_staged(cx, cx->kill_ids.p, extra.data(), extra.size() * 4);
        launch_kill_reads(cx->stream, cx->kill_ids.p, (uint32_t)extra.size(), cx->alive.p);
    }
    r.reuse = false;
    r.front_issued = false;
    return false;
}

// a vote decided here and now, filed with the context: its wall time and, in a tracing context, the graph it was taken on
static std::vector<uint32_t> decide_and_file(np2_ctx *cx, const VoteData &vd, bool use_all, int pass) {
    VoteDecideInfo info;
    info.want_graph = cx->trace;
    std::vector<uint32_t> losers = vote_decide(vd, use_all, &info);
    if (!vd.any) return losers; // (nothing was decided)
    if (cx->trace) {
        trace_put(cx, pass, "vote.row_off", info.row_off);
        trace_put(cx, pass, "vote.rows", info.rows);
    }
    cx->timing.host.push_back({"wall_louvain", (float)info.ms});
    return losers;
}

void polish_impl(np2_ctx *cx, np2_contig *c, const np2_opts_t *o, ResultOut &result) {
    PolishRun r;
    r.cx = cx, r.c = c, r.o = *o;
    run_begin(r);
    const bool use_all = o->use_all_reads != 0;
    // The host side of the vote (key order, rows, Louvain: ~1 ms for a 1.5 Mb diploid contig, 100 ms for a chromosome) is
    // the longest host phase of a contig, and the device has nothing to do for it meanwhile.  Without -r the vote kernel
    // has already flagged the reads that disagree with the contig at a marker (main.rs:977); the Louvain only adds the
    // reads of conflicting communities AMONG the others, which is rare (never on the synthetic diploid workloads: the
    // removed reads are exactly the flagged ones).  So the vote is decided on a helper thread (a contig on its own
    // context) or next to the first part of the pass (batch driver) while this pipeline goes on
    // with the next pass on the flagged reads alone: its graph, DP, consensus and LQ regions go to the device at once
    // (a flush nobody waits for in the batch driver), the rest of the pass follows; the decision is awaited before the
    // next vote is collected, or before the result is handed out, and if it removes other reads as well the pass is
    // simply done again with them (its results are a pure function of the live reads).
    struct Decision {
        std::vector<uint32_t> losers;
        double ms = 0;
    };
    struct Pending {
        std::future<Decision> fut;
        std::shared_ptr<VoteData> vd;
        size_t n_bad = 0;
        bool active = false;
    } pend;
    auto settle = [&]() -> bool { // (run_settle_flagged: false = the pass has to be done again)
        if (!pend.active) return true;
        pend.active = false;
        Decision d = pend.fut.get(); // (rethrows what the decision threw: the reference's panics)
        cx->timing.host.push_back({"wall_louvain", (float)d.ms});
        return run_settle_flagged(r, pend.vd->bad, pend.n_bad, d.losers);
    };
    const std::function<void()> settle_then_redo = [&]() {
        if (!settle()) run_pass_front(r); // (again, on the right reads)
    };
    while (!r.final_pass()) {
        auto vd = std::make_shared<VoteData>();
        run_vote_pass(r, *vd, &settle_then_redo);
        // (the tile kernel's phase clocks are read back inside pass_front_issue — through the very staging the pairs still sit
        // in, which may move: tools/pf_prof.py died there)
        if (cx->hooks.pf_prof) vd->own();
        const size_t n_bad = run_start_on_flagged(r, *vd);
        if (n_bad == 0) {
            run_apply_losers(r, decide_and_file(cx, *vd, use_all, (int)r.pass));
            continue;
        }
        pend.vd = vd;
        pend.n_bad = n_bad;
        pend.active = true;
        auto decide = [vd, use_all]() {
            Decision d;
            const double t0 = now_ms();
            d.losers = vote_decide(*vd, use_all);
            d.ms = now_ms() - t0;
            return d;
        };
        if (tl_recorder() == nullptr) {
            // one contig on its own context (a chromosome: ~100 ms of host vote next to ~50 ms of device work for the pass)
            vd->own(); // (the rows sit in the context's read-back staging, which the pipeline goes on using meanwhile)
            pend.fut = std::async(std::launch::async, decide);
        } else {
            // Under the batch driver the decision is taken here and now, next to the part of the pass that is already on
            // its way: with four batch groups the device is the busy part of a step, and seventeen more host threads
            // deciding votes beside the pipelines' own cost more than the rest of the overlap gave (3.72 ms per
            // yeast-sized assembly this way, 3.9 - 4.1 with helper threads; 4.06 without any early start).
            // The rows are read where the vote's read-back left them: nothing has been read back since, and nothing is
            // before the decision stands.
            std::promise<Decision> p;
            pend.fut = p.get_future();
            try {
                p.set_value(decide());
            } catch (...) {
                p.set_exception(std::current_exception());
            }
            (void)settle(); // (a decision that removes more reads: the pass is started again by the next run_pass_front)
        }
    }
    for (;;) {
        run_final_pass(r, result);
        if (settle()) break;
        result.release();
    }
}

} // namespace np2h

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int np2_polish_resident(np2_ctx_t *cx, np2_contig_t *c, const np2_opts_t *opts, uint8_t **out_bases,
                        uint32_t **out_pos, uint64_t *out_len) {
    if (!cx || !c || !opts || !out_len) return NP2_E_ARG;
    ResultOut r;
    r.want_pos = out_pos != nullptr;
    r.want_bases = out_bases != nullptr;
    const double t_wall0 = now_ms(), t_cpu0 = thread_cpu_ms();
    const int rc = abi_guard([&] {
        polish_impl(cx, c, opts, r);
        cx->timing.host.push_back({"wall_polish", (float)(now_ms() - t_wall0)});
        cx->timing.host.push_back({"cpu_polish", (float)(thread_cpu_ms() - t_cpu0)});
        flush_timings(cx);
        return NP2_OK;
    }, ctx_sink(cx, true));
    if (rc != NP2_OK) {
        r.release();
        return rc;
    }
    *out_len = r.len;
    if (out_bases) *out_bases = r.bases;
    if (out_pos) *out_pos = r.pos;
    return NP2_OK;
}

int np2_polish_contig(np2_ctx_t *cx, const uint8_t *ref, uint32_t L, const np2_read_t *reads, uint32_t n_reads,
                      const uint8_t *nibbles, uint64_t nib_bytes, const np2_opts_t *opts, uint8_t **out_bases,
                      uint32_t **out_pos, uint64_t *out_len) {
    np2_contig_t *c = nullptr;
    int rc = np2_contig_upload(cx, ref, L, reads, n_reads, nibbles, nib_bytes, &c);
    if (rc) return rc;
    rc = np2_polish_resident(cx, c, opts, out_bases, out_pos, out_len);
    np2_contig_free(cx, c);
    return rc;
}

} // extern "C"
