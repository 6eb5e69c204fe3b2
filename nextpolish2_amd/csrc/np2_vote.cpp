// The phasing vote: its device half (vote_collect: mark_hete and the pair votes of one pass, read back in the form the
// host half takes) and the host-only entry points of include/np2.h around the host half (np2_vote_host.hpp,
// np2_phase_host.hpp): np2_vote_decide, np2_phase_vote, np2_swiss_order.
#include "np2_polish.hpp"

#include <algorithm>
#include <cstdlib>
#include <vector>

using namespace np2;

namespace {

// The per-read outputs of the vote kernels live in one buffer, [first_reg u32 x RP][ref_w i32 x RP][ref_seen u8 x RP]
// [bad u8 x RP]; in the plain pipeline's (votepack) the row offsets and the adjacency rows follow — one piece to read back
struct VoteLayout {
    size_t RP;       // the reads, padded to a multiple of 64
    size_t per_read; // bytes of the four per-read arrays together
    size_t o_first = 0, o_refw, o_seen, o_bad;
    size_t off_bytes;
    static size_t row_off_bytes(uint32_t R) { return (((size_t)R + 2) * 4 + 15) & ~(size_t)15; }
    explicit VoteLayout(uint32_t R)
        : RP(((size_t)R + 63) & ~(size_t)63), per_read(RP * 10), o_refw(RP * 4), o_seen(RP * 8), o_bad(RP * 9), off_bytes(row_off_bytes(R)) {}
    size_t rows_at() const { return per_read + off_bytes; } // (the row offsets start at per_read)
};

} // namespace

namespace np2h {

// GPU part of the phasing pass: mark_hete (main.rs:916-946), pair votes (948-1002) over the regions whose start lies in
// [own_lo, own_hi)
// `wide`: pairs as (a << 32 | b, counts) — what the shards of a contig export and merge; otherwise the finished adjacency
// rows of the vote's graph, read back in the SAME wait as the counters that size them (one device round trip less, and
// no row building on the host)
void vote_collect(np2_ctx *cx, np2_contig *c, PassCounts &pc, bool asref, bool use_all, int pass, uint32_t own_lo,
                  uint32_t own_hi, VoteData &vd, bool wide, uint64_t key_add) {
    hipStream_t s = cx->stream;
    const uint32_t R = c->R, n_reg = pc.n_reg;
    RegionTables rt = region_tables(cx, n_reg);
    const VoteLayout vl(R);
    uint32_t NE = 0, NU = 0;
    vd = VoteData();
    vd.R = R;
    {
        EventTimer t(cx, "vote_phase");
        cx->reg_lable.ensure(n_reg + 2);
        cx->grp.ensure((size_t)pc.NC_cap + 2);
        cx->ecount.ensure(n_reg + 2);
        cx->eoff.ensure(std::max<size_t>(n_reg + 2, (size_t)c->L + 2));
        const size_t band_words = (size_t)R * EDGE_BAND;
        uint8_t *vbuf;
        uint32_t *row_off;
        if (wide) {
            cx->votebuf.ensure(vl.per_read);
            cx->band_off.ensure((size_t)R + 2);
            vbuf = cx->votebuf.p, row_off = cx->band_off.p;
        } else {
            cx->votepack.ensure(vl.rows_at() + band_words * 2 * sizeof(phase::Graph::Edge) + 64); // (every pair is listed in two rows)
            vbuf = cx->votepack.p, row_off = (uint32_t *)(cx->votepack.p + vl.per_read);
        }
        uint32_t *v_first = (uint32_t *)(vbuf + vl.o_first);
        int32_t *v_refw = (int32_t *)(vbuf + vl.o_refw);
        uint8_t *v_seen = vbuf + vl.o_seen, *v_bad = vbuf + vl.o_bad;
        op_fill(cx, v_first, 0xFF, vl.o_refw - vl.o_first);
        op_fill(cx, v_refw, 0, vl.per_read - vl.o_refw);
        launch_vote_phase(s, rt, asref, use_all, cx->lq_start.p, own_lo, own_hi, cx->reg_lable.p, cx->grp.p, cx->ecount.p,
                          v_refw, v_seen, v_bad, v_first, cx->scal.p + S_ERR);
        exclusive_total_n(cx, cx->ecount.p, cx->eoff.p, n_reg);
        launch_vote_counts(s, v_first, v_bad, R, cx->scal.p + S_M1); // S_M1 = graph keys, S_M2 = invalid reads
        // distinct read pairs + their vote counts, queued behind the vote without waiting for its counts (one read-back
        // less per phasing pass; with no HETE region the three kernels find nothing to do).  Normal case: the raw pair
        // votes are accumulated in the banded matrix (reads are numbered in start order, partners are close); rows read
        // in order = the sorted unique list, at most EDGE_BAND pairs per read.
        cx->band.ensure(band_words + 4);
        cx->band_n.ensure((size_t)R + 2);
        op_fill(cx, cx->scal.p + S_M3, 0, 4);
        launch_edges_row(s, rt, cx->grp.p, cx->ecount.p, cx->pj.p, cx->pcount.p, cx->alive.p, R, cx->band.p, cx->band_n.p,
                         cx->scal.p + S_M3);
        if (wide) {
            exclusive_total_n(cx, cx->band_n.p, row_off, R);
            cx->ekey.ensure(band_words + 2);
            cx->eval.ensure(band_words + 2);
            launch_band_emit(s, cx->band.p, R, row_off, cx->ekey.p, cx->eval.p, cx->scal.p + S_NRAW, key_add);
        } else {
            // the rows' edge counts (both directions of every pair, flagged reads left out), their offsets, the rows
            cx->row_cnt.ensure((size_t)R + 2);
            launch_vote_rows_count(s, cx->band.p, cx->band_n.p, v_bad, use_all, R, cx->row_cnt.p, cx->scal.p + S_NOKEY);
            exclusive_total_n(cx, cx->row_cnt.p, row_off, R);
            launch_vote_rows_emit(s, cx->band.p, cx->band_n.p, v_bad, use_all, v_first, R, row_off, cx->votepack.p + vl.rows_at(),
                                  cx->scal.p + S_NRAW, cx->scal.p + S_NOKEY);
        }
    }
    auto per_read = [&](const uint8_t *vb) {
        vd.first_key.assign((const uint32_t *)(vb + vl.o_first), (const uint32_t *)(vb + vl.o_first) + R);
        vd.ref_w.assign((const int32_t *)(vb + vl.o_refw), (const int32_t *)(vb + vl.o_refw) + R);
        vd.ref_seen.assign(vb + vl.o_seen, vb + vl.o_seen + R);
        vd.bad.assign(vb + vl.o_bad, vb + vl.o_bad + R);
    };
    bool far = false, have_per_read = false;
    {
        std::vector<uint32_t> sc;
        uint8_t *pin = nullptr;
        // edges the first copy has room for: 128 per read (a 30x diploid pileup has ~36 partners above a read and as many
        // below it); more follow in a second copy
        const size_t EB = sizeof(phase::Graph::Edge);
        static_assert(sizeof(phase::Graph::Edge) == 8 && alignof(phase::Graph::Edge) <= 8, "an edge is {u32 neighbour, f32 weight}");
        const uint32_t likely = (uint32_t)std::min<size_t>((size_t)R * EDGE_BAND * 2, std::max<size_t>((size_t)R * 128, 1u << 15));
        if (wide) {
            sc = fetch_scal(cx, cx->scal.p + S_M0, cx->eoff.p + n_reg);
        } else {
            // counters, per-read arrays, row offsets and the rows in ONE wait: the mailbox post, two copies (the second
            // one sized on the device by the number of edges), one synchronisation
            pin = (uint8_t *)cx->pin_d2h.ensure(vl.rows_at() + (size_t)likely * EB + 64);
            const uint32_t seq = ++cx->mbox_seq;
            launch_post(cx->stream, cx->scal.p, S_COUNT, cx->mbox_dev, seq, cx->scal.p + S_M0, cx->eoff.p + n_reg, nullptr, nullptr,
                        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
            op_d2h(cx, pin, cx->votepack.p, vl.rows_at());
            launch_copy_counted(cx->stream, (uint32_t *)(pin + vl.rows_at()), (const uint32_t *)(cx->votepack.p + vl.rows_at()),
                                (const uint32_t *)(cx->votepack.p + vl.per_read) + R, likely * (uint32_t)(EB / 4), (uint32_t)(EB / 4));
            op_sync(cx);
            if (__atomic_load_n(&cx->mbox_host[0], __ATOMIC_ACQUIRE) != seq)
                throw Np2Error(NP2_E_DEVICE, "mailbox not posted after a synchronisation");
            sc.assign(cx->mbox_host + 1, cx->mbox_host + 1 + S_COUNT);
        }
        check_region_err(sc[S_ERR]);
        pc.resolve(sc);
        NE = sc[S_M0];
        if (!cx->trace && sc[S_M1] == 0 && sc[S_M2] == 0) { // no read votes anywhere: nobody can lose
            if (NE) throw Np2Error(NP2_E_DEVICE, "internal: pair edges without voting reads");
            return;
        }
        NU = sc[S_NRAW];
        far = sc[S_M3] != 0 || cx->hooks.edge_sort; // (test hook: force the sort-based path)
        // (counts, read through np2_last_timings by the tests: which form the pass's vote arrived in)
        if (!wide) cx->timing.host.push_back({far ? "vote_sort" : "vote_rows", 1.0f});
        if (!wide) {
            per_read(pin);
            have_per_read = true;
            vd.d_bad = cx->votepack.p + vl.o_bad;
            if (!far) {
                if (NU > likely) { // more edges than the first copy had room for: fetch the whole piece again
                    pin = (uint8_t *)cx->pin_d2h.ensure(vl.rows_at() + (size_t)NU * EB + 64);
                    op_d2h(cx, pin, cx->votepack.p, vl.rows_at() + (size_t)NU * EB);
                    op_sync(cx);
                }
                // (the rows stay in the staging: Graph::adopt_rows borrows them from there)
                vd.off = (const uint32_t *)(pin + vl.per_read), vd.edges = (const phase::Graph::Edge *)(pin + vl.rows_at());
                vd.n_nokey = sc[S_NOKEY];
                if (vd.off[R] != NU) throw Np2Error(NP2_E_DEVICE, "internal: vote rows and edge count disagree");
            }
        }
    }
    vd.any = true;
    if (NE && far) { // some pair lies outside the band (deep pileup): sort the raw votes instead
        {
            EventTimer t(cx, "vote_phase");
            cx->ekey.ensure(NE + 2);
            cx->ekey_s.ensure(NE + 2);
            cx->eval.ensure(NE + 2);
            cx->eval_s.ensure(NE + 2);
            cx->eflag.ensure(NE + 2);
            cx->eidx.ensure(NE + 2);
            cx->ew.ensure(NE + 2);
            cx->tmp.ensure(prim_temp_bytes((size_t)NE + 2));
            launch_edges_write(s, rt, cx->reg_lable.p, cx->grp.p, cx->ecount.p, cx->eoff.p, cx->ekey.p, cx->eval.p);
            unsigned rbits = 1;
            while ((1ull << rbits) < (uint64_t)R + 1) ++rbits;
            prim_op(cx, [=](hipStream_t st) {
                if (prim_sort_pairs_u64_u32(st, cx->tmp.p, cx->tmp.cap, cx->ekey.p, cx->ekey_s.p, cx->eval.p, cx->eval_s.p, NE,
                                            32 + rbits))
                    throw Np2Error(NP2_E_DEVICE, "rocprim edge sort failed");
            });
            launch_edge_reduce(s, cx->ekey_s.p, cx->eval_s.p, NE, cx->eflag.p, (uint32_t *)cx->ew.p);
            exclusive_total(cx, cx->eflag.p, cx->eidx.p, NE);
            // compact into ekey / eval (packed agree | disagree << 16 counts)
            launch_edge_compact(s, cx->ekey_s.p, cx->eflag.p, cx->eidx.p, (const uint32_t *)cx->ew.p, NE, cx->ekey.p,
                                cx->eval.p, cx->scal.p + S_NRAW);
            NU = fetch_scal(cx)[S_NRAW];
        }
    } else if (!NE) {
        NU = 0;
    }
    if (wide || far) {
        // one wait for everything the host side of the vote still needs: unique pairs, their counts, (wide:) the per-read
        // vote arrays
        const size_t b_key = ((size_t)NU * 8 + 15) & ~(size_t)15, b_w = ((size_t)NU * 4 + 15) & ~(size_t)15;
        const size_t b_pr = have_per_read ? 0 : vl.per_read;
        uint8_t *pin = (uint8_t *)cx->pin_d2h.ensure(b_key + b_w + b_pr + 64);
        if (tl_recorder()) {
            // batch driver: the pieces are gathered into one device buffer by copy kernels (one launch each for all
            // contigs of the batch) and cross the bus as ONE transfer per contig
            cx->votepack2.ensure(b_key + b_w + b_pr + 64);
            op_copy_d2d(cx, cx->votepack2.p, cx->ekey.p, (size_t)NU * 8);
            op_copy_d2d(cx, cx->votepack2.p + b_key, cx->eval.p, (size_t)NU * 4);
            if (b_pr) op_copy_d2d(cx, cx->votepack2.p + b_key + b_w, cx->votebuf.p, b_pr);
            op_d2h(cx, pin, cx->votepack2.p, b_key + b_w + b_pr);
        } else {
            op_d2h(cx, pin, cx->ekey.p, (size_t)NU * 8);
            op_d2h(cx, pin + b_key, cx->eval.p, (size_t)NU * 4);
            if (b_pr) op_d2h(cx, pin + b_key + b_w, cx->votebuf.p, b_pr);
        }
        op_sync(cx);
        // the pairs stay where they landed (the context's pinned read-back staging: valid until its next read-back; a
        // chromosome's list is 200 MB): the plain pipeline decides the vote right away, a shard copies them first
        vd.view_key = (const uint64_t *)pin, vd.view_cnt = (const uint32_t *)(pin + b_key), vd.view_n = NU;
        vd.key_added = wide && !far; // (the sort path's keys are local)
        if (b_pr) {
            per_read(pin + b_key + b_w);
            if (wide) vd.d_bad = cx->votebuf.p + vl.o_bad; // (where the vote kernel left the flags: np2_shard_vote's early start)
        }
    }
    if (cx->trace) {
        vd.own(); // (the traces below read back through the same staging)
        trace_put(cx, pass, "hete.lable", d2h(cx, cx->reg_lable.p, n_reg));
        trace_put(cx, pass, "hete.kscore", d2h(cx, cx->kscore.p, pc.NC));
    }
}

} // namespace np2h

extern "C" {

int np2_vote_decide(const np2_vote_t *votes, int n_votes, uint32_t n_reads_total, const np2_opts_t *opts, uint32_t *losers,
                    uint32_t *n_losers) {
    if (!votes || n_votes < 1 || !opts || !losers || !n_losers) return NP2_E_ARG;
    return abi_guard([&] {
        const bool use_all = opts->use_all_reads != 0;
        VoteData vd;
        if (const int rc = vote_merge(votes, n_votes, n_reads_total, vd)) return rc;
        // test hook (no device needed): the same vote in the form the plain pipeline reads back from the vote kernels
        // — finished adjacency rows —, so that the adopting path is checked against recorded votes on the CPU
        if (getenv("NP2_VOTE_COMPACT") && !vote_rows_from_pairs(vd, use_all)) return NP2_E_UNSUPPORTED; // (such a vote takes the wide form)
        const std::vector<uint32_t> ls = vote_decide(vd, use_all);
        *n_losers = (uint32_t)ls.size();
        std::copy(ls.begin(), ls.end(), losers);
        return NP2_OK;
    });
}

int np2_phase_vote(const uint32_t *keys, uint32_t n_keys, const uint32_t *pa, const uint32_t *pb, const float *pw,
                   uint64_t n_pairs, const uint32_t *ref_ids, const float *ref_w, uint32_t n_ref, int has_ref,
                   uint32_t *out_ids, uint32_t *n_out) {
    if (!keys || !out_ids || !n_out) return NP2_E_ARG;
    return abi_guard([&] {
        uint32_t mx = 0;
        for (uint32_t i = 0; i < n_keys; ++i) mx = std::max(mx, keys[i]);
        for (uint32_t i = 0; i < n_ref; ++i) mx = std::max(mx, ref_ids[i]);
        phase::Graph g;
        g.reserve_ids(mx + 1);
        for (uint32_t i = 0; i < n_keys; ++i) g.add_key(keys[i]);
        if (!g.add_edges(n_pairs, [&](uint64_t i) { return pa[i]; }, [&](uint64_t i) { return pb[i]; },
                         [&](uint64_t i) { return pw[i]; }))
            return NP2_E_ARG;
        std::vector<float> rw(mx + 1, 0.f);
        std::vector<uint8_t> rs(mx + 1, 0);
        for (uint32_t i = 0; i < n_ref; ++i) {
            rw[ref_ids[i]] = ref_w[i];
            rs[ref_ids[i]] = 1;
        }
        std::vector<uint32_t> losers;
        if (!phase::losing_reads(std::move(g), has_ref != 0, rw, rs, losers)) return NP2_E_REFPANIC;
        std::sort(losers.begin(), losers.end());
        losers.erase(std::unique(losers.begin(), losers.end()), losers.end());
        *n_out = (uint32_t)losers.size();
        for (size_t i = 0; i < losers.size(); ++i) out_ids[i] = losers[i];
        return NP2_OK;
    });
}

// host-only test hook: iteration order of the product's SwissTable order model (np2_phase_host.hpp) after a script of
// op 0 = insert(key), 1 = remove(key), 2 = entry(key).or_insert — checked against hand-traced vectors
int np2_swiss_order(const uint32_t *ops, const uint32_t *keys, uint32_t n, uint32_t *out, uint32_t *n_out) {
    if (!ops || !keys || !out || !n_out) return NP2_E_ARG;
    return abi_guard([&] {
        phase::SwissOrderMap<int> m;
        for (uint32_t i = 0; i < n; ++i) {
            if (ops[i] == 0)
                m.put(keys[i], 0);
            else if (ops[i] == 1)
                m.take(keys[i], nullptr);
            else if (!m.has(keys[i]))
                m.put_vacant(keys[i], 0);
        }
        uint32_t c = 0;
        m.each([&](uint32_t k, const int &) { out[c++] = k; });
        *n_out = c;
        return NP2_OK;
    });
}

} // extern "C"
