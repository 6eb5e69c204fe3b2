// The shards of one contig (multi-GPU: reference intervals of a long contig), C ABI np2_shard_* of include/np2.h: plan,
// upload, and the protocol vote / apply per phasing pass, final.  The pipeline itself is np2_polish.cpp's stepper.
#include "np2_polish.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

using namespace np2;

namespace {

// ---- shards of one contig ----------------------------------------------------------------------------------------------
// A shard polishes the sub-contig [sub_lo, sub_hi) that holds every read overlapping its owned interval widened by a halo,
// as if it were a contig of its own; inside [own_lo - halo, own_hi + halo) every read of the whole contig is present, so
// graph, DP (exact between clean positions), LQ regions, candidates and recheck chains there are those of
// the whole contig.  What is not local: the phasing vote (collected per shard over the regions it owns, decided once per
// contig on the merged votes, main.rs:948-1015) and the reads it removes (applied everywhere).
struct ShardRun {
    PolishRun run;
    np2_shard_plan_t plan{};
    uint32_t verify = 0; // positions beyond the owned interval that are emitted as well (checked by the stitcher)
    // last exported vote (borrowed by the caller until the next call)
    std::vector<uint64_t> v_key;
    std::vector<uint32_t> v_cnt, v_read, v_first;
    std::vector<int32_t> v_refw;
    std::vector<uint8_t> v_flags;
    // np2_shard_final_device: the owned slice of the device-resident result
    uint64_t own_off = 0, own_len = 0;
    bool have_piece = false;
    // the pass started on the reads the vote kernel flagged while the ranks' votes are merged and decided (np2_shard_vote /
    // np2_shard_apply): the flags it went by, local read numbers
    bool spec = false;
    std::vector<uint8_t> spec_bad;
    size_t spec_n_bad = 0;
};
inline uint32_t shard_global_read(const np2_shard_plan_t &pl, uint32_t local) { return local == 0 ? 0u : pl.read_lo + local - 1; }

// A splice cursor that got stuck (update_consensus_with_lqseqs, main.rs:1036-1056) leaves every region to its right
// untouched — contig-wide: a shard cannot reproduce that on its own, whichever shard sees it (the first one included:
// the shards to its right would go on splicing).  Only a region stuck beyond the right end of the zone is harmless:
// coverage is partial there (an artefact of the cut) and everything it freezes lies outside of what this shard emits.
void shard_check_stuck(ShardRun *sr) {
    np2_ctx *cx = sr->run.cx;
    const np2_shard_plan_t &pl = sr->plan;
    if (!sr->run.n_reg) return;
    std::vector<uint32_t> rounds = d2h(cx, cx->scal.p + S_COUNT, 2 * (cx->yaks.size() + 1));
    uint32_t worst = 0; // highest region index + 1 = the leftmost stuck region over all rounds
    for (size_t v = 0; v < rounds.size(); v += 2) worst = std::max(worst, rounds[v]);
    if (!worst) return;
    if (worst > sr->run.n_reg) throw Np2Error(NP2_E_DEVICE, "internal: stuck region index out of range");
    const uint32_t at = d2h(cx, cx->lq_start.p + (worst - 1), 1)[0];
    if ((uint64_t)at + pl.sub_lo < pl.zone_hi)
        throw Np2Error(NP2_E_UNSUPPORTED, "splice cursor stuck inside a shard: polish this contig unsharded");
}

// a block of the process-wide pinned pool for one read-back
struct PinnedBlock {
    void *p = nullptr;
    explicit PinnedBlock(size_t bytes) : p(pinned_pool().get(std::max<size_t>(bytes, 64))) {
        if (!p) throw Np2Error(NP2_E_NOMEM, "hipHostMalloc failed");
    }
    ~PinnedBlock() {
        if (std::uncaught_exceptions() > 0) (void)hipDeviceSynchronize(); // (a copy into it may still be in flight)
        pinned_pool().put(p);
    }
    PinnedBlock(const PinnedBlock &) = delete;
    PinnedBlock &operator=(const PinnedBlock &) = delete;
};

} // namespace

extern "C" {

int np2_shard_plan(const np2_read_t *reads, uint32_t n_reads, uint32_t L, uint32_t n_shards, uint32_t halo,
                   np2_shard_plan_t *out) {
    if (!reads || !out || n_reads < 1 || n_shards < 1 || L < 3) return NP2_E_ARG;
    for (uint32_t k = 0; k < n_shards; ++k) {
        np2_shard_plan_t &p = out[k];
        p.own_lo = (uint32_t)((uint64_t)L * k / n_shards);
        p.own_hi = (uint32_t)((uint64_t)L * (k + 1) / n_shards);
        if (k) p.own_lo &= ~1023u; // (cuts on tile boundaries; the last shard ends at L)
        if (k + 1 < n_shards) p.own_hi &= ~1023u;
        if (p.own_hi <= p.own_lo) return NP2_E_ARG; // contig too short for that many shards
        const uint32_t zlo = p.own_lo > halo ? p.own_lo - halo : 0u;
        const uint32_t zhi = (uint64_t)p.own_hi + halo < L ? p.own_hi + halo : L;
        // every read overlapping the zone, whole; the sub-contig spans from the first start to the last end among them
        uint32_t rlo = 0xFFFFFFFFu, rhi = 0, slo = zlo, shi = zhi;
        for (uint32_t r = 1; r < n_reads; ++r) {
            const np2_read_t &rd = reads[r];
            if (rd.flags & NP2_READ_DROPPED) continue;
            if (rd.aln_t_e < zlo || rd.aln_t_s >= zhi) continue;
            rlo = std::min(rlo, r);
            rhi = std::max(rhi, r + 1);
            slo = std::min(slo, rd.aln_t_s);
            shi = std::max(shi, rd.aln_t_e + 1);
        }
        if (rlo == 0xFFFFFFFFu) rlo = rhi = 1;
        p.read_lo = rlo;
        p.read_hi = rhi;
        p.sub_lo = k == 0 ? 0u : (slo & ~63u); // (64-aligned: the packed contig slice starts on a byte / word boundary)
        p.sub_hi = k + 1 == n_shards ? L : shi;
        p.zone_lo = zlo;
        p.zone_hi = zhi;
    }
    return NP2_OK;
}

int np2_shard_upload(np2_ctx_t *cx, const uint8_t *ref, uint32_t L, const np2_read_t *reads, uint32_t n_reads,
                     const uint8_t *nibbles, uint64_t nib_bytes, const np2_shard_plan_t *pl, np2_contig_t **out) {
    if (!cx || !ref || !reads || !nibbles || !pl || !out) return NP2_E_ARG;
    *out = nullptr;
    return abi_guard([&] {
        if (pl->sub_hi > L || pl->sub_lo >= pl->sub_hi || pl->read_hi > n_reads || pl->read_lo < 1 || pl->read_lo > pl->read_hi)
            throw Np2Error(NP2_E_ARG, "shard plan does not fit the contig");
        const uint32_t Ls = pl->sub_hi - pl->sub_lo, n = 1 + (pl->read_hi - pl->read_lo);
        // local read 0: the sub-contig aligned to itself, packed here (AlignSeq::new of main.rs:1732-1739 on the slice)
        const uint64_t ref_bytes = ((((uint64_t)Ls + 1) >> 1) + 1 + 15) & ~15ull;
        // nibble streams of the shard's reads: one contiguous piece of the contig's buffer (reads are stored in order)
        uint64_t lo = ~0ull, hi = 0;
        for (uint32_t r = pl->read_lo; r < pl->read_hi; ++r) {
            lo = std::min<uint64_t>(lo, reads[r].nib_off);
            hi = std::max<uint64_t>(hi, reads[r].nib_off + (((uint64_t)reads[r].n_cols + 1) >> 1) + 1);
        }
        if (lo == ~0ull) lo = hi = 0;
        if (hi + 16 > nib_bytes && hi) throw Np2Error(NP2_E_ARG, "nibble stream (plus 16 B tail padding) exceeds the buffer");
        const uint64_t piece = hi > lo ? ((hi - lo + 15) & ~15ull) : 0;
        const uint64_t total = ref_bytes + piece + 64;
        std::vector<uint8_t> host(total, 0);
        for (uint32_t i = 0; i < Ls; ++i) {
            const uint8_t code = ascii_to_code(ref[pl->sub_lo + i]);
            host[i >> 1] |= (i & 1) ? code : (uint8_t)(code << 4);
        }
        host[Ls >> 1] |= (Ls & 1) ? 0x0F : 0xFF;
        if (piece) memcpy(host.data() + ref_bytes, nibbles + lo, std::min<uint64_t>(piece, nib_bytes - lo));
        std::vector<np2_read_t> rds(n);
        memset(rds.data(), 0, n * sizeof(np2_read_t));
        rds[0].aln_t_s = 0, rds[0].aln_t_e = Ls - 1, rds[0].n_cols = Ls, rds[0].nib_off = 0;
        for (uint32_t i = 1; i < n; ++i) {
            const np2_read_t &g = reads[pl->read_lo + i - 1];
            np2_read_t &d = rds[i];
            d = g;
            const bool outside = (g.flags & NP2_READ_DROPPED) || g.aln_t_e < pl->zone_lo || g.aln_t_s >= pl->zone_hi;
            if (outside) { // keeps its index (like a read the clip filter emptied, main.rs:571)
                d.flags |= NP2_READ_DROPPED;
                d.n_cols = 0;
                d.aln_t_s = d.aln_t_e = 0;
                d.nib_off = ref_bytes; // (any valid 16-B aligned slot: never decoded)
                continue;
            }
            if (g.aln_t_s < pl->sub_lo || g.aln_t_e >= pl->sub_hi) throw Np2Error(NP2_E_ARG, "shard plan: read outside the sub-contig");
            d.aln_t_s = g.aln_t_s - pl->sub_lo;
            d.aln_t_e = g.aln_t_e - pl->sub_lo;
            d.nib_off = ref_bytes + (g.nib_off - lo);
        }
        return np2_contig_upload(cx, ref + pl->sub_lo, Ls, rds.data(), n, host.data(), total, out);
    }, ctx_sink(cx));
}

int np2_shard_begin(np2_ctx_t *cx, np2_contig_t *c, const np2_shard_plan_t *pl, const np2_opts_t *opts, uint32_t verify,
                    np2_shard_run_t **out) {
    if (!cx || !c || !pl || !opts || !out) return NP2_E_ARG;
    *out = nullptr;
    return abi_guard([&] {
        std::unique_ptr<ShardRun> sr(new ShardRun());
        sr->plan = *pl;
        sr->verify = verify;
        sr->run.cx = cx, sr->run.c = c, sr->run.o = *opts;
        sr->run.own_lo = pl->own_lo - pl->sub_lo;
        sr->run.own_hi = pl->own_hi - pl->sub_lo;
        sr->run.wide_votes = true; // (exported as np2_vote_t and merged with the other shards')
        if (c->L != pl->sub_hi - pl->sub_lo || c->R != 1 + (pl->read_hi - pl->read_lo))
            throw Np2Error(NP2_E_ARG, "contig is not the upload of this shard plan");
        run_begin(sr->run);
        *out = (np2_shard_run_t *)sr.release();
        return NP2_OK;
    }, ctx_sink(cx));
}
void np2_shard_end(np2_shard_run_t *h) { delete (ShardRun *)h; }
int np2_shard_passes_left(np2_shard_run_t *h) {
    ShardRun *sr = (ShardRun *)h;
    return sr ? (int)(sr->run.o.iter_count - sr->run.pass) : 0;
}

int np2_shard_vote(np2_shard_run_t *h, np2_vote_t *out) {
    ShardRun *sr = (ShardRun *)h;
    if (!sr || !out || sr->run.final_pass()) return NP2_E_ARG;
    np2_ctx *cx = sr->run.cx;
    return abi_guard([&] {
        VoteData vd;
        const np2_shard_plan_t &pl = sr->plan;
        // (local read i >= 1 is contig read read_lo + i - 1 and read 0 never enters a pair: one 64-bit add renumbers both
        // ends, and the keys stay sorted; the emitting kernel adds it — a chromosome's shard exports tens of millions of pairs)
        const uint64_t shift = pl.read_lo - 1, add = (shift << 32) | shift;
        sr->run.key_add = add;
        run_vote_pass(sr->run, vd);
        sr->v_key.clear(), sr->v_cnt.clear(), sr->v_read.clear(), sr->v_first.clear(), sr->v_refw.clear(), sr->v_flags.clear();
        const uint64_t *out_key = nullptr;
        const uint32_t *out_cnt = nullptr;
        size_t out_np = 0;
        if (vd.any) {
            // region index -> contig position: the merged key order of the contig's weight map is by descending region
            // start (regions are listed right to left, main.rs:1613-1620), read index within a region.  (Read back through
            // a staging block of its own: the pairs are still where the vote's read-back left them, in the context's.)
            std::vector<uint32_t> start(sr->run.n_reg);
            if (sr->run.n_reg) {
                PinnedBlock tmp((size_t)sr->run.n_reg * 4 + 64); // (NP2_E_NOMEM on failure; given back on every path)
                op_d2h(cx, tmp.p, cx->lq_start.p, (size_t)sr->run.n_reg * 4);
                op_sync(cx);
                memcpy(start.data(), tmp.p, (size_t)sr->run.n_reg * 4);
            }
            out_np = (size_t)vd.n_pairs();
            if (vd.view_key && vd.key_added) {
                // the pairs stay in the read-back staging: valid until this context's next read-back, i.e. the next np2_shard_*
                // call of this run (np2.h) — no host pass over them at all
                out_key = vd.view_key, out_cnt = vd.view_cnt;
            } else {
                const uint64_t *k = vd.keys();
                const uint32_t *cn = vd.cnts();
                sr->v_key.resize(out_np);
                for (size_t i = 0; i < out_np; ++i) sr->v_key[i] = k[i] + (vd.key_added ? 0 : add);
                sr->v_cnt.assign(cn, cn + out_np);
                out_key = sr->v_key.data(), out_cnt = sr->v_cnt.data();
            }
            for (uint32_t r = 0; r < vd.R; ++r) {
                const bool votes = vd.first_key[r] != 0xFFFFFFFFu;
                if (!votes && !vd.ref_seen[r] && !vd.bad[r]) continue;
                sr->v_read.push_back(shard_global_read(pl, r));
                sr->v_first.push_back(votes ? start[vd.first_key[r]] + pl.sub_lo : 0xFFFFFFFFu);
                sr->v_refw.push_back(vd.ref_w[r]);
                sr->v_flags.push_back((uint8_t)((votes ? 1 : 0) | (vd.ref_seen[r] ? 2 : 0) | (vd.bad[r] ? 4 : 0)));
            }
        }
        out->n_pairs = out_np;
        out->pair_key = out_key;
        out->pair_cnt = out_cnt;
        out->n_reads = (uint32_t)sr->v_read.size();
        out->read_id = sr->v_read.data();
        out->first_pos = sr->v_first.data();
        out->ref_w = sr->v_refw.data();
        out->flags = sr->v_flags.data();
        // The decision is taken elsewhere — votes gathered, merged, Louvain: ~90 ms for a diploid chromosome — and the device
        // has nothing to do meanwhile: as in polish_impl the next pass starts at once on the reads the vote kernel has
        // flagged, and np2_shard_apply settles it.  Only kernels are issued here, no read-back: the exported pairs stay
        // valid where they are.
        sr->spec_n_bad = run_start_on_flagged(sr->run, vd);
        sr->spec = sr->spec_n_bad != 0;
        if (sr->spec) sr->spec_bad = vd.bad;
        if (cx->hooks.shard_spec_log)
            fprintf(stderr, "[np2 shard] vote: any %d, flags on the device %d, early start %d (%zu flagged)\n", (int)vd.any, vd.d_bad != nullptr, (int)sr->spec, sr->spec_n_bad);
        return NP2_OK;
    }, ctx_sink(cx));
}

int np2_shard_apply(np2_shard_run_t *h, const uint32_t *losers, uint32_t n) {
    ShardRun *sr = (ShardRun *)h;
    if (!sr || (n && !losers) || (sr->run.final_pass() && !sr->spec)) return NP2_E_ARG; // (a pass started early has advanced the counter)
    np2_ctx *cx = sr->run.cx;
    return abi_guard([&] {
        std::vector<uint32_t> local;
        const np2_shard_plan_t &pl = sr->plan;
        for (uint32_t i = 0; i < n; ++i) {
            if (losers[i] == 0) throw Np2Error(NP2_E_REFPANIC, "reference would panic: the contig itself was voted out");
            if (losers[i] >= pl.read_lo && losers[i] < pl.read_hi) local.push_back(losers[i] - pl.read_lo + 1);
        }
        if (sr->spec) { // the pass is under way on the flagged reads (np2_shard_vote): is it the right one?
            sr->spec = false;
            (void)run_settle_flagged(sr->run, sr->spec_bad, sr->spec_n_bad, local); // (if not, run_pass_front starts it again)
            return NP2_OK;
        }
        // (no identical-pass reuse across shards: a neighbour's removals are not visible here, the decision would
        // differ from shard to shard only in cost, never in result — but keep it simple)
        run_apply_losers(sr->run, local);
        if (n) sr->run.reuse = false;
        return NP2_OK;
    }, ctx_sink(cx));
}

int np2_shard_final(np2_shard_run_t *h, uint8_t **out_bases, uint32_t **out_pos, uint64_t *out_len) {
    ShardRun *sr = (ShardRun *)h;
    if (!sr || !out_bases || !out_pos || !out_len || !sr->run.final_pass()) return NP2_E_ARG;
    np2_ctx *cx = sr->run.cx;
    ResultOut r;
    const int rc = abi_guard([&] {
        run_final_pass(sr->run, r);
        const np2_shard_plan_t &pl = sr->plan;
        shard_check_stuck(sr);
        // keep the owned interval (+ the verification margin), in contig coordinates
        const uint32_t lo = pl.own_lo > sr->verify ? pl.own_lo - sr->verify : 0u;
        const uint64_t hi = (uint64_t)pl.own_hi + sr->verify;
        uint64_t w = 0;
        for (uint64_t i = 0; i < r.len; ++i) {
            const uint64_t gp = (uint64_t)r.pos[i] + pl.sub_lo;
            if (gp < lo || gp >= hi) continue;
            r.bases[w] = r.bases[i];
            r.pos[w] = (uint32_t)gp;
            ++w;
        }
        r.len = w;
        return NP2_OK;
    }, ctx_sink(cx));
    if (rc != NP2_OK) {
        r.release();
        return rc;
    }
    *out_bases = r.bases;
    *out_pos = r.pos;
    *out_len = r.len;
    return NP2_OK;
}

int np2_shard_final_device(np2_shard_run_t *h, np2_shard_piece_t *out) {
    ShardRun *sr = (ShardRun *)h;
    if (!sr || !out || !sr->run.final_pass()) return NP2_E_ARG;
    np2_ctx *cx = sr->run.cx;
    memset(out, 0, sizeof *out);
    void *blocks[4] = {nullptr, nullptr, nullptr, nullptr}; // (the pinned strips: given back unless handed out)
    const int rc = abi_guard([&] {
        ResultOut r;
        r.want_bases = false, r.want_pos = false; // the polished sub-contig stays on the device
        run_final_pass(sr->run, r);
        shard_check_stuck(sr);
        const np2_shard_plan_t &pl = sr->plan;
        const uint32_t v = sr->verify;
        // positions in sub-contig coordinates; the consensus is ordered by position
        auto sub = [&](uint64_t p) -> uint32_t { return p <= pl.sub_lo ? 0u : (uint32_t)std::min<uint64_t>(p - pl.sub_lo, 0xFFFFFFFFull); };
        const uint32_t t[6] = {sub(pl.own_lo > v ? pl.own_lo - v : 0u), sub(pl.own_lo), sub((uint64_t)pl.own_lo + v),
                               sub(pl.own_hi > v ? pl.own_hi - v : 0u), sub(pl.own_hi), sub((uint64_t)pl.own_hi + v)};
        cx->shard_bounds.ensure(8);
        const uint32_t *M_p = cx->mlen.p; // (a device copy of the final length: any buffer holding it will do)
        {
            // the final length is known on the host (fetch_result read it back): stage it next to the bounds
            const uint32_t Mh = (uint32_t)cx->last_len;
            cx->mlen.ensure(32);
            h2d_staged(cx, cx->mlen.p + 31, &Mh, 4);
            M_p = cx->mlen.p + 31;
        }
        launch_shard_bounds(cx->stream, cx->last_dpos, M_p, t, cx->shard_bounds.p);
        const std::vector<uint32_t> b = d2h(cx, cx->shard_bounds.p, 8);
        sr->own_off = b[1];
        sr->own_len = b[4] - b[1];
        sr->have_piece = true;
        out->own_len = sr->own_len;
        out->dev_bases = cx->last_dbase + b[1];
        out->dev_pos = cx->last_dpos + b[1];
        out->first_pos = b[6] + pl.sub_lo;
        out->last_pos = b[7] + pl.sub_lo;
        out->lo_len = b[2] - b[0];
        out->hi_len = b[5] - b[3];
        auto strip = [&](uint32_t i0, uint32_t n, uint8_t *&hb, uint32_t *&hp, int slot) {
            if (!n) return;
            hb = (uint8_t *)(blocks[slot] = pinned_pool().get((size_t)n + 1));
            hp = (uint32_t *)(blocks[slot + 1] = pinned_pool().get(((size_t)n + 1) * 4));
            if (!hb || !hp) throw Np2Error(NP2_E_NOMEM, "pinned strip allocation failed");
            op_d2h(cx, hb, cx->last_dbase + i0, n);
            op_d2h(cx, hp, cx->last_dpos + i0, (size_t)n * 4);
        };
        strip(b[0], out->lo_len, out->lo_bases, out->lo_pos, 0);
        strip(b[3], out->hi_len, out->hi_bases, out->hi_pos, 2);
        op_sync(cx);
        for (uint32_t i = 0; i < out->lo_len; ++i) out->lo_pos[i] += pl.sub_lo;
        for (uint32_t i = 0; i < out->hi_len; ++i) out->hi_pos[i] += pl.sub_lo;
        flush_timings(cx); // (np2_last_timings: the stage timers of the whole run, the dense pass of np2_shard_begin included)
        return NP2_OK;
    }, ctx_sink(cx));
    if (rc != NP2_OK)
        for (void *p : blocks)
            if (p) pinned_pool().put(p);
    return rc;
}

int np2_shard_fetch(np2_shard_run_t *h, uint8_t *dst_bases, uint32_t *dst_pos) {
    ShardRun *sr = (ShardRun *)h;
    if (!sr || !dst_bases || !sr->have_piece) return NP2_E_ARG;
    np2_ctx *cx = sr->run.cx;
    return abi_guard([&] {
        HIPCHK(hipSetDevice(cx->device));
        if (!cx->last_dbase) throw Np2Error(NP2_E_ARG, "the shard's device result is gone (another call used its context)");
        if (sr->own_len) {
            op_d2h(cx, dst_bases, cx->last_dbase + sr->own_off, sr->own_len);
            if (dst_pos) op_d2h(cx, dst_pos, cx->last_dpos + sr->own_off, sr->own_len * 4);
            op_sync(cx);
            if (dst_pos) {
                const uint32_t add = sr->plan.sub_lo;
                if (add)
                    for (uint64_t i = 0; i < sr->own_len; ++i) dst_pos[i] += add;
            }
        }
        return NP2_OK;
    }, ctx_sink(cx));
}

} // extern "C"
