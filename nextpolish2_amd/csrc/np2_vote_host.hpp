#pragma once
// Host half of the phasing vote (phase_reads_by_lqseqs, main.rs:948-1015): what a pass hands over (VoteData), the merge of
// the shards' votes (vote_merge), the rows form of a vote from its pair list (vote_rows_from_pairs) and the decision
// (vote_decide: the weight maps in the reference's key-creation order, then the Louvain of np2_phase_host.hpp).
// Host-only and threaded: no HIP, no context, so that a plain C++ compiler builds it and a program of its own runs it
// under the sanitizers (tests/tools/vote_host_test.cpp).  The device half is vote_collect (np2_vote.cpp).
#include "../../include/np2.h"
#include "np2_abi.hpp"
#include "np2_phase_host.hpp"
#include "np2_vote_band.hpp"

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <future>
#include <utility>
#include <vector>

namespace np2h {

using namespace np2;

// What one phasing pass hands to the host side of the vote.  Everything in it is additive over the HETE regions it was
// collected from, so the shards of one contig (np2_shard_*) each collect theirs over the regions they own and the
// contig's owner merges them before the Louvain.
struct VoteData {
    uint32_t R = 0;                   // reads of the (sub-)contig, local numbering
    bool any = false;                 // false: no read votes anywhere, nobody can lose
    std::vector<uint64_t> pair_key;   // a << 32 | b (a < b), ascending
    std::vector<uint32_t> pair_cnt;   // HETE regions in which the pair agrees | disagrees << 16
    // ... or, instead of the two vectors, a view of a caller's arrays (np2_vote_decide with one sorted vote: a
    // chromosome's pair list is 200 MB, not to be copied for nothing)
    const uint64_t *view_key = nullptr;
    const uint32_t *view_cnt = nullptr;
    uint64_t view_n = 0;
    // ... or the finished adjacency rows of the plain pipeline (k_vote_rows_emit: row v of the vote's graph = edges
    // [off[v], off[v + 1]), its partners below it, then those above it, flagged reads already left out unless every read
    // is used), again a view of the staging; n_nokey: pairs with an endpoint that never voted (an internal error)
    const uint32_t *off = nullptr;
    const phase::Graph::Edge *edges = nullptr;
    uint32_t n_nokey = 0;
    std::vector<uint32_t> off_own;
    std::vector<phase::Graph::Edge> edges_own;
    bool rows() const { return off != nullptr; }
    const uint64_t *keys() const { return view_key ? view_key : pair_key.data(); }
    const uint32_t *cnts() const { return view_key ? view_cnt : pair_cnt.data(); }
    uint64_t n_pairs() const { return view_key ? view_n : (uint64_t)pair_key.size(); } // (not of the rows form)
    void own() { // copy a view into the vectors (the viewed memory is about to be reused)
        if (rows() && off_own.empty()) {
            off_own.assign(off, off + R + 1);
            edges_own.assign(edges, edges + off[R]);
            off = off_own.data(), edges = edges_own.data();
        }
        if (!view_key) return;
        pair_key.assign(view_key, view_key + view_n);
        pair_cnt.assign(view_cnt, view_cnt + view_n);
        view_key = nullptr, view_cnt = nullptr, view_n = 0;
    }
    std::vector<uint32_t> first_key;  // per read: creation rank of its key in the reference's weight map = index of the
                                      // first HETE region it votes in (0xFFFFFFFF: none); shards: see vote_merge
    std::vector<int32_t> ref_w;       // per read: summed weight against the contig's own candidate (ref_data[0])
    std::vector<uint8_t> ref_seen, bad;
    const uint8_t *d_bad = nullptr;   // the `bad` flags where the vote kernel left them on the device (until the next vote)
    bool key_added = false;           // (wide form) the pair keys already carry the shard's read-number shift
};

// data weight of a pair from its packed counts (agree | disagree << 16) = sum(w), unless the pair disagrees in 3 or more
// regions: then -(#disagreements) (dif <= -3 overwrites, main.rs:996-1002)
inline float pair_weight(uint32_t cnt) {
    const int32_t same = (int32_t)(cnt & 0xFFFFu), neg = (int32_t)(cnt >> 16);
    return (float)(neg >= 3 ? -neg : same - neg);
}
// the packed counts of one pair from two shards, added half by half -> false: a half outgrows its 16 bits
inline bool add_pair_counts(uint32_t a, uint32_t b, uint32_t &out) {
    const uint32_t same = (a & 0xFFFFu) + (b & 0xFFFFu), neg = (a >> 16) + (b >> 16);
    if (same > 0xFFFFu || neg > 0xFFFFu) return false;
    out = same | (neg << 16);
    return true;
}

// The rows form of a vote from its sorted pair list, on the host: a plain serial restatement of what k_vote_rows_count /
// the row-total scan / k_vote_rows_emit deliver (np2_regions.hip), and the model those kernels are tested against.
// Row v = partners below v ascending, then partners above v ascending; weight: pair_weight; unless every read is used, a
// flagged read has an empty row and appears in none; pairs with an endpoint that never voted are counted, not listed.
// -> false: the list is not sorted by (a, b) with a < b, or a pair lies outside the band (b - a - 1 >= EDGE_BAND) — the
// kernels' band does not hold such a vote.
inline bool vote_rows_from_pairs(VoteData &vd, bool use_all) {
    const uint32_t R = vd.R;
    const uint64_t *k = vd.keys();
    const uint32_t *cn = vd.cnts();
    const uint64_t np = vd.n_pairs();
    std::vector<uint32_t> n_lo(R, 0), n_up(R, 0);
    uint32_t nokey = 0;
    auto listed = [&](uint64_t i, uint32_t &a, uint32_t &b) { // is pair i an edge of the rows?
        a = (uint32_t)(k[i] >> 32), b = (uint32_t)k[i];
        if (a >= R || b >= R || vd.first_key[a] == 0xFFFFFFFFu || vd.first_key[b] == 0xFFFFFFFFu) return false;
        return use_all || !(vd.bad[a] | vd.bad[b]);
    };
    for (uint64_t i = 0; i < np; ++i) {
        uint32_t a = (uint32_t)(k[i] >> 32), b = (uint32_t)k[i];
        if (b <= a || b - a - 1 >= EDGE_BAND || (i && k[i - 1] >= k[i])) return false;
        if (a >= R || b >= R || vd.first_key[a] == 0xFFFFFFFFu || vd.first_key[b] == 0xFFFFFFFFu) ++nokey;
        if (listed(i, a, b)) ++n_lo[b], ++n_up[a];
    }
    vd.off_own.assign((size_t)R + 1, 0);
    std::vector<uint32_t> cur_lo(R), cur_up(R);
    for (uint32_t v = 0; v < R; ++v) {
        cur_lo[v] = vd.off_own[v], cur_up[v] = vd.off_own[v] + n_lo[v];
        vd.off_own[v + 1] = cur_up[v] + n_up[v];
    }
    vd.edges_own.resize(vd.off_own[R]);
    for (uint64_t i = 0; i < np; ++i) {
        uint32_t a, b;
        if (!listed(i, a, b)) continue;
        const float w = pair_weight(cn[i]);
        vd.edges_own[cur_lo[b]++] = phase::Graph::Edge(a, w);
        vd.edges_own[cur_up[a]++] = phase::Graph::Edge(b, w);
    }
    vd.off = vd.off_own.data(), vd.edges = vd.edges_own.data(), vd.n_nokey = nokey;
    return true;
}

// The votes of a contig's shards as ONE vote in contig-wide read numbers.  Per read: weights against the contig's own
// candidate add up, flags are or-ed, the first vote is the rightmost HETE region over all shards.  Every shard's pairs
// arrive sorted by key (a << 32 | b): the contig's list is their merge, the counts of a pair that shares regions of two
// shards added up before the weight rule is applied (main.rs:996-1002).  Neighbouring shards share only the reads of
// their halos, so a merge step is mostly two block copies.  A single sorted vote is not copied: `out` views the caller's
// arrays.  -> NP2_OK; NP2_E_ARG: a read id or a pair's endpoint outside the contig's reads; NP2_E_UNSUPPORTED: a pair's
// counts outgrow 16 bits.
inline int vote_merge(const np2_vote_t *votes, int n_votes, uint32_t n_reads_total, VoteData &out) {
    VoteData &vd = out;
    vd = VoteData();
    vd.R = n_reads_total;
    vd.first_key.assign(n_reads_total, 0xFFFFFFFFu);
    vd.ref_w.assign(n_reads_total, 0);
    vd.ref_seen.assign(n_reads_total, 0);
    vd.bad.assign(n_reads_total, 0);
    std::vector<uint32_t> first_pos(n_reads_total, 0);
    std::vector<uint8_t> votes_any(n_reads_total, 0);
    std::vector<uint64_t> mk, tk;
    std::vector<uint32_t> mc, tc;
    for (int v = 0; v < n_votes; ++v) {
        const np2_vote_t &x = votes[v];
        for (uint32_t i = 0; i < x.n_reads; ++i) {
            const uint32_t r = x.read_id[i];
            if (r >= n_reads_total) return NP2_E_ARG;
            vd.any = true;
            vd.ref_w[r] += x.ref_w[i];
            if (x.flags[i] & 2) vd.ref_seen[r] = 1;
            if (x.flags[i] & 4) vd.bad[r] = 1;
            if (x.flags[i] & 1) { // the read's first vote = its rightmost HETE region over all shards
                if (!votes_any[r] || x.first_pos[i] > first_pos[r]) first_pos[r] = x.first_pos[i];
                votes_any[r] = 1;
            }
        }
        if (!x.n_pairs) continue;
        // (the keys arrive from other ranks: both endpoints index per-read arrays below; unsorted input is sorted here)
        std::vector<uint64_t> sk;
        std::vector<uint32_t> sc;
        const uint64_t *xk = x.pair_key;
        const uint32_t *xc = x.pair_cnt;
        bool sorted = true;
        { // (2 x 10^7 pairs for a chromosome: on all threads)
            std::vector<uint8_t> st(phase::host_threads(), 0); // bit 0: an endpoint outside the contig's reads, bit 1: unsorted
            phase::parallel_ranges((size_t)x.n_pairs, (size_t)1 << 18, [&](unsigned t, size_t lo, size_t hi) {
                uint8_t f = 0;
                for (size_t i = lo; i < hi; ++i) {
                    if ((uint32_t)(xk[i] >> 32) >= n_reads_total || (uint32_t)xk[i] >= n_reads_total) f |= 1;
                    if (i && !(xk[i - 1] < xk[i])) f |= 2;
                }
                st[t] = f;
            });
            for (uint8_t f : st) {
                if (f & 1) return NP2_E_ARG;
                if (f & 2) sorted = false;
            }
        }
        if (!sorted) {
            std::vector<std::pair<uint64_t, uint32_t>> tmp(x.n_pairs);
            for (uint64_t i = 0; i < x.n_pairs; ++i) tmp[i] = {xk[i], xc[i]};
            std::sort(tmp.begin(), tmp.end());
            for (auto &t : tmp) {
                if (!sk.empty() && sk.back() == t.first) {
                    if (!add_pair_counts(sc.back(), t.second, sc.back())) return NP2_E_UNSUPPORTED;
                } else {
                    sk.push_back(t.first);
                    sc.push_back(t.second);
                }
            }
            xk = sk.data(), xc = sc.data();
        }
        const size_t nx = sorted ? (size_t)x.n_pairs : sk.size();
        if (n_votes == 1 && sorted) { // the caller's arrays as they are
            vd.view_key = xk, vd.view_cnt = xc, vd.view_n = nx;
            continue;
        }
        if (mk.empty()) {
            mk.assign(xk, xk + nx);
            mc.assign(xc, xc + nx);
            continue;
        }
        // merge (mk, mc) with (xk, xc): the part of mk below xk[0] and the part of xk above mk.back() are copied en bloc
        tk.clear(), tc.clear();
        tk.reserve(mk.size() + nx), tc.reserve(mk.size() + nx);
        size_t i = (size_t)(std::lower_bound(mk.begin(), mk.end(), xk[0]) - mk.begin()), j = 0;
        tk.insert(tk.end(), mk.begin(), mk.begin() + (long)i);
        tc.insert(tc.end(), mc.begin(), mc.begin() + (long)i);
        while (i < mk.size() && j < nx) {
            if (mk[i] < xk[j]) {
                tk.push_back(mk[i]), tc.push_back(mc[i]), ++i;
            } else if (xk[j] < mk[i]) {
                tk.push_back(xk[j]), tc.push_back(xc[j]), ++j;
            } else {
                uint32_t sum;
                if (!add_pair_counts(mc[i], xc[j], sum)) return NP2_E_UNSUPPORTED;
                tk.push_back(mk[i]), tc.push_back(sum), ++i, ++j;
            }
        }
        tk.insert(tk.end(), mk.begin() + (long)i, mk.end());
        tc.insert(tc.end(), mc.begin() + (long)i, mc.end());
        tk.insert(tk.end(), xk + j, xk + nx);
        tc.insert(tc.end(), xc + j, xc + nx);
        mk.swap(tk), mc.swap(tc);
    }
    if (!vd.view_key) {
        vd.pair_key.swap(mk);
        vd.pair_cnt.swap(mc);
    }
    for (uint32_t r = 0; r < n_reads_total; ++r)
        if (votes_any[r]) vd.first_key[r] = 0xFFFFFFFEu - first_pos[r]; // ascending = right to left
    return NP2_OK;
}

// What a decision reports beside its losers: its wall time (the "wall_louvain" entry of the caller's timings) and, when
// asked for (a tracing context), the graph it was taken on, whichever path built it ("vote.row_off" / "vote.rows")
struct VoteDecideInfo {
    double ms = 0;
    bool want_graph = false;
    std::vector<uint32_t> row_off;
    std::vector<phase::Graph::Edge> rows;
};
inline double vote_clock_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Host part of the vote: rebuild the weight maps in the reference's key-creation order, then Louvain
// (louvain.rs:290-356).  Outer keys of `data` are created region by region (index order), valid non-ref candidates in
// position (= read index) order, first occurrence wins.  -> the losers, ascending, each once.
inline std::vector<uint32_t> vote_decide(const VoteData &vd, bool use_all, VoteDecideInfo *info = nullptr) {
    if (!vd.any) return {};
    const uint32_t R = vd.R;
    const uint64_t NU = vd.rows() ? 0 : vd.n_pairs();
    const uint32_t *const pair_cnt = vd.rows() ? nullptr : vd.cnts();
    const double t_host0 = vote_clock_ms();
    // reads with a key, by (creation rank, read): the reads come in read order, so a STABLE sort by rank alone does it —
    // two 16-bit counting passes (a comparison sort of a chromosome's 3 x 10^5 keys was 12 ms)
    std::vector<std::pair<uint32_t, uint32_t>> keys;
    for (uint32_t r = 0; r < R; ++r)
        if (vd.first_key[r] != 0xFFFFFFFFu) keys.emplace_back(vd.first_key[r], r);
    if (keys.size() < 4096) {
        std::sort(keys.begin(), keys.end());
    } else {
        std::vector<std::pair<uint32_t, uint32_t>> tmp(keys.size());
        std::vector<uint32_t> cnt(65537);
        for (int pass = 0; pass < 2; ++pass) {
            const int sh = 16 * pass;
            std::fill(cnt.begin(), cnt.end(), 0u);
            for (const auto &k : keys) ++cnt[((k.first >> sh) & 0xFFFFu) + 1];
            for (size_t i = 0; i < 65536; ++i) cnt[i + 1] += cnt[i];
            for (const auto &k : keys) tmp[cnt[(k.first >> sh) & 0xFFFFu]++] = k;
            keys.swap(tmp);
        }
    }
    const bool prof = getenv("NP2_PHASE_PROFILE") != nullptr;
    double t_mark = t_host0;
    auto mark = [&](const char *what) {
        if (prof) {
            const double t = vote_clock_ms();
            fprintf(stderr, "  vote host: %s %.2f ms\n", what, t - t_mark);
            t_mark = t;
        }
    };
    phase::Graph data;
    data.reserve_ids(R);
    mark("key order");
    for (auto &k : keys) data.add_key(k.second);
    mark("key table");
    // data.retain(..) + per-row retain (main.rs:1004-1010) drop the reads flagged bad and every edge pointing at one:
    // those edges are left out while the rows are built (the rows' relative order is all that is kept of them); rows
    // that arrive finished (the plain pipeline's) have left them out already
    // data.retain(..) on the keys themselves (erase order = bucket order) BEFORE the rows: the rows leave the flagged reads'
    // edges out by themselves, and with the key table final the first level's community map — the keys inserted into a
    // fresh map in the table's iteration order, 10 ms of hash-order emulation for a chromosome — is built on a helper
    // thread beside the rows
    std::vector<uint32_t> bad;
    for (uint32_t r = 0; r < R; ++r)
        if (vd.bad[r]) bad.push_back(r);
    if (!use_all) data.keys.keep_if([&](uint32_t k, phase::Nil &) { return !vd.bad[k]; }); // (is_key follows after the rows: they check their endpoints against it)
    mark("retain");
    std::future<phase::OrderSet> communities;
    if (data.keys.size() >= (1u << 15) && phase::host_threads() > 1)
        communities = std::async(std::launch::async, [&data] { return phase::SignedLouvain::first_communities(data.keys); });
    bool ok = false;
    try {
        if (vd.rows()) {
            ok = vd.n_nokey == 0;
            if (ok) data.adopt_rows(vd.off, vd.edges, R); // (borrowed: vd outlives the decision)
        } else {
            ok = data.add_edges_sorted(vd.keys(), NU, [&](uint64_t i) { return pair_weight(pair_cnt[i]); },
                                       use_all ? nullptr : vd.bad.data());
        }
    } catch (...) {
        if (communities.valid()) communities.wait(); // (it reads data.keys)
        throw;
    }
    phase::OrderSet comm_pre;
    if (communities.valid()) comm_pre = communities.get();
    const bool have_pre = !comm_pre.empty();
    if (!ok) throw Np2Error(NP2_E_DEVICE, "internal: edge endpoint without a key");
    if (!use_all)
        for (uint32_t b : bad) data.is_key[b] = 0;
    mark("keys + edges");
    if (info && info->want_graph) {
        info->row_off = data.off;
        const phase::Graph::Edge *e0 = data.n_ids() ? data.adj(0).b : nullptr;
        info->rows.assign(e0, e0 + (e0 ? data.n_edges() : 0));
    }
    std::vector<float> ref_row(R, 0.f);
    std::vector<uint8_t> ref_have(R, 0);
    bool have_ref = false;
    for (uint32_t r = 0; r < R; ++r)
        if (vd.ref_seen[r]) {
            ref_row[r] = (float)vd.ref_w[r];
            ref_have[r] = 1;
            have_ref = true;
        }
    std::vector<uint32_t> losers;
    if (!phase::losing_reads(std::move(data), have_ref, ref_row, ref_have, losers, have_pre ? &comm_pre : nullptr))
        throw Np2Error(NP2_E_REFPANIC,
                       "reference would panic: the weight of two conflicting community is not less than 0");
    mark("louvain + ranking");
    if (info) info->ms = vote_clock_ms() - t_host0;
    // ascending, each once (flags over the read ids: a comparison sort of a chromosome's 3 x 10^5 losers was 12 ms)
    std::vector<uint8_t> lost(R, 0);
    for (uint32_t b : bad) lost[b] = 1;
    for (uint32_t l : losers)
        if (l < R) lost[l] = 1;
        else throw Np2Error(NP2_E_DEVICE, "internal: loser outside the contig's reads");
    losers.clear();
    for (uint32_t r = 0; r < R; ++r)
        if (lost[r]) losers.push_back(r);
    return losers;
}

} // namespace np2h
