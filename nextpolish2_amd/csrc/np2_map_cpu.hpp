// The mapper on the CPU, one sequence and one read at a time, from the rule's arithmetic in np2_map_core.hpp: what
// np2_map_host (np2_map_host.cpp) runs and what tests/tools/map_core_test.cpp builds with a plain C++ compiler.  No HIP here.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "np2_map_core.hpp"

namespace np2map {

struct Minimizer {
    uint64_t h, x;
};

// a separator stream -> the offsets of its separators ('\n'); false when its last byte is not one
inline bool stream_ends(const uint8_t *s, uint64_t n, std::vector<uint64_t> &ends) {
    ends.clear();
    if (n && s[n - 1] != '\n') return false;
    for (uint64_t at = 0; at < n;) {
        const uint8_t *e = (const uint8_t *)memchr(s + at, '\n', n - at);
        ends.push_back((uint64_t)(e - s));
        at = ends.back() + 1;
    }
    return true;
}

// a weight set in host memory: the listed canonical indices of k-mers of length k, ascending and unique (k = 0: empty)
struct WeightSet {
    uint32_t k = 0;
    std::vector<uint32_t> idx;
    bool empty() const { return idx.empty(); }
    bool listed(uint64_t v) const { return std::binary_search(idx.begin(), idx.end(), (uint32_t)v); }
};

// the minimizers of one sequence in ascending position, appended to `out` as (h, x) with x naming sequence `seq`; under a
// non-empty weight set `ws` (of length k) the window order is push_w's
inline void sketch_seq(const uint8_t *s, uint32_t n, uint32_t seq, uint32_t k, uint32_t w, std::vector<uint64_t> &words, std::vector<Minimizer> &out,
                       const WeightSet *ws = nullptr) {
    words.resize(n);
    Roll r;
    const uint64_t mask = kmer_mask(k);
    if (ws && ws->empty()) ws = nullptr;
    for (uint32_t i = 0; i < n; ++i)
        words[i] = ws ? push_w(r, s[i], k, mask, [&](uint64_t v) { return ws->listed(v); }) : push(r, s[i], k, mask);
    for (uint32_t i = 0; i < n; ++i) {
        auto at = [&](int32_t d) {
            const int64_t j = (int64_t)i + d;
            return j < 0 || j >= (int64_t)n ? W_BREAK : words[(size_t)j];
        };
        if (is_minimizer(at, w)) out.push_back({ws ? word_hash(words[i], mask) : words[i] >> 1, mz_x(seq, i, (uint32_t)(words[i] & 1u))});
    }
}

struct HostIndex {
    uint32_t k = 0, w = 0;
    std::vector<Minimizer> mz; // stably sorted by h from (sequence, position) order
    const WeightSet *ws = nullptr; // the caller's; reads are sketched under it too
    void build(const uint8_t *stream, const std::vector<uint64_t> &ends, uint32_t k_, uint32_t w_, const WeightSet *ws_ = nullptr) {
        k = k_, w = w_, ws = ws_;
        mz.clear();
        std::vector<uint64_t> words;
        uint64_t from = 0;
        for (size_t t = 0; t < ends.size(); ++t) {
            sketch_seq(stream + from, (uint32_t)(ends[t] - from), (uint32_t)t, k, w, words, mz, ws);
            from = ends[t] + 1;
        }
        std::stable_sort(mz.begin(), mz.end(), [](const Minimizer &a, const Minimizer &b) { return a.h < b.h; });
    }
};

struct ReadCounts {
    uint64_t minimizers = 0, anchors = 0, dropped_occ = 0;
};

// one read's anchors in the rule's order, f and p of the recurrence, and the marks and bases finish_read leaves
struct ReadChains {
    std::vector<uint64_t> khi, klo;
    std::vector<int32_t> f, p, base;
    std::vector<uint8_t> mark;
    // the (r, q) pairs of the n anchors that end at `last`, first to last, appended to `chain`
    void append_chain(std::vector<uint32_t> &chain, int32_t last, uint32_t n) const {
        const size_t at = chain.size();
        chain.resize(at + 2 * (size_t)n);
        uint32_t t = n;
        for (int32_t a = last; a >= 0 && t > 0; a = p[a]) {
            --t;
            chain[at + 2 * (size_t)t] = lo_r(klo[a]), chain[at + 2 * (size_t)t + 1] = lo_q(klo[a]);
        }
    }
};

// one read -> its hit (tid -1: unmapped) and what the chaining left in `rc`; returns the primary chain's last anchor or -1
inline int32_t chain_read(const HostIndex &ix, const uint8_t *s, uint32_t qlen, const Opts &o, Hit *hit, ReadChains &rc, ReadCounts *counts) {
    std::vector<uint64_t> words;
    std::vector<Minimizer> mz;
    sketch_seq(s, qlen, 0, o.k, o.w, words, mz, ix.ws);
    std::vector<std::pair<uint64_t, uint64_t>> an; // (hi, lo)
    for (const Minimizer &m : mz) {
        auto lo = std::lower_bound(ix.mz.begin(), ix.mz.end(), m.h, [](const Minimizer &a, uint64_t h) { return a.h < h; });
        auto hi = std::upper_bound(lo, ix.mz.end(), m.h, [](uint64_t h, const Minimizer &a) { return h < a.h; });
        const uint64_t occ = (uint64_t)(hi - lo);
        if (occ > o.max_occ) ++counts->dropped_occ;
        if (occ < 1 || occ > o.max_occ) continue;
        for (auto e = lo; e != hi; ++e) {
            uint64_t khi, klo;
            anchor_of(0, (uint32_t)(m.x & 0xFFFFFFFFu) >> 1, (uint32_t)(m.x & 1u), qlen, e->x, o.k, &khi, &klo);
            an.emplace_back(khi, klo);
        }
    }
    counts->minimizers += mz.size(), counts->anchors += an.size();
    std::sort(an.begin(), an.end());
    const uint32_t n = (uint32_t)an.size();
    std::vector<uint64_t> &khi = rc.khi, &klo = rc.klo;
    std::vector<int32_t> &f = rc.f, &p = rc.p;
    khi.resize(n), klo.resize(n), f.resize(n), p.resize(n), rc.base.resize(n), rc.mark.resize(n);
    for (uint32_t i = 0; i < n; ++i) khi[i] = an[i].first, klo[i] = an[i].second;
    int32_t best_f = 0;
    uint32_t end = 0;
    for (uint32_t i = 0; i < n; ++i) {
        int64_t best = NO_CAND;
        for (uint32_t d = 1; d <= o.lookback && d <= i; ++d) {
            const uint32_t j = i - d;
            best = std::max(best, candidate(khi[i], klo[i], khi[j], klo[j], f[j], j, o));
        }
        settle(best, o.k, &f[i], &p[i]);
        if (f[i] > best_f) best_f = f[i], end = i;
    }
    return finish_read(khi.data(), klo.data(), f.data(), p.data(), rc.mark.data(), rc.base.data(), n, end, qlen, o, hit);
}

// one read -> its hit (tid -1: unmapped) and, with `chain`, its primary chain's (r, q) pairs appended first to last
inline void map_read(const HostIndex &ix, const uint8_t *s, uint32_t qlen, const Opts &o, Hit *hit, std::vector<uint32_t> *chain, ReadCounts *counts) {
    ReadChains rc;
    const int32_t last = chain_read(ix, s, qlen, o, hit, rc, counts);
    if (chain && last >= 0) rc.append_chain(*chain, last, hit->n);
}

// one read -> its units (the rule: np2_io.h, "More chains"): hits[0] is map_read's hit, the kept further chains follow in
// selection order with their classes and parents; with `chain`, every unit's (r, q) pairs appended; returns the units
inline uint32_t map_read_m(const HostIndex &ix, const uint8_t *s, uint32_t qlen, const Opts &o, const MultiOpts &m, Hit *hits, uint32_t *cls,
                           uint32_t *parent, std::vector<uint32_t> *chain, ReadCounts *counts, MoreCounts *mc) {
    ReadChains rc;
    const int32_t last = chain_read(ix, s, qlen, o, &hits[0], rc, counts);
    cls[0] = CLS_PRIMARY, parent[0] = 0;
    if (last < 0) return 1;
    int32_t uend[MAX_CHAINS];
    Family fm;
    const uint32_t n = select_more(rc.khi.data(), rc.klo.data(), rc.f.data(), rc.p.data(), rc.mark.data(), rc.base.data(), (uint32_t)rc.khi.size(),
                                   qlen, o, m, hits[0], fm, hits + 1, cls + 1, parent + 1, uend, mc);
    if (chain) {
        rc.append_chain(*chain, last, hits[0].n);
        for (uint32_t u = 1; u < n; ++u) rc.append_chain(*chain, uend[u - 1], hits[u].n);
    }
    return n;
}

// one mapped read's PAF line, appended to `out`: columns 1 .. 12 and the tags
// (tp: P for a primary and a supplementary chain, S for a secondary one)
inline void paf_line(std::string &out, const char *qname, size_t qname_n, const Hit &h, const std::string &tname, uint64_t tlen, char tp = 'P') {
    char num[256];
    out.append(qname, qname_n);
    int m = snprintf(num, sizeof num, "\t%u\t%u\t%u\t%c\t", h.qlen, h.qs, h.qe, h.rev ? '-' : '+');
    out.append(num, (size_t)m);
    out += tname;
    m = snprintf(num, sizeof num, "\t%llu\t%u\t%u\t%u\t%u\t%u\ttp:A:%c\tcm:i:%u\ts1:i:%u\ts2:i:%u\n", (unsigned long long)tlen, h.ts, h.te,
                 h.matches, h.block, h.mapq, tp, h.n, h.s1, h.s2);
    out.append(num, (size_t)m);
}

} // namespace np2map
