// The mapper's rule as plain integer arithmetic without HIP types (the rule's text: include/np2_io.h, np2_map_*): byte ->
// 2-bit code -> rolled words -> (hash, strand) of the k-mer that ends at a byte, the minimizer test, an anchor's
// coordinates and sort keys, the chaining score, the two linear sweeps behind the primary chain, the mapping quality, and the
// further chains of a read: their selection, hits and classes.
// The same text is the kernels' inner step (np2_map.hip), the host mapper (np2_map_host: np2_map_host.cpp) and a
// stand-alone program (tests/tools/map_core_test.cpp).
#pragma once
#include <cstdint>

#include "np2_kcount_core.hpp" // hash64 (yak_hash64 = minimap2's hash64), NP2_KC_HD

namespace np2map {

static constexpr uint32_t K_MIN = 11, K_MAX = 28, W_MIN = 1, W_MAX = 64, LOOKBACK_MAX = 64;
static constexpr uint32_t MAX_SEQ = 0x7FFFFFFFu;  // a sequence's length: an end position and a strand bit share 32 bits
static constexpr uint32_t MAX_TID = 0x7FFFFFFFu;  // sequences of an index: tid and rel share 32 bits
static constexpr uint32_t MAX_OCC = 1u << 20, MAX_GAP = 1u << 30, MAX_BW = 1u << 20, MAX_CNT = 1u << 30;

struct Opts {
    uint32_t k, w, max_occ, lookback, max_gap, bandwidth, min_cnt, min_score;
};
// (the order of np2_map_hit_t)
struct Hit {
    int32_t tid;
    uint32_t qlen, qs, qe, rev, ts, te, matches, block, mapq, n, s1, s2;
};

// ---- sketch ----------------------------------------------------------------------------------------------------------------
// A byte's word: h << 1 | strand of the k-mer that ends there, W_PAL where that k-mer is its own reverse complement (in the
// run, never chosen), W_BREAK where no k-mer ends (no window holds the byte).  A hash has 2k <= 56 bits.  (Under weights the
// word carries an ordering key above the hash: push_w, below.)
static constexpr uint64_t W_BREAK = ~0ULL, W_PAL = ~0ULL - 1;

NP2_KC_HD uint32_t code(uint8_t ch) { // ACGT in either case; every other byte 4
    const uint32_t u = (uint32_t)(ch & 0xDFu) - (uint32_t)'A';
    const uint32_t VALID = 1u | 1u << 2 | 1u << 6 | 1u << 19; // A C G T
    const uint64_t CODES = 1ull << 4 | 2ull << 12 | 3ull << 38;
    if (u >= 32u || !((VALID >> u) & 1u)) return 4u;
    return (uint32_t)(CODES >> (2u * u)) & 3u;
}

struct Roll {
    uint64_t fw = 0, rv = 0;
    uint32_t l = 0; // bases since the last non-base, capped at k
};
NP2_KC_HD uint64_t kmer_mask(uint32_t k) { return (1ULL << (2u * k)) - 1ULL; }

NP2_KC_HD uint64_t push(Roll &r, uint8_t ch, uint32_t k, uint64_t mask) {
    const uint32_t c = code(ch);
    if (c >= 4u) {
        r.l = 0;
        return W_BREAK;
    }
    r.fw = ((r.fw << 2) | (uint64_t)c) & mask;
    r.rv = (r.rv >> 2) | ((uint64_t)(3u - c) << (2u * (k - 1u)));
    if (r.l < k) ++r.l;
    if (r.l < k) return W_BREAK;
    if (r.fw == r.rv) return W_PAL;
    return np2kc::hash64(r.fw < r.rv ? r.fw : r.rv, mask) << 1 | (r.fw > r.rv ? 1u : 0u);
}

// ---- weighted sketch (winnowmap -W) ----------------------------------------------------------------------------------------
// A weight set is a k-mer length kw in [KW_MIN, KW_MAX] and a set of canonical indices v = min(fw, rv).  A listed k-mer keeps
// its hash as its identity but is ordered by key = M - s(s(s(M - h))), s(y) = y * y >> 2k, M = 4^k - 1: the fixed-point form
// of x -> x^8 on [0, 1), mirrored because the smallest hash wins.  y <= M < 2^30, so y * y < 2^60 and s(y) <= M.
static constexpr uint32_t KW_MIN = 11, KW_MAX = 15;

NP2_KC_HD uint64_t weighted_key(uint64_t h, uint32_t k, uint64_t mask) {
    uint64_t y = mask - h;
    for (int i = 0; i < 3; ++i) y = (y * y) >> (2u * k);
    return mask - y;
}
// A byte's word under weights: key << (2k + 1) | h << 1 | strand.  key, h <= M < 2^30, so a word is below 2^(4k + 1) <= 2^61,
// under W_PAL and W_BREAK; is_minimizer's comparison of word >> 1 is the comparison of (key, h).
static_assert(4 * KW_MAX + 1 <= 61 && (1ULL << 61) < W_PAL, "a weighted word stays below W_PAL and W_BREAK");
NP2_KC_HD uint64_t word_hash(uint64_t word, uint64_t mask) { return (word >> 1) & mask; }

// listed(v): is the canonical index v in the set
template <class Listed> NP2_KC_HD uint64_t push_w(Roll &r, uint8_t ch, uint32_t k, uint64_t mask, Listed listed) {
    const uint32_t c = code(ch);
    if (c >= 4u) {
        r.l = 0;
        return W_BREAK;
    }
    r.fw = ((r.fw << 2) | (uint64_t)c) & mask;
    r.rv = (r.rv >> 2) | ((uint64_t)(3u - c) << (2u * (k - 1u)));
    if (r.l < k) ++r.l;
    if (r.l < k) return W_BREAK;
    if (r.fw == r.rv) return W_PAL;
    const uint64_t v = r.fw < r.rv ? r.fw : r.rv, h = np2kc::hash64(v, mask);
    const uint64_t key = listed(v) ? weighted_key(h, k, mask) : h;
    return key << (2u * k + 1u) | h << 1 | (r.fw > r.rv ? 1u : 0u);
}

// at(d): the word of the byte d places from the candidate (d in [-(w - 1), w - 1]; W_BREAK beyond the sequence).  The
// candidate is the leftmost minimum of some window of w k-mers of its run: L left neighbours are larger, R right
// neighbours are not smaller, and L + R + 1 >= w.
template <class At> NP2_KC_HD bool is_minimizer(At at, uint32_t w) {
    const uint64_t me = at(0);
    if (me >= W_PAL) return false;
    const uint64_t h = me >> 1;
    uint32_t L = 0, R = 0;
    while (L + 1 < w) {
        const uint64_t x = at(-(int32_t)(L + 1));
        if (x == W_BREAK || (x >> 1) <= h) break;
        ++L;
    }
    while (L + R + 1 < w) {
        const uint64_t x = at((int32_t)(R + 1));
        if (x == W_BREAK || (x >> 1) < h) break;
        ++R;
    }
    return L + R + 1 >= w;
}

// a minimizer as the index and the seeding keep it: x = sequence << 32 | end position << 1 | strand
NP2_KC_HD uint64_t mz_x(uint32_t seq, uint32_t end, uint32_t strand) { return (uint64_t)seq << 32 | (uint64_t)end << 1 | strand; }

// ---- anchors ---------------------------------------------------------------------------------------------------------------
// An anchor's two sort keys: hi = read << 32 | rel << 31 | tid, lo = r << 32 | q.  Ascending (hi, lo) is read order and,
// inside a read, the rule's order (rel, tid, r, q).
NP2_KC_HD uint64_t key_hi(uint32_t read, uint32_t rel, uint32_t tid) { return (uint64_t)read << 32 | (uint64_t)rel << 31 | tid; }
NP2_KC_HD uint64_t key_lo(uint32_t r, uint32_t q) { return (uint64_t)r << 32 | q; }
NP2_KC_HD uint32_t hi_rel(uint64_t hi) { return (uint32_t)(hi >> 31) & 1u; }
NP2_KC_HD uint32_t hi_tid(uint64_t hi) { return (uint32_t)hi & 0x7FFFFFFFu; }
NP2_KC_HD uint32_t lo_r(uint64_t lo) { return (uint32_t)(lo >> 32); }
NP2_KC_HD uint32_t lo_q(uint64_t lo) { return (uint32_t)lo; }

// read minimizer (end position `end`, strand `qs`) x index entry x -> the anchor's keys
NP2_KC_HD void anchor_of(uint32_t read, uint32_t end, uint32_t qs, uint32_t qlen, uint64_t x, uint32_t k, uint64_t *hi, uint64_t *lo) {
    const uint32_t rel = qs ^ (uint32_t)(x & 1u);
    const uint32_t r = (uint32_t)(x & 0xFFFFFFFFu) >> 1;
    const uint32_t q = rel ? qlen - 1u - (end - (k - 1u)) : end;
    *hi = key_hi(read, rel, (uint32_t)(x >> 32));
    *lo = key_lo(r, q);
}

// ---- chain -----------------------------------------------------------------------------------------------------------------
NP2_KC_HD uint32_t ilog2_u32(uint32_t v) { // v > 0
    uint32_t l = 0;
    while (v >>= 1) ++l;
    return l;
}
static constexpr int64_t NO_CAND = INT64_MIN;
// candidate j for anchor i: f[j] + sc packed above j, so that the largest packed word is the best score and, of equal
// scores, the largest j; NO_CAND when j is not admissible.  Only the low 32 bits of hi (rel, tid) are compared: the caller
// offers anchors of one read.
NP2_KC_HD int64_t candidate(uint64_t hi_i, uint64_t lo_i, uint64_t hi_j, uint64_t lo_j, int32_t f_j, uint32_t j, const Opts &o) {
    if ((uint32_t)hi_i != (uint32_t)hi_j) return NO_CAND;
    const int64_t dr = (int64_t)lo_r(lo_i) - (int64_t)lo_r(lo_j), dq = (int64_t)lo_q(lo_i) - (int64_t)lo_q(lo_j);
    if (dr <= 0 || dr > (int64_t)o.max_gap || dq <= 0 || dq > (int64_t)o.max_gap) return NO_CAND;
    const int64_t dd = dr > dq ? dr - dq : dq - dr;
    if (dd > (int64_t)o.bandwidth) return NO_CAND;
    int64_t m = dr < dq ? dr : dq;
    if (m > (int64_t)o.k) m = o.k;
    const int64_t pen = dd * (int64_t)o.k / 100 + (dd > 0 ? (int64_t)(ilog2_u32((uint32_t)dd) >> 1) : 0);
    const int64_t v = (int64_t)f_j + m - pen;
    return v * ((int64_t)1 << 32) + (int64_t)j; // (v may be negative: no shift of a negative number)
}
// the best candidate's packed word -> f[i], p[i]
NP2_KC_HD void settle(int64_t best, uint32_t k, int32_t *f, int32_t *p) {
    *f = (int32_t)k, *p = -1;
    if (best == NO_CAND) return;
    const int64_t j = best & 0xFFFFFFFFLL, v = (best - j) / ((int64_t)1 << 32);
    if (v > (int64_t)k) *f = (int32_t)v, *p = (int32_t)j;
}

NP2_KC_HD uint32_t mapq_of(uint32_t s1, uint32_t s2, uint32_t n) {
    if (s1 == 0) return 0;
    const uint32_t d = s1 > s2 ? s1 - s2 : 0;
    const uint64_t q = (60ull * d / s1) * (n < 10 ? n : 10) / 10;
    return q > 60 ? 60u : (uint32_t)q;
}

// The two sweeps of one read, one lane: from f, p of its n_anchors anchors (hi, lo in the rule's order) and `end`, the
// smallest i with the largest f: mark the primary chain, sweep base[] over the unmarked anchors for s2, and fill the hit.
// mark and base are n_anchors scratch entries, every one of them written before it is read.  Returns the chain's last
// anchor (== end) for the export, or -1 for an unmapped read.
NP2_KC_HD int32_t finish_read(const uint64_t *hi, const uint64_t *lo, const int32_t *f, const int32_t *p, uint8_t *mark, int32_t *base,
                              uint32_t n_anchors, uint32_t end, uint32_t qlen, const Opts &o, Hit *out) {
    Hit h{};
    h.tid = -1, h.qlen = qlen;
    *out = h;
    if (n_anchors == 0) return -1;
    for (uint32_t i = 0; i < n_anchors; ++i) mark[i] = 0;
    uint32_t n = 0, matches = o.k, first = end;
    for (int32_t i = (int32_t)end; i >= 0; i = p[i]) {
        mark[i] = 1, ++n, first = (uint32_t)i;
        if (p[i] >= 0) {
            const uint32_t dr = lo_r(lo[i]) - lo_r(lo[p[i]]), dq = lo_q(lo[i]) - lo_q(lo[p[i]]);
            const uint32_t m = dr < dq ? dr : dq;
            matches += m < o.k ? m : o.k;
        }
    }
    int32_t s2 = 0;
    for (uint32_t i = 0; i < n_anchors; ++i) {
        if (mark[i]) continue;
        const int32_t pi = p[i];
        base[i] = pi < 0 ? 0 : mark[pi] ? f[pi] : base[pi];
        if (f[i] - base[i] > s2) s2 = f[i] - base[i];
    }
    const uint32_t s1 = (uint32_t)f[end];
    if (n < o.min_cnt || s1 < o.min_score) return -1;
    const uint32_t q0 = lo_q(lo[first]) - (o.k - 1u), q1 = lo_q(lo[end]) + 1u;
    h.tid = (int32_t)hi_tid(hi[end]);
    h.rev = hi_rel(hi[end]);
    h.qs = h.rev ? qlen - q1 : q0, h.qe = h.rev ? qlen - q0 : q1;
    h.ts = lo_r(lo[first]) - (o.k - 1u), h.te = lo_r(lo[end]) + 1u;
    h.matches = matches;
    h.block = h.qe - h.qs > h.te - h.ts ? h.qe - h.qs : h.te - h.ts;
    h.n = n, h.s1 = s1, h.s2 = (uint32_t)s2;
    h.mapq = mapq_of(s1, (uint32_t)s2, n);
    *out = h;
    return (int32_t)end;
}

// ---- more chains of a read (the rule: include/np2_io.h, "More chains") --------------------------------------------------------
// After finish_read: up to max_chains - 1 further selections over the unmarked anchors, each the largest f[i] - base[i] (of
// equal scores the smallest i) followed back through p while anchors are unmarked; the kept chains are classed against the
// parents before them on forward read coordinates.  The pieces below are what the kernel (k_map_chain_more: a wavefront's
// arg-max and block-wise re-sweep around them) and the host twin (select_more, one lane) share.
static constexpr uint32_t MAX_CHAINS = 16, NO_UNIT = 0xFFFFFFFFu;
static constexpr uint32_t CLS_PRIMARY = 0, CLS_SUPP = 1, CLS_SEC = 2;
struct MultiOpts {
    uint32_t max_chains, supplementary, secondary_n, mask_pm, pri_pm;
};
struct MoreCounts {
    uint32_t selections, dropped_cnt, dropped_pri, kept_supp, kept_sec;
};

NP2_KC_HD const char *check_multi(const MultiOpts &m) {
    if (m.max_chains < 1 || m.max_chains > MAX_CHAINS) return "max_chains must lie in 1 .. 16";
    if (m.supplementary > 1) return "supplementary must be 0 or 1";
    if (m.secondary_n > MAX_CHAINS - 1) return "secondary_n must lie in 0 .. 15";
    if (m.mask_pm < 1 || m.mask_pm > 1000) return "mask_pm must lie in 1 .. 1000";
    if (m.pri_pm > 1000) return "pri_pm must lie in 0 .. 1000";
    return nullptr;
}

// base of an unmarked anchor whose predecessor is pi, against the current marks (finish_read's sweep, one step)
NP2_KC_HD int32_t base_step(int32_t pi, const uint8_t *mark, const int32_t *f, const int32_t *base) {
    return pi < 0 ? 0 : mark[pi] ? f[pi] : base[pi];
}
// an unmarked anchor's selection key: the largest key is the largest score and, of equal scores, the smallest i
NP2_KC_HD int64_t more_key(int32_t score, uint32_t i) { return (int64_t)score * ((int64_t)1 << 32) + (int64_t)(0xFFFFFFFFu - i); }
NP2_KC_HD void more_unkey(int64_t key, int64_t *score, uint32_t *i) {
    const int64_t low = key & 0xFFFFFFFFLL;
    *score = (key - low) / ((int64_t)1 << 32), *i = 0xFFFFFFFFu - (uint32_t)low;
}

// The chain that ends at the unmarked anchor `end`, followed back through p while anchors are unmarked: its anchors are
// marked, and the hit is filled as finish_read fills the primary's, from the chain's own anchors, with s1 = score (s2 and
// mapq stay 0: classify and family_end set them).  Returns the chain's first anchor.
NP2_KC_HD uint32_t take_chain(const uint64_t *hi, const uint64_t *lo, const int32_t *p, uint8_t *mark, uint32_t end, uint32_t score, uint32_t qlen,
                              const Opts &o, Hit *out) {
    Hit h{};
    uint32_t n = 0, matches = o.k, first = end;
    for (int32_t i = (int32_t)end; i >= 0 && !mark[i]; i = p[i]) {
        mark[i] = 1, ++n, first = (uint32_t)i;
        if (p[i] >= 0 && !mark[p[i]]) {
            const uint32_t dr = lo_r(lo[i]) - lo_r(lo[p[i]]), dq = lo_q(lo[i]) - lo_q(lo[p[i]]);
            const uint32_t m = dr < dq ? dr : dq;
            matches += m < o.k ? m : o.k;
        }
    }
    const uint32_t q0 = lo_q(lo[first]) - (o.k - 1u), q1 = lo_q(lo[end]) + 1u;
    h.tid = (int32_t)hi_tid(hi[end]), h.qlen = qlen;
    h.rev = hi_rel(hi[end]);
    h.qs = h.rev ? qlen - q1 : q0, h.qe = h.rev ? qlen - q0 : q1;
    h.ts = lo_r(lo[first]) - (o.k - 1u), h.te = lo_r(lo[end]) + 1u;
    h.matches = matches;
    h.block = h.qe - h.qs > h.te - h.ts ? h.qe - h.qs : h.te - h.ts;
    h.n = n, h.s1 = score;
    *out = h;
    return first;
}

// A read's parents so far, the primary first: the interval on the forward read, the score, the largest score classed
// secondary to it, its kept secondaries, and its place among the read's units (NO_UNIT: a supplementary that is not reported).
struct Family {
    uint32_t n_par, n_units;
    uint32_t qs[MAX_CHAINS], qe[MAX_CHAINS], s1[MAX_CHAINS], s2[MAX_CHAINS], n_sec[MAX_CHAINS], unit[MAX_CHAINS];
};
NP2_KC_HD void family_begin(Family &fm, const Hit &primary) {
    fm.n_par = 1, fm.n_units = 1;
    fm.qs[0] = primary.qs, fm.qe[0] = primary.qe, fm.s1[0] = primary.s1, fm.s2[0] = primary.s2, fm.n_sec[0] = 0, fm.unit[0] = 0;
}
// A chain with min_cnt anchors or more, in selection order -> its class; *unit: its place among the read's units when it is
// kept, else NO_UNIT; *parent: the unit it is secondary to, or its own.  At most MAX_CHAINS - 1 chains follow a family_begin.
NP2_KC_HD uint32_t classify(Family &fm, const Hit &h, const MultiOpts &m, uint32_t *unit, uint32_t *parent) {
    const uint32_t len_c = h.qe - h.qs;
    for (uint32_t P = 0; P < fm.n_par; ++P) {
        const uint32_t a = h.qs > fm.qs[P] ? h.qs : fm.qs[P], b = h.qe < fm.qe[P] ? h.qe : fm.qe[P];
        const uint32_t ov = b > a ? b - a : 0, len_p = fm.qe[P] - fm.qs[P];
        if ((uint64_t)ov * 1000u <= (uint64_t)m.mask_pm * (len_c < len_p ? len_c : len_p)) continue;
        if (P > 0 && h.s1 > fm.s2[P]) fm.s2[P] = h.s1; // (the primary keeps finish_read's s2)
        const bool keep = fm.unit[P] != NO_UNIT && (uint64_t)h.s1 * 1000u >= (uint64_t)m.pri_pm * fm.s1[P] && fm.n_sec[P] < m.secondary_n;
        if (keep) ++fm.n_sec[P];
        *unit = keep ? fm.n_units++ : NO_UNIT, *parent = fm.unit[P];
        return CLS_SEC;
    }
    const uint32_t P = fm.n_par++;
    fm.qs[P] = h.qs, fm.qe[P] = h.qe, fm.s1[P] = h.s1, fm.s2[P] = 0, fm.n_sec[P] = 0;
    fm.unit[P] = m.supplementary ? fm.n_units++ : NO_UNIT;
    *unit = *parent = fm.unit[P];
    return CLS_SUPP;
}
// after the last selection: the reported supplementaries' s2 and mapq; uh[u - 1] is unit u's hit
NP2_KC_HD void family_end(const Family &fm, Hit *uh) {
    for (uint32_t P = 1; P < fm.n_par; ++P) {
        if (fm.unit[P] == NO_UNIT) continue;
        Hit &h = uh[fm.unit[P] - 1u];
        h.s2 = fm.s2[P], h.mapq = mapq_of(h.s1, h.s2, h.n);
    }
}
// one selected chain with its hit -> dropped, or classed and, when kept, written as the read's next unit.  uh, ucls, upar,
// uend: max_chains - 1 entries each, unit u at u - 1.
NP2_KC_HD void place_chain(Family &fm, const Hit &h, uint32_t end, const Opts &o, const MultiOpts &m, Hit *uh, uint32_t *ucls, uint32_t *upar,
                           int32_t *uend, MoreCounts *mc) {
    ++mc->selections;
    if (h.n < o.min_cnt) {
        ++mc->dropped_cnt;
        return;
    }
    uint32_t unit, parent;
    const uint32_t cls = classify(fm, h, m, &unit, &parent);
    if (unit == NO_UNIT) {
        if (cls == CLS_SEC) ++mc->dropped_pri;
        return;
    }
    ++(cls == CLS_SEC ? mc->kept_sec : mc->kept_supp);
    uh[unit - 1u] = h, ucls[unit - 1u] = cls, upar[unit - 1u] = parent, uend[unit - 1u] = (int32_t)end;
}

// The further selections of one mapped read, one lane (the host twin; the kernel runs the same steps with a wavefront's
// arg-max and re-sweep): on the f, p, mark and base finish_read left.  Returns the read's units, the primary included.
NP2_KC_HD uint32_t select_more(const uint64_t *hi, const uint64_t *lo, const int32_t *f, const int32_t *p, uint8_t *mark, int32_t *base,
                               uint32_t n_anchors, uint32_t qlen, const Opts &o, const MultiOpts &m, const Hit &primary, Family &fm, Hit *uh,
                               uint32_t *ucls, uint32_t *upar, int32_t *uend, MoreCounts *mc) {
    family_begin(fm, primary);
    for (uint32_t sel = 1; sel < m.max_chains; ++sel) {
        int64_t best = NO_CAND;
        for (uint32_t i = 0; i < n_anchors; ++i) {
            if (mark[i]) continue;
            const int64_t key = more_key(f[i] - base[i], i);
            if (key > best) best = key;
        }
        if (best == NO_CAND) break;
        int64_t score;
        uint32_t end;
        more_unkey(best, &score, &end);
        if (score < (int64_t)o.min_score) break;
        Hit h;
        const uint32_t first = take_chain(hi, lo, p, mark, end, (uint32_t)score, qlen, o, &h);
        for (uint32_t i = first; i < n_anchors; ++i)
            if (!mark[i]) base[i] = base_step(p[i], mark, f, base);
        place_chain(fm, h, end, o, m, uh, ucls, upar, uend, mc);
    }
    family_end(fm, uh);
    return fm.n_units;
}

// the options' ranges; nullptr when they hold, otherwise what is wrong (unsupported: k, w, lookback; the others: argument)
NP2_KC_HD const char *check_opts(const Opts &o, bool *unsupported) {
    *unsupported = true;
    if (o.k < K_MIN || o.k > K_MAX) return "k: the mapper is built for 11 <= k <= 28";
    if (o.w < W_MIN || o.w > W_MAX) return "w: the mapper is built for 1 <= w <= 64";
    if (o.lookback < 1 || o.lookback > LOOKBACK_MAX) return "lookback: the mapper is built for 1 <= lookback <= 64";
    *unsupported = false;
    if (o.max_occ < 1 || o.max_occ > MAX_OCC) return "max_occ must lie in 1 .. 2^20";
    if (o.max_gap < 1 || o.max_gap > MAX_GAP) return "max_gap must lie in 1 .. 2^30";
    if (o.bandwidth > MAX_BW) return "bandwidth must be at most 2^20";
    if (o.min_cnt > MAX_CNT || o.min_score > MAX_CNT) return "min_cnt and min_score must be at most 2^30";
    return nullptr;
}

} // namespace np2map
