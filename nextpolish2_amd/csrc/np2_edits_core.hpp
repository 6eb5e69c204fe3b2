// The edit rule of np2_edits_* (include/np2.h) as plain integer arithmetic without HIP types: what one lane of the kernels
// in np2_edits.hip does per position, per raw run and per edit.  The same text is the kernels' inner step and a one-lane
// host program (edits_host below, driven by tests/tools/edits_core_test.cpp on a machine without a GPU).  Bases, k-mers
// and hashes of the support counters are np2_kcount_core.hpp's, counts np2_qv_core.hpp's.
//
// Names: ref[0..L) the contig; out[0..n) the polished bases with their contig positions pos[0..n), non-decreasing;
// first = pos[0], last = pos[n-1].  A position's GROUP is the output bases stamped with it: out[gstart[p] .. gend[p]).
#pragma once
#include <cstdint>
#include <vector>

#include "np2_qv_core.hpp"

namespace np2edits {

static constexpr uint32_t NONE = 0xFFFFFFFFu;  // gstart of a position no output base is stamped with
static constexpr uint32_t WAVE_SIDE = 64;      // a raw run with a side longer than this is trimmed by a wavefront
static constexpr uint32_t MAX_TABLES = 8;      // k-mer tables one call can judge its edits by
enum Kind : uint32_t { SNV = 0, MNV = 1, INS = 2, DEL = 3, CPX = 4 };
// device error word
static constexpr uint32_t E_POS_RANGE = 1u;    // a position >= L
static constexpr uint32_t E_POS_ORDER = 2u;    // positions decrease
static constexpr uint32_t E_INTERNAL = 4u;     // a run or an offset outside its array (never on checked input)
// (np2_lookback.hpp's LB_ERR, 0x400, is or-ed into the same word by the scans)

// bytes compare without regard to ASCII case
NP2_KC_HD uint8_t fold(uint8_t c) { return (c >= (uint8_t)'a' && c <= (uint8_t)'z') ? (uint8_t)(c - 32u) : c; }
NP2_KC_HD bool same(uint8_t a, uint8_t b) { return fold(a) == fold(b); }

// rule 1: position p of the span is clean when its group is one base equal to ref[p]
NP2_KC_HD bool clean(const uint8_t *ref, const uint8_t *out, const uint32_t *gstart, const uint32_t *gend, uint32_t p) {
    const uint32_t g = gstart[p];
    return g != NONE && gend[p] - g == 1u && same(out[g], ref[p]);
}

// rule 3 by one lane: common suffix, then common prefix (s and o_s advance)
NP2_KC_HD void trim(const uint8_t *ref, const uint8_t *out, uint32_t &s, uint32_t &o_s, uint32_t &lr, uint32_t &la) {
    while (lr && la && same(ref[s + lr - 1], out[o_s + la - 1])) --lr, --la;
    while (lr && la && same(ref[s], out[o_s])) ++s, ++o_s, --lr, --la;
}

// rule 4
NP2_KC_HD uint32_t kind_of(uint32_t lr, uint32_t la) {
    if (lr == 0) return INS;
    if (la == 0) return DEL;
    if (lr == la) return lr == 1 ? SNV : MNV;
    return CPX;
}

// rule 5: how far an INS / DEL whose string is x[0..len) moves left from s, never below lo.  Rotating x right by one
// per step means that step j compares ref[s - 1 - j] with x[(len - 1 - j) mod len]: no step depends on another.
NP2_KC_HD uint32_t shift_of(const uint8_t *ref, const uint8_t *x, uint32_t len, uint32_t s, uint32_t lo) {
    uint32_t j = 0, at = len - 1;
    while (s - j > lo && same(ref[s - 1 - j], x[at])) {
        ++j;
        at = at ? at - 1 : len - 1;
    }
    return j;
}
// byte j of x rotated right `sh` times
NP2_KC_HD uint32_t rot_src(uint32_t j, uint32_t len, uint32_t sh) {
    const uint32_t r = sh % len;
    return j >= r ? j - r : j + len - r;
}

// rule 6: the k-mers wholly inside seq[max(0, at - (k-1)) .. min(n, at + len + (k-1))) end at bases [lo_end, hi)
NP2_KC_HD void window(uint64_t n, uint64_t at, uint64_t len, uint32_t k, uint64_t &lo_end, uint64_t &hi) {
    const uint64_t lo = at >= k - 1 ? at - (k - 1) : 0;
    hi = at + len + (k - 1) < n ? at + len + (k - 1) : n;
    lo_end = lo + (k - 1);
}
// the k-mer ending at base e (e >= k - 1): true and its table hash when all k bytes are bases
NP2_KC_HD bool kmer_at(const uint8_t *seq, uint64_t e, uint32_t k, uint64_t mask, uint64_t *hash) {
    np2kc::Roll r;
    bool ok = false;
    for (uint64_t b = e + 1 - k; b <= e; ++b) ok = np2kc::push(r, seq[b], k, mask, hash);
    return ok;
}

// ---- the one-lane host program ------------------------------------------------------------------------------------------
struct Edit { uint32_t ref_pos, ref_len, out_off, alt_len, kind; };
struct Totals {
    uint32_t has_span = 0, first = 0, last = 0;
    uint64_t raw_runs = 0, same_runs = 0, n_kind[5] = {0, 0, 0, 0, 0}, bases_inserted = 0, bases_deleted = 0, outside = 0;
};
struct HostResult {
    uint32_t err = 0;
    std::vector<Edit> edits;
    std::vector<uint32_t> ref_off{0}, alt_off{0};
    std::vector<uint8_t> ref_pool, alt_pool;
    Totals t;
};

inline HostResult edits_host(const uint8_t *ref, uint32_t L, const uint8_t *out, const uint32_t *pos, uint32_t n) {
    HostResult h;
    for (uint32_t i = 0; i < n; ++i) {
        if (pos[i] >= L) h.err |= E_POS_RANGE;
        if (i && pos[i - 1] > pos[i]) h.err |= E_POS_ORDER;
    }
    h.t.outside = L;
    if (h.err || n == 0) return h;
    std::vector<uint32_t> gstart(L, NONE), gend(L, 0);
    for (uint32_t i = 0; i < n; ++i) {
        if (i == 0 || pos[i - 1] != pos[i]) gstart[pos[i]] = i;
        if (i == n - 1 || pos[i + 1] != pos[i]) gend[pos[i]] = i + 1;
    }
    const uint32_t first = pos[0], last = pos[n - 1];
    h.t.has_span = 1, h.t.first = first, h.t.last = last;
    h.t.outside = (uint64_t)L - (last - first + 1);
    uint32_t prev_end = first; // one past the previous real edit's trimmed REF, before its own shift
    for (uint32_t p = first; p <= last;) {
        if (clean(ref, out, gstart.data(), gend.data(), p)) {
            ++p;
            continue;
        }
        uint32_t e = p;
        while (e < last && !clean(ref, out, gstart.data(), gend.data(), e + 1)) ++e;
        ++h.t.raw_runs;
        uint32_t s = p, o_s = p > first ? gstart[p - 1] + 1 : 0, o_e = e < last ? gstart[e + 1] : n;
        uint32_t lr = e - p + 1, la = o_e - o_s;
        p = e + 1;
        trim(ref, out, s, o_s, lr, la);
        if (!lr && !la) {
            ++h.t.same_runs;
            continue;
        }
        const uint32_t kind = kind_of(lr, la), end = s + lr;
        uint32_t sh = 0;
        if (kind == INS) sh = shift_of(ref, out + o_s, la, s, prev_end);
        if (kind == DEL) sh = shift_of(ref, ref + s, lr, s, prev_end);
        for (uint32_t j = 0; j < lr; ++j) h.ref_pool.push_back(ref[s + (kind == DEL ? rot_src(j, lr, sh) : j)]);
        for (uint32_t j = 0; j < la; ++j) h.alt_pool.push_back(out[o_s + (kind == INS ? rot_src(j, la, sh) : j)]);
        h.ref_off.push_back((uint32_t)h.ref_pool.size());
        h.alt_off.push_back((uint32_t)h.alt_pool.size());
        h.edits.push_back(Edit{s - sh, lr, o_s - sh, la, kind});
        ++h.t.n_kind[kind];
        if (la > lr) h.t.bases_inserted += la - lr;
        if (lr > la) h.t.bases_deleted += lr - la;
        prev_end = end;
    }
    return h;
}

// rule 6 for one edit and one sequence, `count_of(hash)` being the table's answer after the threshold
template <class F> inline void support_host(const uint8_t *seq, uint64_t n, uint64_t at, uint64_t len, uint32_t k, F count_of,
                                            uint32_t &n_kmers, uint32_t &n_absent) {
    uint64_t lo_end, hi;
    window(n, at, len, k, lo_end, hi);
    const uint64_t mask = np2kc::kmer_mask(k);
    n_kmers = n_absent = 0;
    for (uint64_t e = lo_end; e < hi; ++e) {
        uint64_t hash = 0;
        if (!kmer_at(seq, e, k, mask, &hash)) continue;
        ++n_kmers;
        if (count_of(hash) == 0) ++n_absent;
    }
}

} // namespace np2edits
