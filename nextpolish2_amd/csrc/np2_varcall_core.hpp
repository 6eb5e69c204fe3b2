// The rule of the read-supported variant caller (np2_varcall.hip, include/np2_io.h: np2_varcall_*), as plain arithmetic
// without HIP types: base codes, which records are counted, which CIGAR operations are indel events, their left shift, the
// allele key and the call tests.  The same text is the kernels' lane code, the host twin (np2_varcall_host: call_contig at
// the end of this file walks a contig on one thread) and a stand-alone host program (tests/tools/varcall_core_test.cpp).
//
// Definitions (a contig ref[L], alignment records with BAM CIGAR words len << 4 | op and BAM 4-bit SEQ):
//   codes     reference bytes, case-insensitive: A C G T = 0..3, anything else 4 (N); SEQ nibbles 1 2 4 8 = 0..3, others 4
//   counted   np2depth::counted under this rule's flags / mapq / fraction, 0 <= pos < L, no N operation (else "skipped"),
//             l_seq == sum of len over M I S = X (else "no SEQ"; SEQ * has l_seq 0)
//   cov[p]    counted records with pos <= p < min(pos + span, L) (span as in the depth report: M D = X)
//   alt[p][b] counted records with an M/=/X column at p < L whose read base is b in A C G T, ref[p] in A C G T, b != ref[p]
//   event     an I or D operation of 1 <= n <= max_indel bases whose neighbours in the CIGAR are both M, = or X, with a
//             preceding run (the consecutive M/=/X operations before it) of m >= 1 columns; a = reference position of the
//             column before it, qa = that column's query index.  D: a + n < L.  I: a + 1 < L and every inserted base A C G T.
//   shift     the largest t <= m - 1 whose steps j = 0 .. t-1 all hold: I: read[qa-j+n] == read[qa-j], both A C G T;
//             D: ref[a-j] == ref[a-j+n] and read[qa-j] == ref[a-j], all A C G T.  No step changes cov or alt.
//   key       (a' = a - t, kind DEL 0 / INS 1, n, bases): I: read[qa-t+1 .. qa-t+n] packed 2 bits each, first base highest;
//             D: 0.  hi = a' << 6 | kind << 5 | n, lo = bases: ascending (hi, lo) is (anchor, kind, n, bases).
//   call      tests in integers, c * 1000 >= pm * d.  SNV at p: d = cov[p], the alt base of the greatest count (ties A < C <
//             G < T), c its count.  Indel per (a', kind): the allele of the greatest count (ties: smaller n, then smaller
//             bases), d = min(cov[a'], cov[a'+1]).  Called iff d >= min_depth, c >= min_alt and c*1000 >= het_pm*d; hom iff
//             c*1000 >= hom_pm*d.  Order: by position, there SNV, DEL, INS.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/np2_io.h"
#include "np2_depth_core.hpp"

#if defined(__HIPCC__)
#define NP2_VC_HD __host__ __device__ __forceinline__
#else
#define NP2_VC_HD inline
#endif

namespace np2vc {

static constexpr uint32_t MAX_INDEL = 28;                       // 2 bits a base: 56 bits of the key's low word
static constexpr uint32_t DEFAULT_MIN_DEPTH = 8, DEFAULT_MIN_ALT = 3, DEFAULT_HOM_PM = 800, DEFAULT_HET_PM = 250, DEFAULT_MIN_MAPQ = 5;
static constexpr uint16_t DEFAULT_EXCLUDE_FLAGS = 0xF04;
enum : uint32_t { SNV = 0, DEL = 1, INS = 2 };                  // np2_varcall_t::kind (the order at one position)
enum : uint32_t { KEY_DEL = 0, KEY_INS = 1 };                   // the key's kind bit
enum : uint32_t { GT_NONE = 0, GT_HET = 1, GT_HOM = 2 };        // np2_varcall_t::gt
enum : uint32_t { REC_OUT = 0, REC_SKIPPED = 1, REC_NO_SEQ = 2, REC_COUNTED = 3 };

struct Rule {
    double min_aligned_fra;
    uint32_t exclude_flags, min_mapq, min_depth, min_alt, hom_pm, het_pm, max_indel;
};
// what np2_varcall_* refuses with NP2_E_ARG (min_alt 0 would call every position without a read behind it)
NP2_VC_HD bool rule_ok(const Rule &r) {
    return np2depth::fra_ok(r.min_aligned_fra) && r.hom_pm <= 1000 && r.het_pm <= r.hom_pm && r.max_indel >= 1 && r.max_indel <= MAX_INDEL &&
           r.min_alt >= 1;
}

NP2_VC_HD uint32_t ref_code(uint8_t c) {
    switch (c | 0x20) {
    case 'a': return 0;
    case 'c': return 1;
    case 'g': return 2;
    case 't': return 3;
    default: return 4;
    }
}
NP2_VC_HD uint32_t nib_code(uint32_t nib) { return nib == 1 ? 0u : nib == 2 ? 1u : nib == 4 ? 2u : nib == 8 ? 3u : 4u; }
// code of query base q of a record whose SEQ starts at seq (high nibble first)
NP2_VC_HD uint32_t read_code(const uint8_t *seq, uint64_t q) {
    const uint32_t b = seq[q >> 1];
    return nib_code((q & 1) ? (b & 15u) : (b >> 4));
}
NP2_VC_HD bool is_m(uint32_t op) { return op == 0 || op == 7 || op == 8; }
static constexpr uint32_t OPS_QUERY = 1u << 0 | 1u << 1 | 1u << 4 | 1u << 7 | 1u << 8; // M I S = X: bases of SEQ
NP2_VC_HD uint32_t ref_adv(uint32_t word) { return ((np2depth::OPS_SPAN >> (word & 15u)) & 1u) ? word >> 4 : 0u; }
NP2_VC_HD uint32_t query_adv(uint32_t word) { return ((OPS_QUERY >> (word & 15u)) & 1u) ? word >> 4 : 0u; }

// the sums of a CIGAR, or of a part of one
struct Walk {
    np2depth::Measure m;
    uint64_t query = 0; // M I S = X
    uint32_t has_n = 0;
};
NP2_VC_HD void add_op(Walk &w, uint32_t word) {
    np2depth::add_op(w.m, word);
    w.query += query_adv(word);
    w.has_n |= (word & 15u) == 3u ? 1u : 0u;
}
NP2_VC_HD uint32_t admit(uint32_t flag, uint32_t mapq, uint32_t n_cigar, int32_t pos, uint32_t l_seq, uint32_t L, const Walk &w, const Rule &r) {
    if (!np2depth::counted(flag, mapq, n_cigar, w.m, r.exclude_flags, r.min_mapq, r.min_aligned_fra)) return REC_OUT;
    if (pos < 0 || (uint32_t)pos >= L) return REC_OUT;
    if (w.has_n) return REC_SKIPPED;
    if ((uint64_t)l_seq != w.query) return REC_NO_SEQ;
    return REC_COUNTED;
}

// the shifts: read(q) and ref(p) give codes; qa - (m - 1) and a - (m - 1) are the first column of the preceding run
template <class Read> NP2_VC_HD uint64_t shift_ins(uint64_t qa, uint32_t n, uint64_t m, Read read) {
    uint64_t t = 0;
    while (t + 1 < m) {
        const uint32_t x = read(qa - t), y = read(qa - t + n);
        if (x > 3 || x != y) break;
        ++t;
    }
    return t;
}
template <class Read, class Ref> NP2_VC_HD uint64_t shift_del(uint64_t a, uint64_t qa, uint32_t n, uint64_t m, Read read, Ref ref) {
    uint64_t t = 0;
    while (t + 1 < m) {
        const uint32_t x = ref(a - t), y = ref(a - t + n), z = read(qa - t);
        if (x > 3 || x != y || x != z) break;
        ++t;
    }
    return t;
}
// n bases from query index q on, first base highest; false: one of them is not A C G T
template <class Read> NP2_VC_HD bool pack_bases(uint64_t q, uint32_t n, Read read, uint64_t &bases) {
    bases = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = read(q + i);
        if (c > 3) return false;
        bases = bases << 2 | c;
    }
    return true;
}
NP2_VC_HD uint64_t key_hi(uint32_t anchor, uint32_t key_kind, uint32_t n) { return (uint64_t)anchor << 6 | (uint64_t)key_kind << 5 | n; }
NP2_VC_HD uint32_t key_anchor(uint64_t hi) { return (uint32_t)(hi >> 6); }
NP2_VC_HD uint32_t key_kind(uint64_t hi) { return (uint32_t)(hi >> 5) & 1u; }
NP2_VC_HD uint32_t key_n(uint64_t hi) { return (uint32_t)hi & 31u; }
static constexpr unsigned KEY_HI_BITS = 38, KEY_LO_BITS = 56;

// One I or D operation (CIGAR word k of n_cigar at cg, starting at reference offset r_off from pos and at query index q_off)
// -> its key after the left shift; false: not an event.
template <class Read, class Ref>
NP2_VC_HD bool event_key(const uint32_t *cg, uint32_t n_cigar, uint32_t k, int32_t pos, uint64_t r_off, uint64_t q_off, uint32_t L, const Rule &rule,
                         Read read, Ref ref, uint64_t &hi, uint64_t &lo) {
    const uint32_t op = cg[k] & 15u, n = cg[k] >> 4;
    if ((op != 1 && op != 2) || n < 1 || n > rule.max_indel || k == 0 || k + 1 >= n_cigar) return false;
    if (!is_m(cg[k - 1] & 15u) || !is_m(cg[k + 1] & 15u)) return false;
    uint64_t m = 0;
    for (uint32_t j = k; j > 0 && is_m(cg[j - 1] & 15u); --j) m += cg[j - 1] >> 4;
    if (m < 1) return false;
    const uint64_t a = (uint64_t)(uint32_t)pos + r_off - 1, qa = q_off - 1; // (m >= 1: both offsets are at least 1)
    if (op == 2) {
        if (a + n >= (uint64_t)L) return false;
        const uint64_t t = shift_del(a, qa, n, m, read, ref);
        hi = key_hi((uint32_t)(a - t), KEY_DEL, n), lo = 0;
        return true;
    }
    if (a + 1 >= (uint64_t)L) return false;
    uint64_t bases;
    if (!pack_bases(qa + 1, n, read, bases)) return false;
    const uint64_t t = shift_ins(qa, n, m, read);
    if (!pack_bases(qa - t + 1, n, read, bases)) return false; // (shifted-in bases were compared: A C G T)
    hi = key_hi((uint32_t)(a - t), KEY_INS, n), lo = bases;
    return true;
}

NP2_VC_HD bool reaches(uint32_t c, uint32_t d, uint32_t pm) { return (uint64_t)c * 1000u >= (uint64_t)pm * d; }
NP2_VC_HD uint32_t judge(uint32_t d, uint32_t c, const Rule &r) {
    if (d < r.min_depth || c < r.min_alt || !reaches(c, d, r.het_pm)) return GT_NONE;
    return reaches(c, d, r.hom_pm) ? GT_HOM : GT_HET;
}
// the alt base of the greatest count at a position whose reference code is rc < 4 (ties: the smaller code)
NP2_VC_HD void best_snv(const uint32_t *alt4, uint32_t rc, uint32_t &b, uint32_t &c) {
    b = rc == 0 ? 1u : 0u, c = alt4[b];
    for (uint32_t x = b + 1; x < 4; ++x)
        if (x != rc && alt4[x] > c) b = x, c = alt4[x];
}
NP2_VC_HD np2_varcall_t make_call(uint32_t pos, uint32_t depth, uint32_t count, uint64_t bases, uint32_t kind, uint32_t gt, uint32_t len, uint32_t alt_code) {
    np2_varcall_t v;
    v.pos = pos, v.depth = depth, v.count = count, v.pad0 = 0, v.bases = bases;
    v.kind = (uint8_t)kind, v.gt = (uint8_t)gt, v.len = (uint8_t)len, v.alt_code = (uint8_t)alt_code, v.pad1 = 0;
    return v;
}
// stats.calls index
NP2_VC_HD uint32_t call_slot(uint32_t kind, uint32_t gt) { return kind * 2u + (gt - 1u); }

// ---- the whole rule on one thread (the host twin and the core test) ---------------------------------------------------------
struct Contig {
    std::vector<uint32_t> cov, alt; // [L], [4 L]
    std::vector<np2_varcall_t> calls;
    np2_varcall_stats_t stats;
};
// seq_bytes bounds every SEQ read: a counted record whose SEQ lies outside returns false (nothing else is checked here)
inline bool call_contig(const uint8_t *ref, uint32_t L, const np2_bamrec_t *recs, uint32_t n_recs, const uint32_t *cigar, const uint8_t *seq4,
                        uint64_t seq_bytes, const Rule &rule, Contig &out) {
    out.cov.assign(L, 0), out.alt.assign((size_t)4 * L, 0), out.calls.clear();
    memset(&out.stats, 0, sizeof out.stats);
    np2_varcall_stats_t &st = out.stats;
    st.records_seen = n_recs;
    if (L == 0) return true;
    std::vector<uint32_t> diff((size_t)L + 1, 0);
    std::vector<std::pair<uint64_t, uint64_t>> keys;
    auto refc = [&](uint64_t p) { return ref_code(ref[p]); };
    for (uint32_t i = 0; i < n_recs; ++i) {
        const np2_bamrec_t &r = recs[i];
        const uint32_t *cg = cigar + r.cigar_off;
        Walk w;
        for (uint32_t k = 0; k < r.n_cigar; ++k) add_op(w, cg[k]);
        const uint32_t adm = admit(r.flag, r.mapq, r.n_cigar, r.pos, r.l_seq, L, w, rule);
        st.records_skipped += adm == REC_SKIPPED, st.records_no_seq += adm == REC_NO_SEQ, st.records_counted += adm == REC_COUNTED;
        if (adm != REC_COUNTED) continue;
        if (r.l_seq && r.seq_off + ((uint64_t)r.l_seq + 1) / 2 > seq_bytes) return false;
        uint32_t lo, hi;
        np2depth::cover(r.pos, w.m.span, L, lo, hi);
        diff[lo] += 1, diff[hi] -= 1;
        const uint8_t *sq = seq4 + r.seq_off;
        auto readc = [&](uint64_t q) { return read_code(sq, q); };
        uint64_t r_off = 0, q_off = 0;
        for (uint32_t k = 0; k < r.n_cigar; ++k) {
            const uint32_t op = cg[k] & 15u, len = cg[k] >> 4;
            if (is_m(op)) {
                const uint64_t p0 = (uint64_t)(uint32_t)r.pos + r_off;
                const uint64_t cols = p0 < L ? std::min<uint64_t>(len, L - p0) : 0;
                for (uint64_t j = 0; j < cols; ++j) {
                    const uint32_t rc = refc(p0 + j), b = readc(q_off + j);
                    if (rc < 4 && b < 4 && b != rc) out.alt[4 * (p0 + j) + b] += 1;
                }
            } else {
                uint64_t khi, klo;
                if (event_key(cg, r.n_cigar, k, r.pos, r_off, q_off, L, rule, readc, refc, khi, klo)) keys.emplace_back(khi, klo);
            }
            r_off += ref_adv(cg[k]), q_off += query_adv(cg[k]);
        }
    }
    uint32_t run = 0;
    for (uint32_t p = 0; p < L; ++p) run += diff[p], out.cov[p] = run;
    st.events = keys.size();
    std::sort(keys.begin(), keys.end());
    // the best allele of every (anchor, kind): index into keys and its count
    struct Best {
        uint32_t anchor, kind, count;
        uint64_t hi, lo;
    };
    std::vector<Best> best;
    for (size_t i = 0; i < keys.size();) {
        size_t j = i;
        while (j < keys.size() && keys[j] == keys[i]) ++j;
        ++st.alleles;
        const uint32_t a = key_anchor(keys[i].first), kd = key_kind(keys[i].first), c = (uint32_t)(j - i);
        if (best.empty() || best.back().anchor != a || best.back().kind != kd) best.push_back(Best{a, kd, c, keys[i].first, keys[i].second});
        else if (c > best.back().count) best.back() = Best{a, kd, c, keys[i].first, keys[i].second};
        i = j;
    }
    size_t bi = 0;
    auto emit = [&](const np2_varcall_t &v) { out.calls.push_back(v), st.calls[call_slot(v.kind, v.gt)] += 1; };
    for (uint32_t p = 0; p < L; ++p) {
        const uint32_t rc = refc(p), d = out.cov[p];
        if (rc < 4 && d >= rule.min_depth) ++st.callable;
        if (rc < 4) {
            uint32_t b, c;
            best_snv(&out.alt[(size_t)4 * p], rc, b, c);
            if (const uint32_t gt = judge(d, c, rule)) emit(make_call(p, d, c, 0, SNV, gt, 1, b));
        }
        for (; bi < best.size() && best[bi].anchor == p; ++bi) { // (DEL before INS: the key's order)
            const Best &x = best[bi];
            const uint32_t d2 = std::min(d, p + 1 < L ? out.cov[p + 1] : 0u);
            if (const uint32_t gt = judge(d2, x.count, rule))
                emit(make_call(p, d2, x.count, x.lo, x.kind == KEY_DEL ? DEL : INS, gt, key_n(x.hi), 0));
        }
    }
    return true;
}

} // namespace np2vc
