// The short-read adapter rule (np2_sradapt.hip) as plain arithmetic without HIP types: option validation, the packed
// adapter, the overlap bounds and limit the kernel's lanes share, and the whole rule over one pair / one read, one position
// after the other (judge_pair / judge_single), for the stand-alone host program (tests/tools/sradapt_core_test.cpp) and hosts
// that hold a single pair; no device path goes through the serial functions.  The rule is this project's own, built on
// fastp's documented options; it is not pinned against the fastp binary.  include/np2_io.h states it; in short:
//
//   A base byte is case-folded; A/T and C/G are complements; any other byte is unknown and matches nothing.  Steps 1 - 3 of
//   the quality rule (np2_srqc_core.hpp) give every read its kept span [a, b), n = b - a.
//   A. pair overlap: x = mate 1's span, rcy = reverse complement of mate 2's.  For a shift s, x[i] faces rcy[i - s] over
//      i in [max(0, s), min(n1, n2 + s)), l(s) positions, d(s) of them unknown or different.  s is accepted if l(s) >= O and
//      d(s) <= min(D, P * l(s) / 100).  Tried s = 0, 1, 2, .. and then -1, -2, ..; the first accepted wins: T = n2 + s,
//      b1 = a1 + min(n1, T), b2 = a2 + min(n2, T).  Not searched when a span is longer than 1024 bases or shorter than O.
//   B. adapter by sequence, for a read A did not decide (span of 4 .. 1024 bases): the smallest p in [0, n - 4] with at most
//      c / 8 mismatches over c = min(n - p, A) letters; b = a + p.
//   C. step 4 of the quality rule over the new span; in a pair, the mate of a single failing read gets class 4.
#pragma once
#include <cstdint>

#include "np2_srqc_core.hpp"

namespace np2sradapt {

enum : uint32_t { PAIRED = 1u, FLAGS_ALL = 1u };
enum : uint32_t { MATE_FAILED = 4 };                                       // the class beside np2srqc's 0 .. 3
enum : uint32_t { HOW_NONE = 0, HOW_OVERLAP = 1, HOW_SEQ = 2 };
// totals, in the order of np2_sradapt_stats_t: np2srqc's seven, then
enum : uint32_t {
    T_MATE_FAILED = 7, T_PAIRS = 8, T_PAIRS_OVERLAP = 9, T_PAIRS_UNSEARCHED = 10, T_TRIMMED_OVERLAP = 11, T_TRIMMED_SEQ = 12,
    T_ADAPTER_BASES = 13, N_TOTALS = 14
};

static constexpr uint32_t MAX_SPAN = 1024, MIN_ADAPTER = 4, MAX_ADAPTER = 64, MAX_PERCENT = 100;

// The options as the kernel takes them: an adapter is two bit planes of its letters' codes, letter j in bit j.
struct Opts {
    uint32_t flags, overlap_min, overlap_diff, overlap_diff_percent;
    uint32_t a_len[2]; // 0: no adapter for that mate
    uint64_t a_lo[2], a_hi[2];
};
NP2_SRQC_HD Opts defaults() { return Opts{PAIRED, 30, 5, 20, {0, 0}, {0, 0}, {0, 0}}; }

// A base's 2-bit code, or 4 for an unknown byte: A 0, C 1, T 2, G 3, so that the complement is code ^ 2
NP2_SRQC_HD uint32_t base_code(uint32_t byte) {
    const uint32_t c = byte & 0xDFu;
    return (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? (c >> 1) & 3u : 4u;
}

// nullptr: valid; otherwise what is wrong.  `letters` may be nullptr (no adapter).
NP2_SRQC_HD const char *pack_adapter(const char *letters, uint32_t &len, uint64_t &lo, uint64_t &hi) {
    len = 0, lo = hi = 0;
    if (!letters) return nullptr;
    uint32_t n = 0;
    for (; letters[n]; ++n) {
        const char c = letters[n];
        if (n >= MAX_ADAPTER) return "an adapter sequence has 4 to 64 letters";
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return "an adapter sequence is letters of ACGT";
        const uint64_t code = base_code((uint8_t)c);
        lo |= (code & 1) << n, hi |= (code >> 1) << n;
    }
    if (n < MIN_ADAPTER) return "an adapter sequence has 4 to 64 letters";
    len = n;
    return nullptr;
}

// The options of a call (the fields of np2_sradapt_opts_t) -> the kernel's.  nullptr: valid.
NP2_SRQC_HD const char *make_opts(uint32_t flags, uint32_t overlap_min, uint32_t overlap_diff, uint32_t overlap_diff_percent,
                                  const char *adapter1, const char *adapter2, Opts &o) {
    o = Opts{flags, overlap_min, overlap_diff, overlap_diff_percent, {0, 0}, {0, 0}, {0, 0}};
    if ((flags & ~FLAGS_ALL) != 0) return "unknown flag bits";
    if (overlap_min < 1 || overlap_min > MAX_SPAN) return "overlap_min must be in [1, 1024]";
    if (overlap_diff > MAX_SPAN) return "overlap_diff must be in [0, 1024]";
    if (overlap_diff_percent > MAX_PERCENT) return "overlap_diff_percent must be in [0, 100]";
    if (adapter2 && !adapter1) return "adapter2 needs adapter1";
    if (!(flags & PAIRED) && !adapter1) return "single-end reads are trimmed by sequence: adapter1 is needed";
    if (const char *why = pack_adapter(adapter1, o.a_len[0], o.a_lo[0], o.a_hi[0])) return why;
    if (!adapter2) {
        o.a_len[1] = o.a_len[0], o.a_lo[1] = o.a_lo[0], o.a_hi[1] = o.a_hi[0];
        return nullptr;
    }
    return pack_adapter(adapter2, o.a_len[1], o.a_lo[1], o.a_hi[1]);
}

// ---- step A's arithmetic ------------------------------------------------------------------------------------------------------
NP2_SRQC_HD bool searchable(uint32_t n1, uint32_t n2, const Opts &o) {
    return n1 <= MAX_SPAN && n2 <= MAX_SPAN && n1 >= o.overlap_min && n2 >= o.overlap_min;
}
NP2_SRQC_HD bool past_cap(uint32_t n1, uint32_t n2) { return n1 > MAX_SPAN || n2 > MAX_SPAN; }
// shifts with l(s) >= O: s = 0 .. n_forward - 1 and s = -1 .. -n_backward (both spans at least O long)
NP2_SRQC_HD uint32_t n_forward(uint32_t n1, const Opts &o) { return n1 - o.overlap_min + 1; }
NP2_SRQC_HD uint32_t n_backward(uint32_t n2, const Opts &o) { return n2 - o.overlap_min; }
// l(s) for s >= 0, and for s = -t < 0
NP2_SRQC_HD uint32_t overlap_forward(uint32_t n1, uint32_t n2, uint32_t s) { return n1 - s < n2 ? n1 - s : n2; }
NP2_SRQC_HD uint32_t overlap_backward(uint32_t n1, uint32_t n2, uint32_t t) { return n2 - t < n1 ? n2 - t : n1; }
NP2_SRQC_HD uint32_t diff_limit(uint32_t len, const Opts &o) {
    const uint32_t p = o.overlap_diff_percent * len / 100u; // at most 100 * 1024
    return p < o.overlap_diff ? p : o.overlap_diff;
}
// two bases face each other and agree (codes of base_code; the second already complemented)
NP2_SRQC_HD bool match(uint32_t cx, uint32_t cy) { return cx < 4u && cx == cy; }
// the spans' new lengths once s is accepted; T = n2 + s
NP2_SRQC_HD void accept(uint32_t n1, uint32_t n2, int32_t s, uint32_t &m1, uint32_t &m2, uint32_t &insert) {
    insert = (uint32_t)((int32_t)n2 + s);
    m1 = n1 < insert ? n1 : insert, m2 = n2 < insert ? n2 : insert;
}

// ---- step B's arithmetic ------------------------------------------------------------------------------------------------------
NP2_SRQC_HD bool seq_searchable(uint32_t n, uint32_t a_len) { return a_len != 0 && n >= MIN_ADAPTER && n <= MAX_SPAN; }
NP2_SRQC_HD uint32_t seq_compared(uint32_t n, uint32_t p, uint32_t a_len) { return n - p < a_len ? n - p : a_len; }
NP2_SRQC_HD uint32_t seq_limit(uint32_t c) { return c / 8u; }
NP2_SRQC_HD uint32_t adapter_code(const Opts &o, uint32_t which, uint32_t j) {
    return (uint32_t)((o.a_lo[which] >> j) & 1u) | (uint32_t)((o.a_hi[which] >> j) & 1u) << 1;
}

// ---- the rule, serially ---------------------------------------------------------------------------------------------------------
struct Read {
    uint32_t begin, end, cls, how, insert;
};

// step A over x = s1[a1, b1), y = s2[a2, b2): true and the accepted shift, or false
inline bool find_overlap(const uint8_t *x, uint32_t n1, const uint8_t *y, uint32_t n2, const Opts &o, int32_t &shift) {
    if (!searchable(n1, n2, o)) return false;
    auto diffs = [&](uint32_t x0, uint32_t j0, uint32_t len) { // x[x0 + i] against rcy[j0 + i]
        uint32_t d = 0;
        for (uint32_t i = 0; i < len; ++i) {
            const uint32_t cy = base_code(y[n2 - 1 - (j0 + i)]);
            d += match(base_code(x[x0 + i]), cy < 4u ? cy ^ 2u : 4u) ? 0u : 1u;
        }
        return d;
    };
    for (uint32_t s = 0; s < n_forward(n1, o); ++s) {
        const uint32_t len = overlap_forward(n1, n2, s);
        if (diffs(s, 0, len) <= diff_limit(len, o)) return shift = (int32_t)s, true;
    }
    for (uint32_t t = 1; t <= n_backward(n2, o); ++t) {
        const uint32_t len = overlap_backward(n1, n2, t);
        if (diffs(0, t, len) <= diff_limit(len, o)) return shift = -(int32_t)t, true;
    }
    return false;
}

// step B over r[0, n): the winning p, or n
inline uint32_t find_adapter(const uint8_t *r, uint32_t n, const Opts &o, uint32_t which) {
    const uint32_t a_len = o.a_len[which];
    if (!seq_searchable(n, a_len)) return n;
    for (uint32_t p = 0; p + MIN_ADAPTER <= n; ++p) {
        const uint32_t c = seq_compared(n, p, a_len);
        uint32_t m = 0;
        for (uint32_t j = 0; j < c; ++j) m += base_code(r[p + j]) == adapter_code(o, which, j) ? 0u : 1u;
        if (m <= seq_limit(c)) return p;
    }
    return n;
}

inline uint32_t classify_span(const uint8_t *s, const uint8_t *q, uint32_t a, uint32_t b, const np2srqc::Opts &qc) {
    uint32_t n_n = 0, lowq = 0;
    for (uint32_t i = a; i < b; ++i) n_n += np2srqc::is_n(s[i]) ? 1u : 0u, lowq += np2srqc::phred(q[i]) < qc.qualified_q ? 1u : 0u;
    return np2srqc::classify(b - a, n_n, lowq, qc);
}

inline void seq_step(const uint8_t *s, const Opts &o, uint32_t which, Read &r) {
    const uint32_t n = r.end - r.begin, p = find_adapter(s + r.begin, n, o, which);
    if (p < n) r.end = r.begin + p, r.how = HOW_SEQ;
}

inline Read judge_single(const uint8_t *s, const uint8_t *q, uint32_t n, const np2srqc::Opts &qc, const Opts &o) {
    Read r{0, 0, 0, HOW_NONE, 0};
    (void)np2srqc::judge_serial(s, q, n, qc, r.begin, r.end);
    seq_step(s, o, 0, r);
    r.cls = classify_span(s, q, r.begin, r.end, qc);
    return r;
}

inline void judge_pair(const uint8_t *s1, const uint8_t *q1, uint32_t len1, const uint8_t *s2, const uint8_t *q2, uint32_t len2,
                       const np2srqc::Opts &qc, const Opts &o, Read &r1, Read &r2) {
    r1 = r2 = Read{0, 0, 0, HOW_NONE, 0};
    (void)np2srqc::judge_serial(s1, q1, len1, qc, r1.begin, r1.end);
    (void)np2srqc::judge_serial(s2, q2, len2, qc, r2.begin, r2.end);
    const uint32_t n1 = r1.end - r1.begin, n2 = r2.end - r2.begin;
    int32_t shift = 0;
    if (find_overlap(s1 + r1.begin, n1, s2 + r2.begin, n2, o, shift)) {
        uint32_t m1, m2, insert;
        accept(n1, n2, shift, m1, m2, insert);
        r1.insert = r2.insert = insert;
        if (m1 < n1) r1.end = r1.begin + m1, r1.how = HOW_OVERLAP;
        if (m2 < n2) r2.end = r2.begin + m2, r2.how = HOW_OVERLAP;
    } else {
        seq_step(s1, o, 0, r1);
        seq_step(s2, o, 1, r2);
    }
    r1.cls = classify_span(s1, q1, r1.begin, r1.end, qc);
    r2.cls = classify_span(s2, q2, r2.begin, r2.end, qc);
    if (r1.cls != 0 && r2.cls == 0) r2.cls = MATE_FAILED;
    else if (r2.cls != 0 && r1.cls == 0) r1.cls = MATE_FAILED;
}

// one read's share of the totals; `n` its bases, `b0` its span's end before A and B
inline void add_read(uint64_t *t, const Read &r, uint32_t n, uint32_t b0) {
    t[np2srqc::T_READS] += 1, t[np2srqc::T_BASES_IN] += n, t[np2srqc::T_BASES_OUT] += r.cls == 0 ? r.end - r.begin : 0u;
    t[r.cls == MATE_FAILED ? (uint32_t)T_MATE_FAILED : np2srqc::T_PASS + r.cls] += 1;
    t[T_TRIMMED_OVERLAP] += r.how == HOW_OVERLAP, t[T_TRIMMED_SEQ] += r.how == HOW_SEQ, t[T_ADAPTER_BASES] += b0 - r.end;
}

} // namespace np2sradapt
