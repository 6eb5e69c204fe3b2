// The short-read quality rule (np2_srqc.hip) as plain arithmetic without HIP types: option validation, the fixed trims,
// the window test, the class of a read.  The same text is the kernel's lane code, the host side's argument check and a
// stand-alone host program (tests/tools/srqc_core_test.cpp).  The rule is this project's own, built on the options of the
// reference README's fastp recipe; it is not pinned against the fastp binary.
//
// One read: n bases s[0..n), n quality bytes, p[i] = max(0, byte - 33).
//   1. a = min(trim_front, n), b = max(a, n - trim_tail) (saturating): the kept span is [a, b)
//   2. cut_front, if on and b > a: the smallest i with a <= i, i + W <= b and p[i] + .. + p[i+W-1] >= M * W.  None: a = b.
//      Otherwise a = i, then a += 1 while a < b and s[a] is N / n.
//   3. cut_tail, if on and b > a: the largest j with j <= b, j - W >= a and p[j-W] + .. + p[j-1] >= M * W.  None: b = a.
//      Otherwise b = j, then b -= 1 while b > a and s[b-1] is N / n.
//   4. len = b - a, nN = N / n in [a, b), lowq = positions of [a, b) with p < Q.  Class, in this order: 1 too short
//      (len < min_len or len == 0), 2 too many N (nN > n_base_limit), 3 low quality (100 * lowq > U * len), else 0 pass.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NP2_SRQC_HD __host__ __device__ __forceinline__
#else
#define NP2_SRQC_HD inline
#endif

namespace np2srqc {

enum : uint32_t { CUT_FRONT = 1u, CUT_TAIL = 2u, FLAGS_ALL = 3u };
enum : uint32_t { PASS = 0, TOO_SHORT = 1, TOO_MANY_N = 2, LOW_QUALITY = 3, N_CLASSES = 4 };
// totals, in the order of np2_srqc_stats_t
enum : uint32_t { T_READS = 0, T_PASS = 1, T_TOO_SHORT = 2, T_TOO_MANY_N = 3, T_LOW_QUALITY = 4, T_BASES_IN = 5, T_BASES_OUT = 6, N_TOTALS = 7 };

static constexpr uint32_t MAX_WINDOW = 1000, MAX_Q = 93, MAX_PERCENT = 100;

// the ten options (the layout of np2_srqc_opts_t)
struct Opts {
    uint32_t trim_front, trim_tail, cut_window, cut_mean_q, n_base_limit, qualified_q, unqualified_percent, min_len, flags;
};
// the reference README's recipe: fastp -5 -3 -n 0 -f 5 -F 5 -t 5 -T 5 -q 20 (window 4, mean 20, 40 % unqualified, length 15)
NP2_SRQC_HD Opts recipe() { return Opts{5, 5, 4, 20, 0, 20, 40, 15, CUT_FRONT | CUT_TAIL}; }

// nullptr: valid; otherwise what is wrong
NP2_SRQC_HD const char *invalid(const Opts &o) {
    if (o.cut_window < 1 || o.cut_window > MAX_WINDOW) return "cut_window must be in [1, 1000]";
    if (o.cut_mean_q > MAX_Q) return "cut_mean_q must be in [0, 93]";
    if (o.qualified_q > MAX_Q) return "qualified_q must be in [0, 93]";
    if (o.unqualified_percent > MAX_PERCENT) return "unqualified_percent must be in [0, 100]";
    if ((o.flags & ~FLAGS_ALL) != 0) return "unknown flag bits";
    return nullptr;
}

NP2_SRQC_HD uint32_t phred(uint32_t byte) { return byte > 33u ? byte - 33u : 0u; }
NP2_SRQC_HD bool is_n(uint32_t byte) { return byte == 'N' || byte == 'n'; }

// step 1
NP2_SRQC_HD void fixed_trim(uint32_t n, const Opts &o, uint32_t &a, uint32_t &b) {
    a = o.trim_front < n ? o.trim_front : n;
    const uint32_t rest = o.trim_tail < n ? n - o.trim_tail : 0u;
    b = rest > a ? rest : a;
}
// a window's sum passes: at most 1000 values of at most 222 against at most 93 * 1000, all far inside 32 bits
NP2_SRQC_HD uint32_t window_floor(const Opts &o) { return o.cut_mean_q * o.cut_window; }
NP2_SRQC_HD bool window_ok(uint32_t sum, const Opts &o) { return sum >= window_floor(o); }
// windows that fit [a, b): start positions a .. a + n_windows - 1
NP2_SRQC_HD uint32_t n_windows(uint32_t a, uint32_t b, const Opts &o) { return b - a >= o.cut_window ? b - a - o.cut_window + 1 : 0u; }

// step 4 (64-bit products: lowq and len may be any u32)
NP2_SRQC_HD uint32_t classify(uint32_t len, uint32_t n_n, uint32_t lowq, const Opts &o) {
    if (len < o.min_len || len == 0) return TOO_SHORT;
    if (n_n > o.n_base_limit) return TOO_MANY_N;
    if ((uint64_t)100 * lowq > (uint64_t)o.unqualified_percent * len) return LOW_QUALITY;
    return PASS;
}

// The whole rule over one read, one position after the other: what the kernel's wave computes with prefix sums and ballots.
// For the stand-alone program and for hosts that hold a single read; no device path goes through it.
NP2_SRQC_HD uint32_t judge_serial(const uint8_t *s, const uint8_t *q, uint32_t n, const Opts &o, uint32_t &a, uint32_t &b) {
    fixed_trim(n, o, a, b);
    const uint32_t W = o.cut_window;
    if ((o.flags & CUT_FRONT) && b > a) {
        const uint32_t nw = n_windows(a, b, o);
        uint32_t sum = 0, i = 0;
        bool found = false;
        for (uint32_t j = 0; nw && j < W; ++j) sum += phred(q[a + j]);
        for (; i < nw; ++i) {
            if (window_ok(sum, o)) {
                found = true;
                break;
            }
            if (i + 1 < nw) sum += phred(q[a + i + W]) - phred(q[a + i]);
        }
        if (!found) a = b;
        else
            for (a += i; a < b && is_n(s[a]); ++a) {}
    }
    if ((o.flags & CUT_TAIL) && b > a) {
        const uint32_t nw = n_windows(a, b, o);
        uint32_t sum = 0, u = 0;
        bool found = false;
        for (uint32_t j = 0; nw && j < W; ++j) sum += phred(q[b - 1 - j]);
        for (; u < nw; ++u) { // the window [b - u - W, b - u)
            if (window_ok(sum, o)) {
                found = true;
                break;
            }
            if (u + 1 < nw) sum += phred(q[b - u - W - 1]) - phred(q[b - u - 1]);
        }
        if (!found) b = a;
        else
            for (b -= u; b > a && is_n(s[b - 1]); --b) {}
    }
    uint32_t n_n = 0, lowq = 0;
    for (uint32_t i = a; i < b; ++i) n_n += is_n(s[i]) ? 1u : 0u, lowq += phred(q[i]) < o.qualified_q ? 1u : 0u;
    return classify(b - a, n_n, lowq, o);
}

} // namespace np2srqc
