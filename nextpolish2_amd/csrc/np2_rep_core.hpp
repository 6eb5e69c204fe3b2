// Per-lane arithmetic of the repetitive k-mer list (np2_rep.hip; the rule is in include/np2_io.h): byte -> 2-bit code ->
// rolled forward / reverse-complement words -> "k bases seen" -> canonical index into the direct-addressed counter table;
// index -> text; and the threshold rule over a (count value, occurrences) list.  Plain integer arithmetic without HIP types:
// the same text is the count kernel's inner step, the host driver's selection and a one-lane host program
// (tests/tools/rep_core_test.cpp).  code() and Roll are the k-mer counter's (np2_kcount_core.hpp).
#pragma once
#include "np2_kcount_core.hpp"

namespace np2rep {
using np2kc::Roll;

static constexpr uint32_t K_MIN = 2, K_MAX = 16, K_DEFAULT = 15;
static constexpr uint64_t MAX_KMERS = 0xFFFFFFFFull; // a counter is a uint32 and can hold every k-mer of the stream

// counters of the table for k: every 2k-bit word is an index (the canonical ones are the ones that get counted)
NP2_KC_HD uint64_t table_size(uint32_t k) { return 1ULL << (2u * k); }

// One byte of the stream.  True when the last k bytes were all bases: *v is then min(fw, rv) of the k-mer that ENDS at
// this byte, first base most significant, A=0 C=1 G=2 T=3: the lexicographically smaller of the k-mer and its reverse
// complement.  *v <= 4^k - 1 always: fw is masked, rv is shifted down before its top base is set.
NP2_KC_HD bool push(Roll &r, uint8_t ch, uint32_t k, uint64_t mask, uint32_t *v) {
    const uint32_t c = np2kc::code(ch);
    if (c >= 4u) {
        r.l = 0;
        return false;
    }
    r.fw = ((r.fw << 2) | (uint64_t)c) & mask;
    r.rv = (r.rv >> 2) | ((uint64_t)(3u - c) << (2u * (k - 1u)));
    if (r.l < k) ++r.l;
    if (r.l < k) return false;
    *v = (uint32_t)(r.fw < r.rv ? r.fw : r.rv);
    return true;
}

// k-mers a stream of n bytes can hold at most
NP2_KC_HD uint64_t max_kmers(uint64_t n, uint32_t k) { return n >= k ? n - k + 1 : 0; }

NP2_KC_HD uint32_t revcomp(uint32_t v, uint32_t k) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < k; ++i, v >>= 2) r = r << 2 | (3u - (v & 3u));
    return r;
}
// k upper-case letters, no terminator
NP2_KC_HD void index_text(uint32_t v, uint32_t k, char *out) {
    for (uint32_t i = 0; i < k; ++i) out[i] = "ACGT"[(v >> (2u * (k - 1u - i))) & 3u];
}

// target of `distinct = f` over D counters above 0, in IEEE double
NP2_KC_HD uint64_t target_of(double f, uint64_t D) { return (uint64_t)(f * (double)D); }

// The threshold rule over a list in ascending value order, entry i standing for the value values[i] (or i itself without
// `values`) that occurs occ[i] times: the first entry with occ > 0 whose running sum of occ reaches `target`; *before = the
// sum in front of it.  n when there is none (an empty list, or target above the total).  The host driver runs it twice:
// over the histogram of the counts' high halves, then over the low halves inside the chosen bin with target - *before.
NP2_KC_HD uint64_t select_entry(const uint64_t *occ, uint64_t n, uint64_t target, uint64_t *before) {
    uint64_t cum = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (occ[i] == 0) continue;
        if (cum + occ[i] >= target) {
            *before = cum;
            return i;
        }
        cum += occ[i];
    }
    *before = cum;
    return n;
}
// threshold of `distinct = f` over (value, occurrences) pairs in ascending value order; 0 for an empty list
NP2_KC_HD uint32_t threshold_of(const uint32_t *values, const uint64_t *occ, uint64_t n, double f) {
    uint64_t D = 0, before = 0;
    for (uint64_t i = 0; i < n; ++i) D += occ[i];
    const uint64_t i = select_entry(occ, n, target_of(f, D), &before);
    return i < n ? values[i] : 0u;
}

} // namespace np2rep
