// The rule of the assembly-to-reference caller (np2_asmcall.hip, include/np2_io.h: np2_asmcall*), as plain arithmetic without
// HIP types: base codes, the owned SAM interval, what a CIGAR measures, admission, the sort key, the footprint test.  The same
// text is the kernels' lane code, the host twin (np2_asmcall_host: call_all at the end of this file walks everything on one
// thread) and a stand-alone host program (tests/tools/asmcall_core_test.cpp).
//
// Definitions (references T_t at refs[ref_off[t] .. ref_off[t + 1]), g = ref_off[tid] + p a global position; alignments with BAM
// CIGAR words len << 4 | op in SAM orientation over a query stored forward):
//   codes     bytes, case-insensitive: A C G T = 0..3, anything else 4 (N); the complement of c < 4 is 3 - c
//   SAM base  j of an alignment: flag 16: the complement of forward byte q_len - 1 - j, else forward byte j
//   owned     SAM interval [s_lo, s_hi): flag 16: [q_len - own_hi, q_len - own_lo), else [own_lo, own_hi)
//   anchor    of an M = X column: itself; of an I or D operation of n >= 1 bases: the last M = X column before it in the CIGAR
//             (none: the operation is ignored).  A column or operation belongs iff s_lo <= its anchor's SAM index < s_hi
//   cover     belonging M = X columns cover their position, a belonging D the n positions it deletes: one interval [lo, hi)
//   events    SNV: a belonging M or X column with both codes < 4 and different; DEL (a, n), INS (a, n): belonging D, I at
//             anchor position a.  q_pos forward: SNV j -> rev ? q_len - 1 - j : j; INS at SAM q: rev ? q_len - q - n : q; DEL at
//             SAM q (the base after the gap): rev ? q_len - q : q
//   key       g << 2 | kind (SNV 0 < DEL 1 < INS 2): ascending keys, ties in input order, are the output order
//   kept      SNV: cov[g] == 1; DEL: cov == 1 on g .. g + n; INS: cov[g] == 1 and, when g + 1 is inside the reference, cov[g+1] == 1
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/np2_io.h"

#if defined(__HIPCC__)
#define NP2_AC_HD __host__ __device__ __forceinline__
#else
#define NP2_AC_HD inline
#endif

namespace np2ac {

static constexpr uint32_t DEFAULT_MIN_MAPQ = 5, DEFAULT_MIN_ALN = 5000;
static constexpr uint64_t MAX_TOTAL = 0xFFFF0000ull; // reference bases; query bytes + CIGAR words
enum : uint32_t { SNV = 0, DEL = 1, INS = 2 };
enum : uint32_t { ALN_ADMITTED = 0, ALN_UNALIGNED = 1, ALN_LOW_MAPQ = 2, ALN_SKIPPED = 3, ALN_SHORT = 4 };
static constexpr unsigned KEY_BITS = 34;

NP2_AC_HD uint32_t code(uint8_t c) {
    switch (c | 0x20) {
    case 'a': return 0;
    case 'c': return 1;
    case 'g': return 2;
    case 't': return 3;
    default: return 4;
    }
}
NP2_AC_HD uint32_t comp(uint32_t c) { return c < 4 ? 3u - c : c; }
// code of SAM base j of a query of q_len forward bytes at q
NP2_AC_HD uint32_t sam_code(const uint8_t *q, uint32_t q_len, bool rev, uint32_t j) { return rev ? comp(code(q[q_len - 1 - j])) : code(q[j]); }
NP2_AC_HD void owned_sam(const np2_asmaln_t &a, uint32_t &s_lo, uint32_t &s_hi) {
    const bool rev = (a.flag & 16u) != 0;
    s_lo = rev ? a.q_len - a.own_hi : a.own_lo;
    s_hi = rev ? a.q_len - a.own_lo : a.own_hi;
}
NP2_AC_HD bool is_m(uint32_t op) { return op == 0 || op == 7 || op == 8; }
static constexpr uint32_t OPS_REF = 1u << 0 | 1u << 2 | 1u << 7 | 1u << 8;            // M D = X
static constexpr uint32_t OPS_QUERY = 1u << 0 | 1u << 1 | 1u << 4 | 1u << 7 | 1u << 8; // M I S = X
static constexpr uint32_t OPS_KNOWN = OPS_REF | OPS_QUERY;                             // M I D S = X
NP2_AC_HD uint32_t ref_adv(uint32_t word) { return ((OPS_REF >> (word & 15u)) & 1u) ? word >> 4 : 0u; }
NP2_AC_HD uint32_t query_adv(uint32_t word) { return ((OPS_QUERY >> (word & 15u)) & 1u) ? word >> 4 : 0u; }
NP2_AC_HD uint32_t fwd_snv(uint32_t q_len, bool rev, uint32_t j) { return rev ? q_len - 1 - j : j; }
NP2_AC_HD uint32_t fwd_ins(uint32_t q_len, bool rev, uint32_t q, uint32_t n) { return rev ? q_len - q - n : q; }
NP2_AC_HD uint32_t fwd_del(uint32_t q_len, bool rev, uint32_t q) { return rev ? q_len - q : q; }

NP2_AC_HD uint64_t key(uint64_t g, uint32_t kind) { return g << 2 | kind; }
NP2_AC_HD np2_asmvar_t make_var(uint32_t tid, uint32_t pos, uint32_t aln, uint32_t len, uint32_t q_pos, uint32_t kind, uint32_t ref_code,
                                uint32_t alt_code, bool rev) {
    np2_asmvar_t v;
    v.tid = tid, v.pos = pos, v.aln = aln, v.len = len, v.q_pos = q_pos;
    v.kind = (uint8_t)kind, v.ref_code = (uint8_t)ref_code, v.alt_code = (uint8_t)alt_code, v.rev = rev ? 1 : 0;
    return v;
}
// the filter: g the event's global position, ref_end the global end of its reference; ones[i] = positions <= i with cov == 1
NP2_AC_HD bool kept(uint32_t kind, uint64_t g, uint32_t n, uint64_t ref_end, const uint32_t *cov, const uint32_t *ones) {
    if (cov[g] != 1) return false;
    if (kind == SNV) return true;
    if (kind == INS) return g + 1 >= ref_end || cov[g + 1] == 1;
    return g + n < ref_end && ones[g + n] - ones[g] == n; // (g itself was tested)
}

// what an alignment's CIGAR measures (64-bit: 2^32 operations of 2^28 - 1 bases each fit)
struct Measure {
    uint64_t span = 0, query = 0;
    bool foreign = false; // an operation that is none of M I D S = X
};
inline Measure measure(const uint32_t *cg, uint32_t n_cigar) {
    Measure m;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t op = cg[k] & 15u;
        if (!((OPS_KNOWN >> op) & 1u)) m.foreign = true;
        m.span += ref_adv(cg[k]), m.query += query_adv(cg[k]);
    }
    return m;
}
NP2_AC_HD uint32_t admit(uint32_t flag, uint32_t mapq, uint32_t n_cigar, bool foreign, uint64_t span, uint32_t min_mapq, uint32_t min_aln) {
    if ((flag & 4u) || n_cigar == 0) return ALN_UNALIGNED;
    if (mapq < min_mapq) return ALN_LOW_MAPQ;
    if (foreign) return ALN_SKIPPED;
    if (span < (uint64_t)min_aln) return ALN_SHORT;
    return ALN_ADMITTED;
}

// ---- the argument check both doors run before anything else: nullptr = fine, else what is wrong -----------------------------
// adm (or nullptr) takes every alignment's admission outcome; *unsupported is set when the refusal is NP2_E_UNSUPPORTED
inline const char *check(const uint64_t *ref_off, uint32_t n_refs, uint64_t query_bytes, const np2_asmaln_t *alns, uint32_t n_alns,
                         const uint32_t *cigar, uint64_t n_cigar_words, uint32_t min_mapq, uint32_t min_aln, std::vector<uint8_t> *adm,
                         bool *unsupported, uint32_t *bad_aln) {
    *unsupported = false, *bad_aln = 0xFFFFFFFFu;
    if (ref_off[0] != 0) return "ref_off[0] is not 0";
    for (uint32_t t = 0; t < n_refs; ++t)
        if (ref_off[t + 1] < ref_off[t]) return "ref_off is not ascending";
    if (ref_off[n_refs] > MAX_TOTAL) return *unsupported = true, "references of more than 4294901760 bases in total";
    if (query_bytes + n_cigar_words > MAX_TOTAL) return *unsupported = true, "more than 4294901760 query bytes and CIGAR words";
    if (adm) adm->assign(n_alns, ALN_UNALIGNED);
    for (uint32_t i = 0; i < n_alns; ++i) {
        const np2_asmaln_t &a = alns[i];
        *bad_aln = i;
        if (a.n_cigar && (a.cigar_off > n_cigar_words || a.n_cigar > n_cigar_words - a.cigar_off)) return "CIGAR outside the buffer";
        if (a.q_len && (a.q_off > query_bytes || a.q_len > query_bytes - a.q_off)) return "query outside the buffer";
        if (a.own_lo > a.own_hi || a.own_hi > a.q_len) return "owned interval outside the query";
        if ((a.flag & 4u) || a.n_cigar == 0) continue;
        const Measure m = measure(cigar + a.cigar_off, a.n_cigar);
        if (!m.foreign) {
            if (a.tid < 0 || (uint32_t)a.tid >= n_refs) return "tid outside the references";
            if ((uint64_t)a.pos + m.span > ref_off[a.tid + 1] - ref_off[a.tid]) return "alignment beyond the end of its reference";
            if (m.query != a.q_len) return "CIGAR query length differs from q_len";
        }
        if (adm) (*adm)[i] = (uint8_t)admit(a.flag, a.mapq, a.n_cigar, m.foreign, m.span, min_mapq, min_aln);
    }
    *bad_aln = 0xFFFFFFFFu;
    return nullptr;
}

// ---- the whole rule on one thread (the host twin and the core test); the arguments passed check() ----------------------------
struct Result {
    std::vector<uint32_t> cov; // [ref_off[n_refs]]
    std::vector<np2_asmrun_t> runs;
    std::vector<np2_asmvar_t> vars;
    np2_asmcall_stats_t stats;
};
inline void call_all(const uint8_t *refs, const uint64_t *ref_off, uint32_t n_refs, const uint8_t *query, const np2_asmaln_t *alns,
                     uint32_t n_alns, const uint32_t *cigar, const std::vector<uint8_t> &adm, Result &out) {
    const uint64_t G = ref_off[n_refs];
    memset(&out.stats, 0, sizeof out.stats);
    np2_asmcall_stats_t &st = out.stats;
    out.cov.assign(G, 0), out.runs.clear(), out.vars.clear();
    std::vector<uint32_t> diff(G + 1, 0);
    std::vector<std::pair<uint64_t, np2_asmvar_t>> ev;
    st.alns_seen = n_alns;
    for (uint32_t i = 0; i < n_alns; ++i) {
        st.alns_unaligned += adm[i] == ALN_UNALIGNED, st.alns_low_mapq += adm[i] == ALN_LOW_MAPQ, st.alns_skipped += adm[i] == ALN_SKIPPED;
        st.alns_short += adm[i] == ALN_SHORT, st.alns_admitted += adm[i] == ALN_ADMITTED;
        if (adm[i] != ALN_ADMITTED) continue;
        const np2_asmaln_t &a = alns[i];
        const uint32_t *cg = cigar + a.cigar_off;
        const uint8_t *q = query + a.q_off, *ref = refs + ref_off[a.tid];
        const uint64_t g0 = ref_off[a.tid];
        const bool rev = (a.flag & 16u) != 0;
        uint32_t s_lo, s_hi;
        owned_sam(a, s_lo, s_hi);
        uint32_t r = a.pos, qi = 0, aq = 0, ar = 0, lo = 0xFFFFFFFFu, hi = 0;
        bool has = false;
        for (uint32_t k = 0; k < a.n_cigar; ++k) {
            const uint32_t op = cg[k] & 15u, len = cg[k] >> 4;
            if (is_m(op) && len) {
                const uint32_t c_lo = std::max(qi, s_lo), c_hi = std::min(qi + len, s_hi);
                if (c_lo < c_hi) {
                    lo = std::min(lo, r + (c_lo - qi)), hi = std::max(hi, r + (c_hi - qi));
                    for (uint32_t j = c_lo; j < c_hi && op != 7; ++j) {
                        const uint32_t p = r + (j - qi), rc = code(ref[p]), qc = sam_code(q, a.q_len, rev, j);
                        if (rc < 4 && qc < 4 && rc != qc)
                            ev.emplace_back(key(g0 + p, SNV), make_var(a.tid, p, i, 1, fwd_snv(a.q_len, rev, j), SNV, rc, qc, rev)), ++st.found[SNV];
                    }
                }
                has = true, aq = qi + len - 1, ar = r + len - 1;
            } else if ((op == 1 || op == 2) && len && has && aq >= s_lo && aq < s_hi) {
                if (op == 2) {
                    lo = std::min(lo, r), hi = std::max(hi, r + len);
                    ev.emplace_back(key(g0 + ar, DEL), make_var(a.tid, ar, i, len, fwd_del(a.q_len, rev, qi), DEL, 0, 0, rev)), ++st.found[DEL];
                } else {
                    ev.emplace_back(key(g0 + ar, INS), make_var(a.tid, ar, i, len, fwd_ins(a.q_len, rev, qi, len), INS, 0, 0, rev)), ++st.found[INS];
                }
            }
            r += ref_adv(cg[k]), qi += query_adv(cg[k]);
        }
        if (lo < hi) diff[g0 + lo] += 1, diff[g0 + hi] -= 1;
    }
    std::vector<uint32_t> ones(G, 0);
    uint32_t run = 0, n1 = 0;
    for (uint64_t g = 0; g < G; ++g) {
        run += diff[g], out.cov[g] = run;
        n1 += run == 1, ones[g] = n1;
        st.cov0_bases += run == 0, st.cov2_bases += run >= 2;
    }
    st.r_bases = n1;
    for (uint32_t t = 0; t < n_refs; ++t)
        for (uint64_t g = ref_off[t]; g < ref_off[t + 1];) {
            if (out.cov[g] != 1) {
                ++g;
                continue;
            }
            uint64_t e = g;
            while (e < ref_off[t + 1] && out.cov[e] == 1) ++e;
            out.runs.push_back(np2_asmrun_t{t, (uint32_t)(g - ref_off[t]), (uint32_t)(e - ref_off[t])});
            g = e;
        }
    st.runs = out.runs.size();
    std::vector<std::pair<uint64_t, np2_asmvar_t>> keep;
    for (const auto &e : ev) {
        const np2_asmvar_t &v = e.second;
        if (!kept(v.kind, e.first >> 2, v.len, ref_off[v.tid + 1], out.cov.data(), ones.data())) continue;
        keep.push_back(e), ++st.kept[v.kind];
        st.ins_bases += v.kind == INS ? v.len : 0, st.del_bases += v.kind == DEL ? v.len : 0;
    }
    std::stable_sort(keep.begin(), keep.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
    for (const auto &e : keep) out.vars.push_back(e.second);
}

} // namespace np2ac
