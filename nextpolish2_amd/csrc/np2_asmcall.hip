// An assembly's differences from a reference, from the alignments of its segments (include/np2_io.h: np2_asmcall; the rule's
// text is np2_asmcall_core.hpp).
//
//   k_ac_walk      a wavefront per admitted alignment.  64 CIGAR words a step: a wave-wide scan gives every word its reference
//                  and query offsets, a ballot of the M/=/X words and one shuffle give every I or D word its anchor (the last
//                  column of the nearest M/=/X word before it, carried from step to step).  The words of the step that hold
//                  something — a belonging I or D, an M or X word with owned columns — are then taken one after the other, the
//                  columns 64 a step, the query byte against the reference byte, mismatches balloted: each byte is read once.
//                  Two instantiations: the count pass leaves the alignment's number of events and adds +1 / -1 of its covered
//                  interval into the difference array (uint32 words that wrap, as in np2_depth.hip); after a scan of the counts
//                  the emit pass writes the events in CIGAR order from the alignment's offset on, ranked by ballot and prefix
//                  popcount, each with its sort key (ref_off[tid] + pos) << 2 | kind.
//   k_depth_scan   (np2_depth.hip) three times: the coverage from the difference array, the counts of cov == 1 positions
//                  (k_ac_ones writes the flags) that make a deletion's footprint one subtraction, the event offsets.
//   k_ac_runs      a thread owns 8 consecutive positions: a run starts where cov == 1 and the position before is not, or is
//                  another reference's; the r-th start and the r-th end meet in runs[r] through the look-back (np2_lookback.hpp).
//   k_ac_filter    a thread owns 8 events: those whose whole footprint has cov == 1 are compacted in order through the
//                  look-back, as (key, index) pairs for one stable pair sort (rocPRIM); k_ac_gather then writes the records.
// Integer atomics only: no result depends on the order of the alignments.
#include "np2_asmcall.hpp"
#include "np2_blockscan.hpp"

namespace np2 {

namespace {

__device__ __forceinline__ uint32_t wave_min32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ uint32_t wave_max32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_ac_walk(const np2_asmaln_t *__restrict__ alns, const uint32_t *__restrict__ adm, uint32_t n_adm,
                                                 const uint32_t *__restrict__ cigar, const uint8_t *__restrict__ query,
                                                 const uint8_t *__restrict__ refs, const uint64_t *__restrict__ ref_off, uint32_t G,
                                                 uint32_t *__restrict__ diff, uint32_t *__restrict__ ev_cnt, uint64_t *__restrict__ keys,
                                                 np2_asmvar_t *__restrict__ vars, uint32_t ev_cap, AsmDev *__restrict__ ctr) {
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (i >= n_adm) return; // (uniform across the wavefront; the kernel has no barrier)
    const uint32_t ai = adm[i];
    const np2_asmaln_t a = alns[ai];
    const uint32_t *cg = cigar + a.cigar_off;
    const uint8_t *q = query + a.q_off;
    const uint64_t g0 = ref_off[a.tid];
    const uint8_t *ref = refs + g0;
    const bool rev = (a.flag & 16u) != 0;
    const uint64_t lt = (1ull << lane) - 1;
    uint32_t s_lo, s_hi;
    np2ac::owned_sam(a, s_lo, s_hi);
    uint32_t r_base = a.pos, q_base = 0;        // where the step's first word starts
    uint32_t carry_q = 0, carry_r = 0;          // the last M/=/X column of the steps before
    bool carry_has = false;
    uint32_t lo = 0xFFFFFFFFu, hi = 0;          // this lane's part of the covered interval
    uint32_t cursor = EMIT ? (i ? ev_cnt[i - 1] : 0u) : 0u; // (uniform) the next event's slot; the count pass counts from 0
    uint32_t n_del = 0, n_ins = 0;              // (uniform)
    auto put = [&](uint32_t slot, uint32_t pos, uint32_t len, uint32_t q_pos, uint32_t kind, uint32_t rc, uint32_t qc) {
        if (slot < ev_cap) keys[slot] = np2ac::key(g0 + pos, kind), vars[slot] = np2ac::make_var((uint32_t)a.tid, pos, ai, len, q_pos, kind, rc, qc, rev);
        else atomicOr(&ctr->err, AC_ERR_EVENTS);
    };
    for (uint32_t k0 = 0; k0 < a.n_cigar; k0 += 64) {
        const uint32_t k = k0 + lane;
        const uint32_t word = k < a.n_cigar ? cg[k] : 15u; // (op 15, length 0: advances nothing)
        const uint32_t op = word & 15u, len = word >> 4;
        const uint32_t r_adv = np2ac::ref_adv(word), q_adv = np2ac::query_adv(word);
        const uint32_t r_incl = wave_incl_scan<OpAdd>(r_adv), q_incl = wave_incl_scan<OpAdd>(q_adv);
        const uint32_t r_off = r_base + r_incl - r_adv, q_off = q_base + q_incl - q_adv; // reference position, SAM query index
        const bool is_mcol = np2ac::is_m(op) && len > 0;
        const uint64_t mm = __ballot(is_mcol);
        // the anchor of this lane's word, were it an I or D
        const uint32_t end_q = q_off + len - 1, end_r = r_off + len - 1; // (of an M/=/X word: its last column)
        const uint64_t below = mm & lt;
        const int src = below ? 63 - __clzll((long long)below) : 0;
        uint32_t aq = __shfl(end_q, src), ar = __shfl(end_r, src);
        const bool has = below ? true : carry_has;
        if (!below) aq = carry_q, ar = carry_r;
        const bool is_gap = (op == 1 || op == 2) && len > 0 && has && aq >= s_lo && aq < s_hi;
        uint32_t c_lo = 0, c_hi = 0; // the owned columns of an M/=/X word, as SAM query indices
        if (is_mcol) c_lo = max(q_off, s_lo), c_hi = min(q_off + len, s_hi);
        if (c_lo < c_hi) lo = min(lo, r_off + (c_lo - q_off)), hi = max(hi, r_off + (c_hi - q_off));
        if (is_gap && op == 2) lo = min(lo, r_off), hi = max(hi, r_off + len);
        n_del += (uint32_t)__popcll(__ballot(is_gap && op == 2)), n_ins += (uint32_t)__popcll(__ballot(is_gap && op == 1));
        uint64_t work = __ballot(is_gap || (c_lo < c_hi && op != 7));
        while (work) {
            const int w = __builtin_ctzll(work);
            work &= work - 1;
            const uint32_t w_op = __shfl(op, w);
            if (w_op == 1 || w_op == 2) {
                if (EMIT && (int)lane == w)
                    put(cursor, ar, len, op == 2 ? np2ac::fwd_del(a.q_len, rev, q_off) : np2ac::fwd_ins(a.q_len, rev, q_off, len),
                        op == 2 ? np2ac::DEL : np2ac::INS, 0, 0);
                ++cursor;
                continue;
            }
            const uint32_t c0 = __shfl(c_lo, w), c1 = __shfl(c_hi, w), wq = __shfl(q_off, w), wr = __shfl(r_off, w);
            for (uint64_t j0 = c0; j0 < c1; j0 += 64) {
                const uint64_t j = j0 + lane;
                uint32_t rc = 4, qc = 4, p = 0;
                if (j < c1) p = wr + ((uint32_t)j - wq), rc = np2ac::code(ref[p]), qc = np2ac::sam_code(q, a.q_len, rev, (uint32_t)j);
                const bool mis = rc < 4 && qc < 4 && rc != qc;
                const uint64_t mask = __ballot(mis);
                if (EMIT && mis) put(cursor + (uint32_t)__popcll(mask & lt), p, 1, np2ac::fwd_snv(a.q_len, rev, (uint32_t)j), np2ac::SNV, rc, qc);
                cursor += (uint32_t)__popcll(mask);
            }
        }
        if (mm) {
            const int top = 63 - __clzll((long long)mm);
            carry_q = __shfl(end_q, top), carry_r = __shfl(end_r, top), carry_has = true;
        }
        r_base += __shfl(r_incl, 63), q_base += __shfl(q_incl, 63);
    }
    if (!EMIT) {
        lo = wave_min32(lo), hi = wave_max32(hi);
        if (lane == 0) {
            ev_cnt[i] = cursor;
            if (lo < hi) {
                if (g0 + hi <= (uint64_t)G) atomicAdd(&diff[g0 + lo], 1u), atomicAdd(&diff[g0 + hi], 0xFFFFFFFFu); // inside the G + 1 words
                else atomicOr(&ctr->err, AC_ERR_RANGE);
            }
            const uint32_t n_snv = cursor - n_del - n_ins;
            if (n_snv) atomicAdd(&ctr->found[np2ac::SNV], (unsigned long long)n_snv);
            if (n_del) atomicAdd(&ctr->found[np2ac::DEL], (unsigned long long)n_del);
            if (n_ins) atomicAdd(&ctr->found[np2ac::INS], (unsigned long long)n_ins);
        }
    }
}

__global__ __launch_bounds__(256) void k_ac_ones(const uint32_t *__restrict__ cov, uint32_t G, uint32_t *__restrict__ ones) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < G) ones[i] = cov[i] == 1 ? 1u : 0u;
}

__global__ __launch_bounds__(DEPTH_THREADS) void k_ac_runs(Lookback lb, const uint32_t *__restrict__ cov, uint32_t G, const uint64_t *__restrict__ ref_off,
                                                           uint32_t n_refs, np2_asmrun_t *__restrict__ runs, uint32_t max_runs, AsmDev *__restrict__ ctr) {
    __shared__ uint32_t sh[16];
    const uint32_t bid = lb_block_id(lb, sh);
    const uint32_t i0 = bid * DEPTH_TILE + threadIdx.x * DEPTH_ITEMS;
    // cov == 1 of the positions i0 - 1 .. i0 + 8 in bits 0 .. 9 (outside [0, G): not), "first position of a reference" of
    // i0 .. i0 + 8 in bits 0 .. 8 of jm
    uint32_t okm = 0, jm = 0, t0 = 0;
    if (i0 < G) {
        if (i0 > 0 && cov[i0 - 1] == 1) okm |= 1u;
#pragma unroll
        for (uint32_t k = 0; k <= DEPTH_ITEMS; ++k)
            if (k < G - i0 && cov[i0 + k] == 1) okm |= 2u << k;
        // the reference of i0: the first t with ref_off[t + 1] > i0 (i0 < G = ref_off[n_refs]: there is one)
        uint32_t a = 0, b = n_refs - 1;
        while (a < b) {
            const uint32_t m = a + (b - a) / 2;
            if (ref_off[m + 1] > i0) b = m;
            else a = m + 1;
        }
        t0 = a;
        uint32_t t = t0;
        for (uint32_t k = 0; k <= DEPTH_ITEMS && k < G - i0; ++k) {
            while (ref_off[t + 1] <= (uint64_t)i0 + k) ++t; // (i0 + k < G: stops at n_refs - 1 at the latest)
            if (ref_off[t] == (uint64_t)i0 + k) jm |= 1u << k;
        }
    }
    const uint32_t is_start = (okm >> 1) & (~okm | jm) & 0xFFu, is_end = (okm >> 1) & (~(okm >> 2) | (jm >> 1)) & 0xFFu;
    uint32_t total, pre, unused;
    uint32_t rank = block_excl_scan<OpAdd, 16>((uint32_t)__builtin_popcount(is_start), sh, total);
    lb_exclusive2(lb, bid, total, 0u, sh, &ctr->err, pre, unused);
    rank += pre; // runs that start before i0
    if (is_start | is_end) {
        uint32_t t = t0;
        for (uint32_t k = 0; k < DEPTH_ITEMS; ++k) {
            if (!(((is_start | is_end) >> k) & 1u)) continue;
            while (ref_off[t + 1] <= (uint64_t)i0 + k) ++t; // (a live position)
            const uint32_t p = (uint32_t)((uint64_t)i0 + k - ref_off[t]);
            if ((is_start >> k) & 1u) {
                if (rank < max_runs) runs[rank].tid = t, runs[rank].start = p;
                else atomicOr(&ctr->err, AC_ERR_RUNS);
                ++rank;
            }
            if (((is_end >> k) & 1u) && rank - 1 < max_runs) runs[rank - 1].end = p + 1; // (a cov == 1 position follows a start: rank >= 1)
        }
    }
    if (bid == lb.n_blocks - 1 && threadIdx.x == 0) ctr->n_runs = pre + total;
}

__global__ __launch_bounds__(DEPTH_THREADS) void k_ac_filter(Lookback lb, const uint64_t *__restrict__ keys, const np2_asmvar_t *__restrict__ vars, uint32_t n_ev,
                                                             const uint32_t *__restrict__ cov, const uint32_t *__restrict__ ones,
                                                             const uint64_t *__restrict__ ref_off, uint64_t *__restrict__ kept_keys,
                                                             uint64_t *__restrict__ kept_idx, AsmDev *__restrict__ ctr) {
    __shared__ uint32_t sh[16];
    const uint32_t bid = lb_block_id(lb, sh);
    const uint32_t i0 = bid * DEPTH_TILE + threadIdx.x * DEPTH_ITEMS;
    uint32_t keep = 0;
    uint64_t tot[5] = {0, 0, 0, 0, 0}; // kept SNV, DEL, INS; inserted, deleted bases
    for (uint32_t k = 0; k < DEPTH_ITEMS; ++k) {
        if (!(i0 < n_ev && k < n_ev - i0)) break;
        const np2_asmvar_t v = vars[i0 + k];
        if (!np2ac::kept(v.kind, keys[i0 + k] >> 2, v.len, ref_off[v.tid + 1], cov, ones)) continue;
        keep |= 1u << k;
        tot[0] += v.kind == np2ac::SNV, tot[1] += v.kind == np2ac::DEL, tot[2] += v.kind == np2ac::INS;
        tot[3] += v.kind == np2ac::INS ? v.len : 0u, tot[4] += v.kind == np2ac::DEL ? v.len : 0u;
    }
    uint32_t total, pre, unused;
    uint32_t rank = block_excl_scan<OpAdd, 16>((uint32_t)__builtin_popcount(keep), sh, total);
    lb_exclusive2(lb, bid, total, 0u, sh, &ctr->err, pre, unused);
    rank += pre;
    for (uint32_t k = 0; k < DEPTH_ITEMS; ++k)
        if ((keep >> k) & 1u) kept_keys[rank] = keys[i0 + k], kept_idx[rank] = i0 + k, ++rank; // rank < n_ev
#pragma unroll
    for (uint32_t t = 0; t < 5; ++t) {
        const uint64_t v = wave_sum64(tot[t]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(t < 3 ? &ctr->kept[t] : t == 3 ? &ctr->ins_bases : &ctr->del_bases, (unsigned long long)v);
    }
    if (bid == lb.n_blocks - 1 && threadIdx.x == 0) ctr->n_kept = pre + total;
}

__global__ __launch_bounds__(256) void k_ac_gather(const np2_asmvar_t *__restrict__ vars, const uint64_t *__restrict__ idx, uint32_t n,
                                                   np2_asmvar_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = vars[idx[i]];
}

} // namespace

void launch_asmcall_walk(hipStream_t s, const np2_asmaln_t *alns, const uint32_t *adm, uint32_t n_adm, const uint32_t *cigar, const uint8_t *query,
                         const uint8_t *refs, const uint64_t *ref_off, uint32_t G, uint32_t *diff, uint32_t *ev_cnt, uint64_t *keys, np2_asmvar_t *vars,
                         uint32_t ev_cap, AsmDev *ctr) {
    if (!n_adm) return;
    const dim3 grid((uint32_t)(((uint64_t)n_adm * 64 + 255) / 256));
    if (vars) hipLaunchKernelGGL(k_ac_walk<true>, grid, dim3(256), 0, s, alns, adm, n_adm, cigar, query, refs, ref_off, G, diff, ev_cnt, keys, vars, ev_cap, ctr);
    else hipLaunchKernelGGL(k_ac_walk<false>, grid, dim3(256), 0, s, alns, adm, n_adm, cigar, query, refs, ref_off, G, diff, ev_cnt, keys, vars, ev_cap, ctr);
}
void launch_asmcall_ones(hipStream_t s, const uint32_t *cov, uint32_t G, uint32_t *ones) {
    if (G) hipLaunchKernelGGL(k_ac_ones, dim3((uint32_t)(((uint64_t)G + 255) / 256)), dim3(256), 0, s, cov, G, ones);
}
void launch_asmcall_runs(hipStream_t s, const Lookback &lb, const uint32_t *cov, uint32_t G, const uint64_t *ref_off, uint32_t n_refs,
                         np2_asmrun_t *runs, uint32_t max_runs, AsmDev *ctr) {
    if (G) hipLaunchKernelGGL(k_ac_runs, dim3(depth_blocks(G)), dim3(DEPTH_THREADS), 0, s, lb, cov, G, ref_off, n_refs, runs, max_runs, ctr);
}
void launch_asmcall_filter(hipStream_t s, const Lookback &lb, const uint64_t *keys, const np2_asmvar_t *vars, uint32_t n_ev, const uint32_t *cov,
                           const uint32_t *ones, const uint64_t *ref_off, uint64_t *kept_keys, uint64_t *kept_idx, AsmDev *ctr) {
    if (n_ev) hipLaunchKernelGGL(k_ac_filter, dim3(depth_blocks(n_ev)), dim3(DEPTH_THREADS), 0, s, lb, keys, vars, n_ev, cov, ones, ref_off, kept_keys, kept_idx, ctr);
}
void launch_asmcall_gather(hipStream_t s, const np2_asmvar_t *vars, const uint64_t *idx, uint32_t n, np2_asmvar_t *out) {
    if (n) hipLaunchKernelGGL(k_ac_gather, dim3((n + 255) / 256), dim3(256), 0, s, vars, idx, n, out);
}

} // namespace np2
