// Read-supported variants of a contig from its alignment records (include/np2_io.h: np2_varcall_*; the rule's text is
// np2_varcall_core.hpp).
//
//   k_vc_records   a wavefront per record.  The lanes stride over its CIGAR words and the sums of the admission rule are
//                  reduced across the wavefront; lane 0 adds +1 at diff[pos] and -1 at diff[min(pos + span, L)] (uint32 words
//                  that wrap, as in np2_depth.hip).  Then the CIGAR is walked 64 words a step: a wave-wide scan gives every
//                  word its reference and query offsets; the lane of an I or D word applies the event rule and walks the left
//                  shift on its own, a ballot ranks the step's events and one atomic takes their slots (the keys are sorted
//                  afterwards: their order here plays no part); every M/=/X word of the step is then compared by all lanes, 64
//                  columns a step, the SEQ nibble against the reference byte, with an atomic into alt only where they differ.
//   (sorts)        rocPRIM's stable pair sort twice: by the key's low word (bases), then by its high word (anchor, kind, n).
//   k_vc_alleles   a thread per sorted key: key heads are counted (the alleles); the thread of the first key of an (anchor,
//                  kind) walks that group — at most one event per record and anchor: no longer than the depth — and leaves the
//                  first allele of the greatest count in best / best_count.
//   k_depth_scan   (np2_depth.hip) the coverage from diff.
//   k_vc_calls     a thread owns 8 consecutive positions: the SNV, DEL and INS calls of each under the rule, in that order.
//                  Launched once to count them and the callable positions, and once — after the host has made room — to
//                  write them in order: block scan of the threads' counts, look-back (np2_lookback.hpp) over the blocks.
// Integer atomics only: no result depends on the order of the records.
#include "np2_varcall.hpp"
#include "np2_blockscan.hpp"

namespace np2 {

namespace {

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint64_t wave_incl_sum64(uint64_t v, uint32_t lane) {
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_vc_records(const np2_bamrec_t *__restrict__ recs, const uint32_t *__restrict__ cigar,
                                                    const uint8_t *__restrict__ seq, uint64_t seq_bytes, uint32_t n_recs,
                                                    const uint8_t *__restrict__ ref, uint32_t L, np2vc::Rule rule, uint32_t *__restrict__ diff,
                                                    uint32_t *__restrict__ alt, uint64_t *__restrict__ ev_hi, uint64_t *__restrict__ ev_lo,
                                                    uint32_t ev_cap, VarDev *__restrict__ ctr) {
    __shared__ uint32_t sh_n[4]; // records by admission outcome (np2vc::REC_*)
    if (threadIdx.x < 4) sh_n[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (r < n_recs) { // (uniform across the wavefront)
        const np2_bamrec_t rec = recs[r];
        const uint32_t *cg = cigar + rec.cigar_off;
        np2vc::Walk w;
        for (uint32_t k = lane; k < rec.n_cigar; k += 64) np2vc::add_op(w, cg[k]);
        w.m.span = wave_sum64(w.m.span), w.m.aligned = wave_sum64(w.m.aligned), w.m.read_len = wave_sum64(w.m.read_len);
        w.query = wave_sum64(w.query), w.has_n = __ballot(w.has_n != 0) ? 1u : 0u;
        uint32_t adm = np2vc::admit(rec.flag, rec.mapq, rec.n_cigar, rec.pos, rec.l_seq, L, w, rule);
        if (adm == np2vc::REC_COUNTED && rec.l_seq && rec.seq_off + ((uint64_t)rec.l_seq + 1) / 2 > seq_bytes) { // (the host checked: never)
            if (lane == 0) atomicOr(&ctr->err, VC_ERR_SEQ);
            adm = np2vc::REC_NO_SEQ;
        }
        if (lane == 0) atomicAdd(&sh_n[adm], 1u);
        if (adm == np2vc::REC_COUNTED) {
            uint32_t lo, hi;
            if (lane == 0 && np2depth::cover(rec.pos, w.m.span, L, lo, hi)) { // lo < L, hi <= L: inside the L + 1 words
                atomicAdd(&diff[lo], 1u);
                atomicAdd(&diff[hi], 0xFFFFFFFFu);
            }
            const uint8_t *sq = seq + rec.seq_off;
            auto readc = [&](uint64_t q) { return np2vc::read_code(sq, q); }; // q < l_seq = the CIGAR's query length
            auto refc = [&](uint64_t p) { return np2vc::ref_code(ref[p]); };  // p < L by the event rule
            uint64_t r_base = 0, q_base = 0; // offsets at which the step's first word starts
            for (uint32_t k0 = 0; k0 < rec.n_cigar; k0 += 64) {
                const uint32_t k = k0 + lane;
                const uint32_t word = k < rec.n_cigar ? cg[k] : 15u; // (op 15, length 0: advances nothing)
                const uint32_t op = word & 15u, len = word >> 4;
                const uint64_t r_adv = np2vc::ref_adv(word), q_adv = np2vc::query_adv(word);
                const uint64_t r_incl = wave_incl_sum64(r_adv, lane), q_incl = wave_incl_sum64(q_adv, lane);
                const uint64_t r_off = r_base + r_incl - r_adv, q_off = q_base + q_incl - q_adv;
                // indel events of this step
                uint64_t khi = 0, klo = 0;
                bool ev = false;
                if (k < rec.n_cigar && (op == 1 || op == 2)) ev = np2vc::event_key(cg, rec.n_cigar, k, rec.pos, r_off, q_off, L, rule, readc, refc, khi, klo);
                const uint64_t evm = __ballot(ev);
                if (evm) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&ctr->n_events, (uint32_t)__popcll(evm));
                    base = __shfl(base, 0);
                    if (ev) {
                        const uint32_t slot = base + (uint32_t)__popcll(evm & ((1ull << lane) - 1));
                        if (slot >= base && slot < ev_cap) ev_hi[slot] = khi, ev_lo[slot] = klo;
                        else atomicOr(&ctr->err, VC_ERR_EVENTS);
                    }
                }
                // mismatches: the M/=/X words of this step, one after the other, 64 columns at a time
                uint64_t mm = __ballot(np2vc::is_m(op) && len > 0);
                while (mm) {
                    const int src = __builtin_ctzll(mm);
                    mm &= mm - 1;
                    const uint32_t l = __shfl(len, src);
                    const uint64_t p0 = (uint64_t)(uint32_t)rec.pos + __shfl(r_off, src), q0 = __shfl(q_off, src);
                    if (p0 >= L) continue;
                    const uint64_t cols = min((uint64_t)l, (uint64_t)L - p0);
                    for (uint64_t j = lane; j < cols; j += 64) {
                        const uint32_t rc = np2vc::ref_code(ref[p0 + j]), b = readc(q0 + j);
                        if (rc < 4 && b < 4 && b != rc) atomicAdd(&alt[4 * (p0 + j) + b], 1u);
                    }
                }
                r_base += __shfl(r_incl, 63), q_base += __shfl(q_incl, 63);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t first = blockIdx.x * (blockDim.x >> 6);
        atomicAdd(&ctr->n_seen, min(n_recs - first, blockDim.x >> 6));
        if (sh_n[np2vc::REC_COUNTED]) atomicAdd(&ctr->n_counted, sh_n[np2vc::REC_COUNTED]);
        if (sh_n[np2vc::REC_NO_SEQ]) atomicAdd(&ctr->n_no_seq, sh_n[np2vc::REC_NO_SEQ]);
        if (sh_n[np2vc::REC_SKIPPED]) atomicAdd(&ctr->n_skipped, sh_n[np2vc::REC_SKIPPED]);
    }
}

__global__ __launch_bounds__(256) void k_vc_alleles(const uint64_t *__restrict__ ev_hi, const uint64_t *__restrict__ ev_lo, uint32_t n, uint32_t L,
                                                    uint32_t *__restrict__ best, uint32_t *__restrict__ best_count, VarDev *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool head = false;
    if (i < n) {
        const uint64_t h = ev_hi[i], l = ev_lo[i];
        const uint64_t ph = i ? ev_hi[i - 1] : 0, pl = i ? ev_lo[i - 1] : 0;
        head = i == 0 || ph != h || pl != l;
        if (i == 0 || (ph >> 5) != (h >> 5)) { // the first key of its (anchor, kind)
            uint64_t ch = h, cl = l;
            uint32_t first = i, run = 0, bi = i, bc = 0;
            for (uint32_t j = i; j < n; ++j) {
                const uint64_t hj = ev_hi[j];
                if ((hj >> 5) != (h >> 5)) break;
                const uint64_t lj = ev_lo[j];
                if (hj != ch || lj != cl) {
                    if (run > bc) bc = run, bi = first;
                    ch = hj, cl = lj, first = j, run = 0;
                }
                ++run;
            }
            if (run > bc) bc = run, bi = first;
            const uint32_t a = np2vc::key_anchor(h);
            if (a < L) best[2 * (uint64_t)a + np2vc::key_kind(h)] = bi + 1, best_count[2 * (uint64_t)a + np2vc::key_kind(h)] = bc;
        }
    }
    const uint64_t hm = __ballot(head);
    if ((threadIdx.x & 63) == 0 && hm) atomicAdd(&ctr->n_alleles, (uint32_t)__popcll(hm));
}

// the calls at position p: bit kind set in the result, the call in out[kind]
__device__ __forceinline__ uint32_t calls_at(uint32_t p, uint32_t L, const uint8_t *__restrict__ ref, const uint32_t *__restrict__ cov,
                                             const uint32_t *__restrict__ alt, const uint32_t *__restrict__ best, const uint32_t *__restrict__ best_count,
                                             const uint64_t *__restrict__ ev_hi, const uint64_t *__restrict__ ev_lo, const np2vc::Rule &rule,
                                             np2_varcall_t (&out)[3], bool &callable) {
    const uint32_t rc = np2vc::ref_code(ref[p]), d = cov[p];
    uint32_t mask = 0;
    callable = rc < 4 && d >= rule.min_depth;
    if (rc < 4) {
        const uint4 a4 = *reinterpret_cast<const uint4 *>(alt + 4 * (uint64_t)p);
        const uint32_t a[4] = {a4.x, a4.y, a4.z, a4.w};
        uint32_t b, c;
        np2vc::best_snv(a, rc, b, c);
        if (const uint32_t gt = np2vc::judge(d, c, rule)) out[np2vc::SNV] = np2vc::make_call(p, d, c, 0, np2vc::SNV, gt, 1, b), mask |= 1u;
    }
    const uint2 bi = *reinterpret_cast<const uint2 *>(best + 2 * (uint64_t)p);
    if (bi.x | bi.y) {
        const uint2 bc = *reinterpret_cast<const uint2 *>(best_count + 2 * (uint64_t)p);
        const uint32_t d2 = min(d, p + 1 < L ? cov[p + 1] : 0u);
        if (bi.x)
            if (const uint32_t gt = np2vc::judge(d2, bc.x, rule))
                out[np2vc::DEL] = np2vc::make_call(p, d2, bc.x, 0, np2vc::DEL, gt, np2vc::key_n(ev_hi[bi.x - 1]), 0), mask |= 2u;
        if (bi.y)
            if (const uint32_t gt = np2vc::judge(d2, bc.y, rule))
                out[np2vc::INS] = np2vc::make_call(p, d2, bc.y, ev_lo[bi.y - 1], np2vc::INS, gt, np2vc::key_n(ev_hi[bi.y - 1]), 0), mask |= 4u;
    }
    return mask;
}

template <bool EMIT>
__global__ __launch_bounds__(DEPTH_THREADS) void k_vc_calls(Lookback lb, const uint8_t *__restrict__ ref, uint32_t L, const uint32_t *__restrict__ cov,
                                                            const uint32_t *__restrict__ alt, const uint32_t *__restrict__ best,
                                                            const uint32_t *__restrict__ best_count, const uint64_t *__restrict__ ev_hi,
                                                            const uint64_t *__restrict__ ev_lo, np2vc::Rule rule, np2_varcall_t *__restrict__ calls,
                                                            uint32_t max_calls, VarDev *__restrict__ ctr) {
    __shared__ uint32_t sh[16];
    __shared__ uint32_t sh_tot[8]; // callable, the six call totals, all calls
    uint32_t bid = blockIdx.x;
    if (EMIT) bid = lb_block_id(lb, sh);
    const uint32_t i0 = bid * DEPTH_TILE + threadIdx.x * DEPTH_ITEMS;
    np2_varcall_t out[3];
    uint32_t n_mine = 0;
    if (!EMIT) {
        if (threadIdx.x < 8) sh_tot[threadIdx.x] = 0;
        __syncthreads();
        uint32_t tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t k = 0; k < DEPTH_ITEMS; ++k) {
            if (!(i0 < L && k < L - i0)) break;
            bool callable;
            const uint32_t mask = calls_at(i0 + k, L, ref, cov, alt, best, best_count, ev_hi, ev_lo, rule, out, callable);
            tot[0] += callable ? 1u : 0u;
            for (uint32_t kind = 0; kind < 3; ++kind)
                if ((mask >> kind) & 1u) tot[1 + np2vc::call_slot(kind, out[kind].gt)] += 1, tot[7] += 1;
        }
#pragma unroll
        for (uint32_t t = 0; t < 8; ++t) {
            uint32_t v = tot[t];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if ((threadIdx.x & 63) == 0 && v) atomicAdd(&sh_tot[t], v);
        }
        __syncthreads();
        if (threadIdx.x == 0 && sh_tot[0]) atomicAdd(&ctr->callable, (unsigned long long)sh_tot[0]);
        if (threadIdx.x >= 1 && threadIdx.x < 7 && sh_tot[threadIdx.x]) atomicAdd(&ctr->calls[threadIdx.x - 1], (unsigned long long)sh_tot[threadIdx.x]);
        if (threadIdx.x == 7 && sh_tot[7]) atomicAdd(&ctr->n_calls, sh_tot[7]);
    } else {
        for (uint32_t k = 0; k < DEPTH_ITEMS; ++k) {
            if (!(i0 < L && k < L - i0)) break;
            bool callable;
            n_mine += (uint32_t)__builtin_popcount(calls_at(i0 + k, L, ref, cov, alt, best, best_count, ev_hi, ev_lo, rule, out, callable));
        }
        uint32_t total, pre, unused;
        uint32_t rank = block_excl_scan<OpAdd, 16>(n_mine, sh, total);
        lb_exclusive2(lb, bid, total, 0u, sh, &ctr->err, pre, unused);
        rank += pre;
        for (uint32_t k = 0; k < DEPTH_ITEMS && n_mine; ++k) {
            if (!(i0 < L && k < L - i0)) break;
            bool callable;
            const uint32_t mask = calls_at(i0 + k, L, ref, cov, alt, best, best_count, ev_hi, ev_lo, rule, out, callable);
            for (uint32_t kind = 0; kind < 3; ++kind)
                if ((mask >> kind) & 1u) {
                    if (rank < max_calls) calls[rank] = out[kind];
                    else atomicOr(&ctr->err, VC_ERR_CALLS);
                    ++rank;
                }
        }
    }
}

} // namespace

void launch_varcall_records(hipStream_t s, const np2_bamrec_t *recs, const uint32_t *cigar, const uint8_t *seq, uint64_t seq_bytes, uint32_t n_recs,
                            const uint8_t *ref, uint32_t L, np2vc::Rule rule, uint32_t *diff, uint32_t *alt, uint64_t *ev_hi, uint64_t *ev_lo,
                            uint32_t ev_cap, VarDev *ctr) {
    if (n_recs)
        hipLaunchKernelGGL(k_vc_records, dim3((uint32_t)(((uint64_t)n_recs * 64 + 255) / 256)), dim3(256), 0, s, recs, cigar, seq, seq_bytes, n_recs, ref, L,
                           rule, diff, alt, ev_hi, ev_lo, ev_cap, ctr);
}
void launch_varcall_alleles(hipStream_t s, const uint64_t *ev_hi, const uint64_t *ev_lo, uint32_t n, uint32_t L, uint32_t *best, uint32_t *best_count,
                            VarDev *ctr) {
    if (n) hipLaunchKernelGGL(k_vc_alleles, dim3((n + 255) / 256), dim3(256), 0, s, ev_hi, ev_lo, n, L, best, best_count, ctr);
}
void launch_varcall_calls(hipStream_t s, const Lookback &lb, const uint8_t *ref, uint32_t L, const uint32_t *cov, const uint32_t *alt,
                          const uint32_t *best, const uint32_t *best_count, const uint64_t *ev_hi, const uint64_t *ev_lo, np2vc::Rule rule,
                          np2_varcall_t *calls, uint32_t max_calls, VarDev *ctr) {
    if (!L) return;
    if (calls)
        hipLaunchKernelGGL(k_vc_calls<true>, dim3(depth_blocks(L)), dim3(DEPTH_THREADS), 0, s, lb, ref, L, cov, alt, best, best_count, ev_hi, ev_lo, rule,
                           calls, max_calls, ctr);
    else
        hipLaunchKernelGGL(k_vc_calls<false>, dim3(depth_blocks(L)), dim3(DEPTH_THREADS), 0, s, lb, ref, L, cov, alt, best, best_count, ev_hi, ev_lo, rule,
                           calls, max_calls, ctr);
}

} // namespace np2
