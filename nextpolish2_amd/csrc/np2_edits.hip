// Where a polish changed its contig: the output's (base, position) pairs against the contig -> real edits, normalised,
// with the k-mer tables' verdict on each.  The rule is include/np2.h's (np2_edits_*); per-lane arithmetic is
// np2_edits_core.hpp's, which is also a one-lane host program.  wave64, gfx950.
//
//   k_edits_heads    over the output indices: positions checked (< L, non-decreasing: the error word, no fault), group
//                    start and end per position
//   k_edits_flags    over the positions: clean / dirty inside [first, last], run heads and run tails as two bitmaps (a
//                    wavefront's ballot is two words)
//   (look-back scans of the bitmaps' population counts: launch_scan_lb_popc, np2_cand.hip)
//   k_edits_runs     one lane per bitmap word: the r-th head and the r-th tail are raw run r
//   k_edits_trim     one lane per raw run: suffix, then prefix; runs with a side longer than 64 go on a list ...
//   k_edits_trim_wave ... and get a wavefront each: 64 bytes compared per step, the first mismatch by ballot
//   (look-back scan of the "real" flags: launch_scan_lb_excl)
//   k_edits_compact  real edits in run order
//   k_edits_shift    one lane per edit: kind, left-alignment against the previous edit's pre-shift end, the record, totals
//   (look-back scans of the REF / ALT lengths)
//   k_edits_emit     one wavefront per edit: the two string pools, rotated where the edit was shifted
//   k_edits_support  one wavefront per (edit, table): a lane per k-mer end of the two windows, bounded probes, wavefront sums
//
// Counts stay on the device (EditsDev): every kernel after the first reads the number of runs / edits there, is launched
// for a bound the host knows (at most (L + 1) / 2 runs) and returns at once when the error word is set.  Every loop is
// bounded: probes by the sub-table's capacity, a shift by s - lo, a trim by the shorter side.
#include <hip/hip_runtime.h>

#include "np2_edits.hpp"
#include "np2_kmerscan.hpp"

namespace np2 {
using namespace np2edits;

namespace {

static constexpr uint32_t EB = 256; // lanes of a block

// common suffix (SUFFIX) or prefix of ref[s .. s + lr) and out[o .. o + la) by one wavefront: 64 bytes per step
template <bool SUFFIX>
__device__ __forceinline__ uint32_t wave_common(const uint8_t *ref, const uint8_t *out, uint32_t s, uint32_t o, uint32_t lr, uint32_t la,
                                                uint32_t lane) {
    const uint32_t m = lr < la ? lr : la;
    for (uint32_t c0 = 0; c0 < m; c0 += 64) {
        const uint32_t i = c0 + lane;
        const bool eq = i < m && (SUFFIX ? same(ref[s + lr - 1 - i], out[o + la - 1 - i]) : same(ref[s + i], out[o + i]));
        const unsigned long long ne = ~__ballot(eq);
        if (ne) return c0 + (uint32_t)__builtin_ctzll(ne);
    }
    return m;
}

// a raw run's REF and ALT intervals before trimming; false: outside the arrays (never on checked input)
__device__ __forceinline__ bool run_bounds(const EditsSeq &q, const EditsDev *ctr, uint32_t s, uint32_t e, uint32_t &o_s, uint32_t &lr,
                                           uint32_t &la) {
    if (e < s || e >= q.L || s < ctr->first || e > ctr->last) return false;
    o_s = 0;
    uint32_t o_e = q.n;
    if (s > ctr->first) {
        const uint32_t g = q.gstart[s - 1];
        if (g >= q.n) return false;
        o_s = g + 1;
    }
    if (e < ctr->last) o_e = q.gstart[e + 1];
    if (o_e > q.n || o_e < o_s) return false;
    lr = e - s + 1;
    la = o_e - o_s;
    return true;
}

// one window of rule 6 by a wavefront: a lane per k-mer end
__device__ __forceinline__ void wave_window(const YakDev &y, uint32_t min_count, const uint8_t *seq, uint64_t n, uint64_t at, uint64_t len,
                                            uint32_t lane, uint32_t &n_kmers, uint32_t &n_absent) {
    uint64_t lo_end, hi;
    window(n, at, len, y.k, lo_end, hi);
    const uint64_t mask = np2kc::kmer_mask(y.k);
    uint32_t a = 0, b = 0;
    for (uint64_t e = lo_end + lane; e < hi; e += 64) {
        uint64_t h = 0;
        if (!kmer_at(seq, e, y.k, mask, &h)) continue;
        ++a;
        if (get_bounded(y, h, min_count) == 0) ++b;
    }
    n_kmers = wave_sum(a);
    n_absent = wave_sum(b);
}

} // namespace

// the contig as np2_contig_upload keeps it (nibble codes, position p in nibble p & 1 of byte p >> 1) -> ASCII
__global__ __launch_bounds__(EB) void k_edits_unpack_ref(const uint8_t *__restrict__ refnib, uint32_t L, uint8_t *__restrict__ ref) {
    const uint32_t p = blockIdx.x * EB + threadIdx.x;
    if (p >= L) return;
    const uint32_t c = (refnib[p >> 1] >> (4 * (p & 1))) & 7u;
    ref[p] = (uint8_t)((0x4E4D4E2D54474341ull >> (8 * c)) & 0xFF); // "ACGT-NMN"
}

__global__ __launch_bounds__(EB) void k_edits_heads(EditsSeq q, EditsDev *ctr) {
    const uint32_t i = blockIdx.x * EB + threadIdx.x;
    if (i >= q.n) return;
    const uint32_t p = q.pos[i];
    const uint32_t before = i ? q.pos[i - 1] : p, after = i + 1 < q.n ? q.pos[i + 1] : p;
    uint32_t bad = 0;
    if (p >= q.L) bad |= E_POS_RANGE;
    if (before > p) bad |= E_POS_ORDER;
    if (bad) {
        atomicOr(&ctr->err, bad);
        return;
    }
    if (i == 0 || before != p) q.gstart[p] = i;
    if (i + 1 == q.n || after != p) q.gend[p] = i + 1;
    if (i == 0) ctr->first = p, ctr->has_span = 1u;
    if (i + 1 == q.n) ctr->last = p;
}

__global__ __launch_bounds__(EB) void k_edits_flags(EditsSeq q, EditsDev *ctr, uint32_t *__restrict__ hbits, uint32_t *__restrict__ tbits,
                                                    uint32_t n_words) {
    const uint32_t p = blockIdx.x * EB + threadIdx.x;
    const bool live = ctr->err == 0 && ctr->has_span != 0 && ctr->first <= ctr->last;
    const uint32_t first = ctr->first, last = ctr->last;
    auto dirty = [&](uint32_t x) { return live && x >= first && x <= last && !clean(q.ref, q.out, q.gstart, q.gend, x); };
    bool head = false, tail = false;
    if (p < q.L && dirty(p)) {
        head = !(p > 0 && dirty(p - 1));
        tail = !(p + 1 < q.L && dirty(p + 1));
    }
    const unsigned long long hb = __ballot(head), tb = __ballot(tail);
    const uint32_t lane = threadIdx.x & 63u, w = (p >> 5);
    if ((lane == 0 || lane == 32) && w < n_words) {
        hbits[w] = (uint32_t)(hb >> lane);
        tbits[w] = (uint32_t)(tb >> lane);
    }
    if (p == 0) ctr->outside = live ? (unsigned long long)q.L - ((unsigned long long)last - first + 1ull) : (unsigned long long)q.L;
}

__global__ __launch_bounds__(EB) void k_edits_runs(const uint32_t *__restrict__ hbits, const uint32_t *__restrict__ tbits,
                                                   const uint32_t *__restrict__ hoff, const uint32_t *__restrict__ toff, uint32_t n_words,
                                                   EditsRuns r, EditsDev *ctr) {
    const uint32_t w = blockIdx.x * EB + threadIdx.x;
    if (w == 0) {
        const uint32_t nh = hoff[n_words], nt = toff[n_words];
        if (nh != nt || nh > r.max_runs) atomicOr(&ctr->err, E_INTERNAL);
        ctr->n_raw = nh <= r.max_runs ? nh : 0u;
    }
    if (w >= n_words || ctr->err) return;
    uint32_t b = hbits[w], at = hoff[w];
    while (b) { // (at most 32 turns)
        const uint32_t j = (uint32_t)__builtin_ctz(b);
        b &= b - 1;
        if (at < r.max_runs) r.run_s[at] = 32u * w + j;
        ++at;
    }
    b = tbits[w], at = toff[w];
    while (b) {
        const uint32_t j = (uint32_t)__builtin_ctz(b);
        b &= b - 1;
        if (at < r.max_runs) r.run_e[at] = 32u * w + j;
        ++at;
    }
}

__global__ __launch_bounds__(EB) void k_edits_trim(EditsSeq q, EditsRuns r, EditsDev *ctr) {
    const uint32_t i = blockIdx.x * EB + threadIdx.x;
    if (i >= r.max_runs) return;
    r.real[i] = 0; // (the scan runs over max_runs flags)
    if (ctr->err || i >= ctr->n_raw) return;
    uint32_t s = r.run_s[i], o_s, lr, la;
    if (!run_bounds(q, ctr, s, r.run_e[i], o_s, lr, la)) {
        atomicOr(&ctr->err, E_INTERNAL);
        return;
    }
    if (lr > WAVE_SIDE || la > WAVE_SIDE) {
        r.long_list[atomicAdd(&ctr->n_long, 1u)] = i; // (n_long <= n_raw <= max_runs)
        return;
    }
    trim(q.ref, q.out, s, o_s, lr, la);
    r.t_s[i] = s, r.t_os[i] = o_s, r.t_lr[i] = lr, r.t_la[i] = la;
    r.real[i] = (lr | la) ? 1u : 0u;
}

__global__ __launch_bounds__(EB) void k_edits_trim_wave(EditsSeq q, EditsRuns r, EditsDev *ctr) {
    if (ctr->err) return;
    const uint32_t lane = threadIdx.x & 63u, n_long = ctr->n_long <= r.max_runs ? ctr->n_long : 0u;
    for (uint32_t w = (blockIdx.x * EB + threadIdx.x) >> 6; w < n_long; w += (gridDim.x * EB) >> 6) {
        const uint32_t i = r.long_list[w];
        if (i >= r.max_runs) continue;
        uint32_t s = r.run_s[i], o_s, lr, la;
        if (!run_bounds(q, ctr, s, r.run_e[i], o_s, lr, la)) continue; // (k_edits_trim saw the same bounds)
        const uint32_t suf = wave_common<true>(q.ref, q.out, s, o_s, lr, la, lane);
        lr -= suf, la -= suf;
        const uint32_t pre = wave_common<false>(q.ref, q.out, s, o_s, lr, la, lane);
        s += pre, o_s += pre, lr -= pre, la -= pre;
        if (lane == 0) {
            r.t_s[i] = s, r.t_os[i] = o_s, r.t_lr[i] = lr, r.t_la[i] = la;
            r.real[i] = (lr | la) ? 1u : 0u;
        }
    }
}

__global__ __launch_bounds__(EB) void k_edits_compact(EditsRuns r, const uint32_t *__restrict__ eidx, EditsList e, EditsDev *ctr) {
    const uint32_t i = blockIdx.x * EB + threadIdx.x;
    if (ctr->err) return;
    if (i == 0) {
        const uint32_t n = eidx[r.max_runs];
        ctr->n_edits = n <= ctr->n_raw ? n : 0u;
        ctr->same_runs = n <= ctr->n_raw ? ctr->n_raw - n : 0u;
    }
    if (i >= ctr->n_raw || !r.real[i]) return;
    const uint32_t at = eidx[i];
    if (at >= r.max_runs) return;
    e.s0[at] = r.t_s[i], e.os0[at] = r.t_os[i], e.lr[at] = r.t_lr[i], e.la[at] = r.t_la[i];
}

__global__ __launch_bounds__(EB) void k_edits_shift(EditsSeq q, EditsList e, uint32_t max_runs, EditsDev *ctr) {
    const uint32_t i = blockIdx.x * EB + threadIdx.x;
    if (ctr->err) return; // (uniform)
    const bool on = i < ctr->n_edits && i < max_runs;
    uint32_t kind = 5, ins = 0, del = 0;
    if (on) {
        const uint32_t s = e.s0[i], o_s = e.os0[i], lr = e.lr[i], la = e.la[i];
        kind = kind_of(lr, la);
        uint32_t lo = ctr->first;
        if (i) {
            const uint32_t pe = e.s0[i - 1] + e.lr[i - 1]; // the previous edit's end before its own shift
            lo = pe > lo ? pe : lo;
        }
        if (s - lo > o_s) lo = s - o_s; // (never on checked input: output and contig run in lock step between two edits)
        uint32_t sh = 0;
        if (s >= lo) {
            if (kind == INS) sh = shift_of(q.ref, q.out + o_s, la, s, lo);
            if (kind == DEL) sh = shift_of(q.ref, q.ref + s, lr, s, lo);
        }
        e.sh[i] = sh;
        e.rec[i] = Edit{s - sh, lr, o_s - sh, la, kind};
        ins = la > lr ? la - lr : 0u;
        del = lr > la ? lr - la : 0u;
    }
    // totals: a wavefront's sums, one atomic per counter
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k) {
        const uint32_t c = (uint32_t)__popcll(__ballot(kind == k));
        if (lane == 0 && c) atomicAdd(&ctr->n_kind[k], c);
    }
    const uint32_t si = wave_sum(ins), sd = wave_sum(del);
    if (lane == 0 && si) atomicAdd(&ctr->bases_inserted, (unsigned long long)si);
    if (lane == 0 && sd) atomicAdd(&ctr->bases_deleted, (unsigned long long)sd);
}

__global__ __launch_bounds__(EB) void k_edits_emit(EditsSeq q, EditsList e, const uint32_t *__restrict__ roff, const uint32_t *__restrict__ aoff,
                                                   uint32_t max_runs, uint8_t *__restrict__ ref_pool, uint8_t *__restrict__ alt_pool, EditsDev *ctr) {
    if (ctr->err) return;
    const uint32_t lane = threadIdx.x & 63u, n_edits = ctr->n_edits <= max_runs ? ctr->n_edits : 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctr->ref_bytes = roff[max_runs], ctr->alt_bytes = aoff[max_runs];
    for (uint32_t i = (blockIdx.x * EB + threadIdx.x) >> 6; i < n_edits; i += (gridDim.x * EB) >> 6) {
        const uint32_t s = e.s0[i], o_s = e.os0[i], lr = e.lr[i], la = e.la[i], sh = e.sh[i], kind = kind_of(lr, la);
        const uint32_t r0 = roff[i], a0 = aoff[i];
        // (REF bytes in all <= last - first + 1 <= L, ALT bytes <= n: the pools' sizes)
        if ((uint64_t)r0 + lr > q.L || (uint64_t)a0 + la > q.n || (uint64_t)s + lr > q.L || (uint64_t)o_s + la > q.n) continue;
        for (uint32_t j = lane; j < lr; j += 64) ref_pool[r0 + j] = q.ref[s + (kind == DEL ? rot_src(j, lr, sh) : j)];
        for (uint32_t j = lane; j < la; j += 64) alt_pool[a0 + j] = q.out[o_s + (kind == INS ? rot_src(j, la, sh) : j)];
    }
}

__global__ __launch_bounds__(EB) void k_edits_support(EditsSeq q, EditsList e, EditsTables t, uint32_t *__restrict__ sup, uint32_t max_runs,
                                                      const EditsDev *ctr) {
    if (ctr->err) return;
    const uint32_t lane = threadIdx.x & 63u, n_edits = ctr->n_edits <= max_runs ? ctr->n_edits : 0u;
    const uint64_t jobs = (uint64_t)n_edits * t.n;
    for (uint64_t w = ((uint64_t)blockIdx.x * EB + threadIdx.x) >> 6; w < jobs; w += ((uint64_t)gridDim.x * EB) >> 6) {
        const uint32_t i = (uint32_t)(w / t.n), ti = (uint32_t)(w % t.n);
        const Edit r = e.rec[i];
        uint32_t c[4];
        wave_window(t.y[ti], t.min_count, q.ref, q.L, r.ref_pos, r.ref_len, lane, c[0], c[1]);
        wave_window(t.y[ti], t.min_count, q.out, q.n, r.out_off, r.alt_len, lane, c[2], c[3]);
        if (lane == 0) *reinterpret_cast<uint4 *>(sup + 4 * w) = make_uint4(c[0], c[1], c[2], c[3]);
    }
}

static dim3 grid_of(uint64_t n) { return dim3((uint32_t)((n + EB - 1) / EB)); }

void launch_edits_unpack_ref(hipStream_t s, const uint8_t *refnib, uint32_t L, uint8_t *ref) {
    if (L) hipLaunchKernelGGL(k_edits_unpack_ref, grid_of(L), dim3(EB), 0, s, refnib, L, ref);
}
void launch_edits_heads(hipStream_t s, const EditsSeq &q, EditsDev *ctr) {
    if (q.n) hipLaunchKernelGGL(k_edits_heads, grid_of(q.n), dim3(EB), 0, s, q, ctr);
}
void launch_edits_flags(hipStream_t s, const EditsSeq &q, EditsDev *ctr, uint32_t *hbits, uint32_t *tbits, uint32_t n_words) {
    if (q.L) hipLaunchKernelGGL(k_edits_flags, grid_of(q.L), dim3(EB), 0, s, q, ctr, hbits, tbits, n_words);
}
void launch_edits_runs(hipStream_t s, const uint32_t *hbits, const uint32_t *tbits, const uint32_t *hoff, const uint32_t *toff,
                       uint32_t n_words, const EditsRuns &r, EditsDev *ctr) {
    hipLaunchKernelGGL(k_edits_runs, grid_of(n_words ? n_words : 1), dim3(EB), 0, s, hbits, tbits, hoff, toff, n_words, r, ctr);
}
void launch_edits_trim(hipStream_t s, const EditsSeq &q, const EditsRuns &r, EditsDev *ctr, uint32_t wave_blocks) {
    hipLaunchKernelGGL(k_edits_trim, grid_of(r.max_runs), dim3(EB), 0, s, q, r, ctr);
    hipLaunchKernelGGL(k_edits_trim_wave, dim3(wave_blocks ? wave_blocks : 1u), dim3(EB), 0, s, q, r, ctr);
}
void launch_edits_compact(hipStream_t s, const EditsRuns &r, const uint32_t *eidx, const EditsList &e, EditsDev *ctr) {
    hipLaunchKernelGGL(k_edits_compact, grid_of(r.max_runs), dim3(EB), 0, s, r, eidx, e, ctr);
}
void launch_edits_shift(hipStream_t s, const EditsSeq &q, const EditsList &e, uint32_t max_runs, EditsDev *ctr) {
    hipLaunchKernelGGL(k_edits_shift, grid_of(max_runs), dim3(EB), 0, s, q, e, max_runs, ctr);
}
void launch_edits_emit(hipStream_t s, const EditsSeq &q, const EditsList &e, const uint32_t *roff, const uint32_t *aoff, uint32_t max_runs,
                       uint8_t *ref_pool, uint8_t *alt_pool, EditsDev *ctr, uint32_t blocks) {
    hipLaunchKernelGGL(k_edits_emit, dim3(blocks ? blocks : 1u), dim3(EB), 0, s, q, e, roff, aoff, max_runs, ref_pool, alt_pool, ctr);
}
void launch_edits_support(hipStream_t s, const EditsSeq &q, const EditsList &e, const EditsTables &t, uint32_t *sup, uint32_t max_runs,
                          const EditsDev *ctr, uint32_t blocks) {
    if (t.n) hipLaunchKernelGGL(k_edits_support, dim3(blocks ? blocks : 1u), dim3(EB), 0, s, q, e, t, sup, max_runs, ctr);
}

} // namespace np2
