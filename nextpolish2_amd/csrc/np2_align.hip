// The aligner's kernels (gfx950): a mapped read's primary chain to a base-level alignment.  The rule: include/np2_io.h,
// np2_map_align_*; every decision is np2_align_core.hpp's text, shared with the host aligner.
//
//   k_align_pins, k_align_plan    one lane per read walks the exported chain (as k_map_chain's lane 0 walks its anchors): pin
//                                 flags and pins + 1 slots, around a scan of the slot counts
//   k_align_classify              one thread per slot: equality test, prefix and suffix trim, class, band and cells
//   k_align_dp                    one wavefront per slot with a matrix.  Lanes lie across the band's diagonals, 64 at a time; the
//                                 previous row's H and F stay in LDS and are overwritten in place (a cell reads slots L and
//                                 L + 1, then writes L).  The in-row dependency of E is a prefix maximum: E(L) = max over L' < L
//                                 of (H~(L') - gap_open + L' gap_ext) - L gap_ext with H~ = max(diagonal, F), which has the
//                                 values of the sequential recurrence because a gap opened from a cell that itself ends a
//                                 deletion never beats extending that deletion.  One byte of traceback bits per cell goes to
//                                 the group's budgeted buffer, rows of W bytes, written 64 in a row.
//   k_align_ops_count, _emit      around a scan: one lane per read counts the raw ops; then one wavefront per read, whose lane 0
//                                 walks back through the bits, concatenates clip, extensions, pins and segments and
//                                 left-aligns, and whose 64 lanes share the columns for NM and AS
#include "np2_align.hpp"

namespace np2 {
using namespace np2aln;

__global__ __launch_bounds__(64) void k_align_pins(AlignJob c) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i > c.n_reads) return;
    uint32_t ns = 0;
    if (i < c.n_reads) {
        const np2map::Hit &h = hit_of(c, i);
        if (h.tid >= 0) ns = mark_pins(c.chain + 2 * (uint64_t)c.coff[i], h.n, c.k, c.pin + c.coff[i]) + 1u;
    }
    c.nslots[i] = ns;
}

__global__ __launch_bounds__(64) void k_align_plan(AlignJob c) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= c.n_reads) return;
    const uint32_t s0 = c.soff[i], s1 = c.soff[i + 1];
    if (s1 == s0) return;
    const np2map::Hit &h = hit_of(c, i);
    const uint32_t t_at = h.tid > 0 ? c.asm_ends[h.tid - 1] + 1u : 0u;
    plan_read(c.chain + 2 * (uint64_t)c.coff[i], h.n, c.k, c.pin + c.coff[i], c.asm_ends[h.tid] - t_at, h.qlen, c.o, c.slots + s0);
    for (uint32_t s = s0; s < s1; ++s) c.slot_read[s] = i;
}

// (the counters are summed over a wavefront first: one atomic per wavefront and counter, not one per slot on one address)
__global__ __launch_bounds__(256) void k_align_classify(AlignJob c, uint32_t n_slots) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    uint32_t kind = K_EMPTY, cells = 0, pins = 0;
    if (s < n_slots) {
        const uint32_t i = c.slot_read[s];
        const Seqs q = seqs_of(c, i);
        Slot x = c.slots[s];
        cells = (uint32_t)classify(q, x, c.o, c.max_cells); // (<= max_cells <= 2^24)
        c.slots[s] = x;
        kind = x.kind;
        if (s == c.soff[i]) pins = c.soff[i + 1] - c.soff[i] - 1u; // the read's first slot counts its pins (<= 2^31 / k)
    }
    if (s <= n_slots) c.cells[s] = cells;
    unsigned long long cells_sum = cells, pins_sum = pins, reads_sum = pins ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) {
        cells_sum += __shfl_xor(cells_sum, o), pins_sum += __shfl_xor(pins_sum, o), reads_sum += __shfl_xor(reads_sum, o);
    }
    unsigned long long n_kind[4];
    for (uint32_t k = 0; k < 4; ++k) n_kind[k] = (unsigned long long)__popcll(__ballot(kind == k));
    if ((threadIdx.x & 63u) == 0) {
        for (uint32_t k = 0; k < 4; ++k)
            if (n_kind[k]) atomicAdd(&c.ctr[C_EQUAL + k], n_kind[k]);
        if (cells_sum) atomicAdd(&c.ctr[C_CELLS], cells_sum);
        if (pins_sum) atomicAdd(&c.ctr[C_PINS], pins_sum), atomicAdd(&c.ctr[C_SEGMENTS], pins_sum - reads_sum);
    }
}

__global__ __launch_bounds__(256) void k_align_read_cells(AlignJob c) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i <= c.n_reads) c.read_cells[i] = c.tb_off[c.soff[i]];
}

__global__ __launch_bounds__(64) void k_align_dp(AlignJob c, uint32_t s0, uint64_t tb_base) {
    __shared__ int32_t sH[MAX_W + 1], sF[MAX_W + 1];
    const uint32_t slot = s0 + blockIdx.x, lane = threadIdx.x;
    if (c.cells[slot] == 0) return; // (the whole block)
    const Slot x = c.slots[slot];
    const uint32_t rd = c.slot_read[slot];
    const Seqs s = seqs_of(c, rd);
    const Opts o = c.o;
    uint8_t *tb = c.tb + (c.tb_off[slot] - tb_base);
    const uint32_t W = x.W;
    const int32_t go = (int32_t)o.gap_open, ge = (int32_t)o.gap_ext;
    for (uint32_t L = lane; L <= W; L += 64) {
        const int32_t j = x.lo + (int32_t)L;
        const bool in = L < W && j >= 0 && j <= (int32_t)x.tl;
        sH[L] = in ? row0_h((uint32_t)j, o) : NEG, sF[L] = NEG;
        if (L < W) tb[L] = in ? (uint8_t)row0_tb((uint32_t)j) : (uint8_t)0;
    }
    __syncthreads();
    int32_t bh = 0, eh = NEG;
    uint32_t bi = 0, bj = 0, ej = 0;
#pragma unroll 1
    for (uint32_t i = 1; i <= x.ql; ++i) {
        const uint32_t qb = slot_q(s, x, i - 1);
        int32_t carry = NEG, hl_c = NEG, el_c = NEG;
        uint8_t *row = tb + (uint64_t)i * W;
#pragma unroll 1
        for (uint32_t base = 0; base < W; base += 64) {
            const uint32_t L = base + lane;
            const bool act = L < W;
            const int32_t j = (int32_t)i + x.lo + (int32_t)L;
            const bool valid = act && j >= 0 && j <= (int32_t)x.tl;
            const int32_t hd = act ? sH[L] : NEG, hu = act ? sH[L + 1] : NEG, fu = act ? sF[L + 1] : NEG;
            __syncthreads();
            uint32_t cf, src;
            const int32_t d = valid && j > 0 ? hd + sub_score(slot_t(s, x, (uint32_t)j - 1u), qb, o) : NEG;
            int32_t f = gap_of(hu, fu, o, &cf);
            const int32_t ht = d > f ? d : f;
            int32_t p = valid ? ht - go + (int32_t)L * ge : NEG; // the prefix maximum's term
            for (int off = 1; off < 64; off <<= 1) {
                const int32_t t = __shfl_up(p, off);
                if ((int)lane >= off && t > p) p = t;
            }
            int32_t ex = __shfl_up(p, 1);
            if (lane == 0 || carry > ex) ex = carry;
            const int32_t top = __shfl(p, 63);
            if (top > carry) carry = top;
            int32_t e = ex - (int32_t)L * ge;
            int32_t h = h_of(d, e, f, &src);
            if (!valid) h = NEG, e = NEG, f = NEG;
            int32_t hl = __shfl_up(h, 1), el = __shfl_up(e, 1);
            if (lane == 0) hl = hl_c, el = el_c;
            hl_c = __shfl(h, 63), el_c = __shfl(e, 63);
            const uint32_t ce = el >= hl - go ? 1u : 0u;
            if (act) {
                row[L] = valid ? (uint8_t)(src | ce << 2 | cf << 3) : (uint8_t)0;
                sH[L] = h, sF[L] = f;
            }
            if (valid && h > bh) bh = h, bi = i, bj = (uint32_t)j;
            if (valid && i == x.ql && h > eh) eh = h, ej = (uint32_t)j;
            __syncthreads();
        }
    }
    if (x.kind == K_CORE) {
        if (lane == 0) c.res[slot] = Res{sH[(uint32_t)((int32_t)x.tl - (int32_t)x.ql - x.lo)], x.ql, x.tl};
        return;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t h2 = __shfl_xor(bh, off), e2 = __shfl_xor(eh, off);
        const uint32_t i2 = __shfl_xor(bi, off), j2 = __shfl_xor(bj, off), ej2 = __shfl_xor(ej, off);
        if (better_cell(h2, i2, j2, bh, bi, bj)) bh = h2, bi = i2, bj = j2;
        if (e2 > eh || (e2 == eh && ej2 < ej)) eh = e2, ej = ej2;
    }
    if (lane == 0) {
        const uint32_t rem = x.kind == K_HEAD ? x.q0 : s.qlen - x.q0;
        c.res[slot] = choose_end(bh, bi, bj, slot_has_end(x, rem), eh, ej, x.ql, o);
    }
}

namespace {
__device__ __forceinline__ ReadIn read_in(const AlignJob &c, uint32_t i, uint64_t tb_base) {
    const uint32_t s0 = c.soff[i];
    ReadIn in;
    in.s = seqs_of(c, i);
    in.chain = c.chain + 2 * (uint64_t)c.coff[i], in.pin = c.pin + c.coff[i];
    in.n = hit_of(c, i).n, in.k = c.k;
    in.slots = c.slots + s0, in.res = c.res + s0, in.tb_off = c.tb_off + s0, in.tb = c.tb, in.tb_base = tb_base;
    in.n_slots = c.soff[i + 1] - s0;
    return in;
}
} // namespace

__global__ __launch_bounds__(64) void k_align_ops_count(AlignJob c, uint32_t g0, uint32_t g1, uint64_t tb_base) {
    const uint32_t i = g0 + blockIdx.x * 64 + threadIdx.x;
    if (i > g1) return;
    uint32_t n = 0;
    if (i < g1 && c.soff[i + 1] > c.soff[i]) {
        const ReadIn in = read_in(c, i, tb_base);
        uint32_t t_start;
        if (!read_over(in)) n = raw_ops(in, nullptr, &t_start);
    }
    c.nops[i] = n;
}

// One wavefront per read.  Lane 0 builds the raw ops and the final CIGAR (a read's walk is sequential); then the 64 lanes share
// the M runs' columns for NM and AS, which is most of the bytes a read's assembly touches.
__global__ __launch_bounds__(64) void k_align_ops_emit(AlignJob c, uint32_t g0, uint32_t g1, uint64_t tb_base) {
    __shared__ Rec s_rec;
    const uint32_t i = g0 + blockIdx.x, lane = threadIdx.x;
    const bool mapped = c.soff[i + 1] > c.soff[i];
    ReadIn in{};
    if (mapped) in = read_in(c, i, tb_base);
    const uint32_t *b = c.b + 2 * (uint64_t)c.ooff[i] + 2 * (uint64_t)(i - g0);
    if (lane == 0) {
        Rec rec = unaligned_rec();
        if (mapped && read_over(in)) {
            atomicAdd(&c.ctr[C_OVERFLOW], 1ull);
        } else if (mapped) {
            uint32_t *a = c.a + c.ooff[i];
            uint32_t t_start;
            const uint32_t n = raw_ops(in, a, &t_start);
            const np2map::Hit &h = hit_of(c, i);
            rec.tid = h.tid, rec.flag = h.rev ? 16u : 0u, rec.mapq = h.mapq;
            const uint32_t clipped = finish_ops(in.s, a, n, t_start, c.o, c.b + 2 * (uint64_t)c.ooff[i] + 2 * (uint64_t)(i - g0), &rec);
            atomicAdd(&c.ctr[C_CLIPPED], (unsigned long long)clipped);
        }
        s_rec = rec;
    }
    __syncthreads(); // (lane 0's CIGAR words are visible to the block)
    const Rec rec = s_rec;
    uint32_t nm = 0, end = 0;
    int32_t as = 0;
    if (rec.tid >= 0) score_ops(in.s, b, rec.n_cigar, rec.pos, c.o, lane, 64u, &nm, &as, &end);
    for (int o = 32; o > 0; o >>= 1) nm += __shfl_xor(nm, o), as += __shfl_xor(as, o);
    if (lane == 0) {
        Rec out = rec;
        out.nm = nm, out.as = as, out.end = end;
        c.recs[i] = out;
    }
}

void launch_align_pins(hipStream_t s, const AlignJob &c) {
    hipLaunchKernelGGL(k_align_pins, dim3((c.n_reads + 1 + 63) / 64), dim3(64), 0, s, c);
}
void launch_align_plan(hipStream_t s, const AlignJob &c) {
    if (c.n_reads == 0) return;
    hipLaunchKernelGGL(k_align_plan, dim3((c.n_reads + 63) / 64), dim3(64), 0, s, c);
}
void launch_align_classify(hipStream_t s, const AlignJob &c, uint32_t n_slots) {
    hipLaunchKernelGGL(k_align_classify, dim3((n_slots + 1 + 255) / 256), dim3(256), 0, s, c, n_slots);
}
void launch_align_read_cells(hipStream_t s, const AlignJob &c) {
    hipLaunchKernelGGL(k_align_read_cells, dim3((c.n_reads + 1 + 255) / 256), dim3(256), 0, s, c);
}
void launch_align_dp(hipStream_t s, const AlignJob &c, uint32_t s0, uint32_t s1, uint64_t tb_base) {
    if (s1 <= s0) return;
    hipLaunchKernelGGL(k_align_dp, dim3(s1 - s0), dim3(64), 0, s, c, s0, tb_base);
}
void launch_align_ops_count(hipStream_t s, const AlignJob &c, uint32_t g0, uint32_t g1, uint64_t tb_base) {
    hipLaunchKernelGGL(k_align_ops_count, dim3((g1 - g0 + 1 + 63) / 64), dim3(64), 0, s, c, g0, g1, tb_base);
}
void launch_align_ops_emit(hipStream_t s, const AlignJob &c, uint32_t g0, uint32_t g1, uint64_t tb_base) {
    if (g1 <= g0) return;
    hipLaunchKernelGGL(k_align_ops_emit, dim3(g1 - g0), dim3(64), 0, s, c, g0, g1, tb_base);
}

} // namespace np2
