// Short-read adapter trimming in front of the k-mer counter: one piece of the separator stream and of its quality stream
// (mates adjacent in pair mode: read 2r is mate 1, read 2r + 1 mate 2) -> per read (begin, end, class, how, insert), the base
// stream masked in place, the totals.  The rule is np2_sradapt_core.hpp's; steps 1 - 3 and the masking are the quality
// filter's (np2_srqc_dev.hpp), so the count kernel reads the masked piece exactly as it reads np2_srqc.hip's.
//
// Layout: a persistent grid strides over the units (a pair, or a read in single mode), one wavefront per unit.
//   pack     the kept spans go to the wavefront's LDS as three bit planes each (code bit 0, code bit 1, unknown; base i in
//            bit i & 31 of word i >> 5): x forward, mate 2 reverse-complemented (read backward through byte-reversed words,
//            code ^ 2).  A lane turns one aligned group of 4 bytes into 4 bits per plane, 8 lanes' nibbles are or-ed
//            through three xor shuffles into one word.  6 planes of PLANE_WORDS words per wavefront; the words past a span
//            are zero, so that a funnel shift may read one word further.
//   overlap  one candidate shift per lane, 64 per pass, forward shifts first.  d(s) over 32-base words: the aligned operand
//            is the same LDS word in every lane (a broadcast), the shifted one is the funnel shift of two words whose index
//            differs between neighbouring lanes only where s crosses a multiple of 32 (two addresses per 32 lanes).  xor of
//            the planes, or of the two differences and the unknown bits, tail mask, popcount; a lane stops once it is over
//            its limit.  The winner is a ballot: the lowest lane of the first pass with a hit (forward: the smallest s;
//            backward: the s nearest to 0).
//   sequence the same with one start p per lane against the adapter's planes, which are kernel arguments (packed on the
//            host, once per call): 64 letters are two words per plane.
//   class    step 4 over the new spans, the pair rule, masking as k_srqc masks, the totals as k_srqc sums them.
// Every store to global memory is a vector store or plain C++.
//
// Memory the kernel may touch: as k_srqc, 8 bytes before and 16 bytes after the n bytes of either stream.
#include <hip/hip_runtime.h>

#include "np2_sradapt.hpp"
#include "np2_srqc_dev.hpp"

namespace np2 {
using namespace srqc_dev;
namespace ad = np2sradapt;

namespace {

static constexpr uint32_t AD_BLOCK = 256, AD_WAVES = AD_BLOCK / 64;
static constexpr uint32_t SPAN_WORDS = ad::MAX_SPAN / 32;  // 32
static constexpr uint32_t PLANE_WORDS = SPAN_WORDS + 3;    // a 64-bit funnel read at bit offset <= 1023 touches word 33
enum : uint32_t { P_LO = 0, P_HI = 1, P_UNK = 2, N_PLANES = 3 };
struct Packed {
    uint32_t w[N_PLANES][PLANE_WORDS];
};

// what a wavefront's lanes wrote to its LDS is visible to all of them afterwards (and the other way round)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The n <= 1024 bases from stream offset `at` forward (RC = 0), or the n bases before `at` backward and complemented.
template <int RC> __device__ __forceinline__ void pack(Packed &pk, const uint8_t *seq, int64_t at, uint32_t n, uint32_t lane) {
#pragma unroll 1
    for (uint32_t o = 0; o < ad::MAX_SPAN; o += 256) {
        const uint32_t ob = o + 4 * lane;
        uint32_t lo = 0, hi = 0, unk = 0;
        if (ob < n) {
            const uint32_t v = RC ? load4_back(seq, at - ob) : load4(seq, at + ob);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                if (ob + j < n) {
                    uint32_t c = ad::base_code(byte_of(v, j));
                    if (RC && c < 4u) c ^= 2u;
                    lo |= (c & 1u) << j, hi |= ((c >> 1) & 1u) << j, unk |= (c >> 2) << j;
                }
            }
        }
        const uint32_t sh = 4u * (lane & 7u);
        lo <<= sh, hi <<= sh, unk <<= sh;
#pragma unroll
        for (int x = 1; x < 8; x <<= 1) lo |= __shfl_xor(lo, x), hi |= __shfl_xor(hi, x), unk |= __shfl_xor(unk, x);
        if ((lane & 7u) == 0) {
            const uint32_t w = (o >> 5) + (lane >> 3);
            pk.w[P_LO][w] = lo, pk.w[P_HI][w] = hi, pk.w[P_UNK][w] = unk;
        }
    }
    if (lane < PLANE_WORDS - SPAN_WORDS) pk.w[P_LO][SPAN_WORDS + lane] = pk.w[P_HI][SPAN_WORDS + lane] = pk.w[P_UNK][SPAN_WORDS + lane] = 0;
    wave_lds_sync();
}

// 32 bits of a plane from bit offset `off`
__device__ __forceinline__ uint32_t bits_at(const uint32_t *plane, uint32_t off) {
    const uint32_t w = off >> 5;
    return (uint32_t)(((uint64_t)plane[w + 1] << 32 | plane[w]) >> (off & 31u));
}
__device__ __forceinline__ uint32_t tail_mask(uint32_t left) { return left >= 32u ? ~0u : (1u << left) - 1u; }

// positions of `len` where f[i] and g[off + i] are unknown or differ; may stop early with any value above `limit`
__device__ __forceinline__ uint32_t diffs(const Packed &f, const Packed &g, uint32_t off, uint32_t len, uint32_t limit) {
    uint32_t d = 0;
    for (uint32_t i = 0; i < len && d <= limit; i += 32) {
        const uint32_t w = i >> 5;
        const uint32_t m = (f.w[P_LO][w] ^ bits_at(g.w[P_LO], off + i)) | (f.w[P_HI][w] ^ bits_at(g.w[P_HI], off + i)) | f.w[P_UNK][w] |
                           bits_at(g.w[P_UNK], off + i);
        d += __popc(m & tail_mask(len - i));
    }
    return d;
}

// step A over the packed spans: true and the accepted shift
__device__ __forceinline__ bool find_overlap(const Packed &x, const Packed &rcy, uint32_t n1, uint32_t n2, const ad::Opts &o, uint32_t lane,
                                             int32_t &shift) {
    const uint32_t nf = ad::n_forward(n1, o), nb = ad::n_backward(n2, o);
    for (uint32_t s0 = 0; s0 < nf; s0 += 64) {
        const uint32_t s = s0 + lane;
        bool hit = false;
        if (s < nf) {
            const uint32_t len = ad::overlap_forward(n1, n2, s), lim = ad::diff_limit(len, o);
            hit = diffs(rcy, x, s, len, lim) <= lim;
        }
        const uint64_t bal = __ballot(hit);
        if (bal) return shift = (int32_t)(s0 + (uint32_t)__builtin_ctzll(bal)), true;
    }
    for (uint32_t t0 = 1; t0 <= nb; t0 += 64) {
        const uint32_t t = t0 + lane;
        bool hit = false;
        if (t <= nb) {
            const uint32_t len = ad::overlap_backward(n1, n2, t), lim = ad::diff_limit(len, o);
            hit = diffs(x, rcy, t, len, lim) <= lim;
        }
        const uint64_t bal = __ballot(hit);
        if (bal) return shift = -(int32_t)(t0 + (uint32_t)__builtin_ctzll(bal)), true;
    }
    return false;
}

// step B over the packed span of n bases: the winning p, or n
__device__ __forceinline__ uint32_t find_adapter(const Packed &x, uint32_t n, const ad::Opts &o, uint32_t which, uint32_t lane) {
    const uint32_t a_len = o.a_len[which];
    const uint64_t a_lo = o.a_lo[which], a_hi = o.a_hi[which];
    const uint32_t n_p = n - ad::MIN_ADAPTER + 1;
    for (uint32_t p0 = 0; p0 < n_p; p0 += 64) {
        const uint32_t p = p0 + lane;
        bool hit = false;
        if (p < n_p) {
            const uint32_t c = ad::seq_compared(n, p, a_len);
            const uint64_t lo = (uint64_t)bits_at(x.w[P_LO], p + 32) << 32 | bits_at(x.w[P_LO], p);
            const uint64_t hi = (uint64_t)bits_at(x.w[P_HI], p + 32) << 32 | bits_at(x.w[P_HI], p);
            const uint64_t unk = (uint64_t)bits_at(x.w[P_UNK], p + 32) << 32 | bits_at(x.w[P_UNK], p);
            const uint64_t m = ((lo ^ a_lo) | (hi ^ a_hi) | unk) & (c >= 64u ? ~0ull : (1ull << c) - 1ull);
            hit = (uint32_t)__popcll(m) <= ad::seq_limit(c);
        }
        const uint64_t bal = __ballot(hit);
        if (bal) return p0 + (uint32_t)__builtin_ctzll(bal);
    }
    return n;
}

struct Span {
    uint32_t start, n, a, b, b0, cls, how, insert;
};

__device__ __forceinline__ void span_of(const uint8_t *seq, const uint8_t *qual, const uint32_t *ends, uint32_t r, const np2srqc::Opts &qc,
                                        uint32_t lane, Span &sp) {
    sp.start = r ? ends[r - 1] + 1 : 0u, sp.n = ends[r] - sp.start;
    kept_span(seq, qual, sp.start, sp.n, qc, lane, sp.a, sp.b);
    sp.b0 = sp.b, sp.how = ad::HOW_NONE, sp.insert = 0, sp.cls = 0;
}
__device__ __forceinline__ void seq_step(Packed &pk, bool packed, const uint8_t *seq, const ad::Opts &o, uint32_t which, uint32_t lane,
                                         Span &sp) {
    const uint32_t n = sp.b - sp.a;
    if (!ad::seq_searchable(n, o.a_len[which])) return;
    if (!packed) pack<0>(pk, seq, (int64_t)sp.start + sp.a, n, lane);
    const uint32_t p = find_adapter(pk, n, o, which, lane);
    if (p < n) sp.b = sp.a + p, sp.how = ad::HOW_SEQ;
}
__device__ __forceinline__ void classify_span(const uint8_t *seq, const uint8_t *qual, const np2srqc::Opts &qc, uint32_t lane, Span &sp) {
    uint32_t n_n, lowq;
    span_counts(seq, qual, sp.start, sp.a, sp.b, qc, lane, n_n, lowq);
    sp.cls = classify(sp.b - sp.a, n_n, lowq, qc);
}
__device__ __forceinline__ void finish(uint8_t *seq, const Span &sp, uint32_t r, np2_sradapt_read_t *reads, unsigned long long *tot,
                                       uint32_t lane) {
    if (sp.cls == PASS) {
        mask_range(seq, sp.start, (uint64_t)sp.start + sp.a, lane);
        mask_range(seq, (uint64_t)sp.start + sp.b, (uint64_t)sp.start + sp.n, lane);
    } else {
        mask_range(seq, sp.start, (uint64_t)sp.start + sp.n, lane);
    }
    if (reads && lane == 0) reads[r] = np2_sradapt_read_t{sp.a, sp.b, sp.cls, sp.how, sp.insert};
    tot[T_READS] += 1, tot[T_BASES_IN] += sp.n, tot[T_BASES_OUT] += sp.cls == PASS ? sp.b - sp.a : 0u;
#pragma unroll
    for (uint32_t c = 0; c < N_CLASSES; ++c) tot[T_PASS + c] += sp.cls == c ? 1u : 0u;
    tot[ad::T_MATE_FAILED] += sp.cls == ad::MATE_FAILED ? 1u : 0u;
    tot[ad::T_TRIMMED_OVERLAP] += sp.how == ad::HOW_OVERLAP ? 1u : 0u, tot[ad::T_TRIMMED_SEQ] += sp.how == ad::HOW_SEQ ? 1u : 0u;
    tot[ad::T_ADAPTER_BASES] += sp.b0 - sp.b;
}

__global__ __launch_bounds__(AD_BLOCK) void k_sradapt(uint8_t *seq, const uint8_t *qual, const uint32_t *ends, uint32_t n_reads, np2srqc::Opts qc,
                                                     ad::Opts o, np2_sradapt_read_t *reads, unsigned long long *totals) {
    __shared__ Packed s_pk[AD_WAVES][2];
    __shared__ unsigned long long s_tot[AD_WAVES][ad::N_TOTALS];
    const uint32_t lane = threadIdx.x & 63, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t n_waves = gridDim.x * AD_WAVES;
    Packed &px = s_pk[wv][0], &py = s_pk[wv][1];
    unsigned long long tot[ad::N_TOTALS]; // (the same in every lane of the wavefront)
#pragma unroll
    for (uint32_t i = 0; i < ad::N_TOTALS; ++i) tot[i] = 0;
    if (o.flags & ad::PAIRED) {
        for (uint32_t u = blockIdx.x * AD_WAVES + wv; u < n_reads / 2; u += n_waves) {
            Span m1, m2;
            span_of(seq, qual, ends, 2 * u, qc, lane, m1);
            span_of(seq, qual, ends, 2 * u + 1, qc, lane, m2);
            const uint32_t n1 = m1.b - m1.a, n2 = m2.b - m2.a;
            int32_t shift = 0;
            bool found = false, x_packed = false;
            wave_lds_sync(); // the unit before has read its planes
            if (ad::searchable(n1, n2, o)) {
                pack<0>(px, seq, (int64_t)m1.start + m1.a, n1, lane);
                pack<1>(py, seq, (int64_t)m2.start + m2.b, n2, lane);
                x_packed = true;
                found = find_overlap(px, py, n1, n2, o, lane, shift);
            }
            if (found) {
                uint32_t k1, k2, insert;
                ad::accept(n1, n2, shift, k1, k2, insert);
                m1.insert = m2.insert = insert;
                if (k1 < n1) m1.b = m1.a + k1, m1.how = ad::HOW_OVERLAP;
                if (k2 < n2) m2.b = m2.a + k2, m2.how = ad::HOW_OVERLAP;
            } else {
                seq_step(px, x_packed, seq, o, 0, lane, m1);
                wave_lds_sync();
                seq_step(py, false, seq, o, 1, lane, m2);
            }
            classify_span(seq, qual, qc, lane, m1);
            classify_span(seq, qual, qc, lane, m2);
            if (m1.cls != PASS && m2.cls == PASS) m2.cls = ad::MATE_FAILED;
            else if (m2.cls != PASS && m1.cls == PASS) m1.cls = ad::MATE_FAILED;
            finish(seq, m1, 2 * u, reads, tot, lane);
            finish(seq, m2, 2 * u + 1, reads, tot, lane);
            tot[ad::T_PAIRS] += 1, tot[ad::T_PAIRS_OVERLAP] += found ? 1u : 0u, tot[ad::T_PAIRS_UNSEARCHED] += ad::past_cap(n1, n2) ? 1u : 0u;
        }
    } else {
        for (uint32_t r = blockIdx.x * AD_WAVES + wv; r < n_reads; r += n_waves) {
            Span m;
            span_of(seq, qual, ends, r, qc, lane, m);
            wave_lds_sync();
            seq_step(px, false, seq, o, 0, lane, m);
            classify_span(seq, qual, qc, lane, m);
            finish(seq, m, r, reads, tot, lane);
        }
    }
    if (lane == 0)
        for (uint32_t i = 0; i < ad::N_TOTALS; ++i) s_tot[wv][i] = tot[i];
    __syncthreads();
    if (threadIdx.x < ad::N_TOTALS) {
        unsigned long long v = 0;
        for (uint32_t w = 0; w < AD_WAVES; ++w) v += s_tot[w][threadIdx.x];
        if (v) atomicAdd(totals + threadIdx.x, v);
    }
}

} // namespace

void launch_sradapt(hipStream_t s, uint8_t *seq, const uint8_t *qual, const uint32_t *ends, uint32_t n_reads, const np2srqc::Opts &qc,
                    const np2sradapt::Opts &o, np2_sradapt_read_t *reads, uint64_t *totals) {
    const uint32_t units = (o.flags & ad::PAIRED) ? n_reads / 2 : n_reads;
    if (!units) return;
    const uint32_t want = (units + AD_WAVES - 1) / AD_WAVES;
    hipLaunchKernelGGL(k_sradapt, dim3(want < 2048u ? want : 2048u), dim3(AD_BLOCK), 0, s, seq, qual, ends, n_reads, qc, o, reads,
                       reinterpret_cast<unsigned long long *>(totals));
}

} // namespace np2
