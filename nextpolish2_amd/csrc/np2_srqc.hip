// Short-read quality filter in front of the k-mer counter: one piece of the separator stream and of its quality stream ->
// per read (begin, end, class), the base stream masked in place, the totals.  The rule is np2_srqc_core.hpp's.
//
// Layout: a persistent grid strides over the reads, one wavefront per read (reads are 100 .. 300 bases: one pass of 64
// lanes x 4 bytes covers 256 of them, so nearly every step below is a single pass; any length and any W <= 1000 go
// through the same loops).  Every load is a lane's aligned 4-byte word (an unaligned group of 4 bytes is the funnel shift
// of two neighbouring aligned words); no lane walks a read.
//   windows  ws(u + 1) = ws(u) + p[entering] - p[leaving]: a lane takes 4 consecutive differences, a wave add-scan of the
//            lanes' sums plus the carry of the pass before gives every window's sum; the first window at or above M * W
//            is a ballot.  The front cut scans forward from a, the tail cut backward from b (a byte-reversed word), so
//            both stop at the first hit.  ws(0) is a wave reduction over the first (last) W values.
//   N skip   the same ballots over the base bytes, forward from the front cut and backward from the tail cut.
//   class    nN and lowq over [a, b) from the aligned words that cover it, two wave reductions.
//   mask     bytes of the read outside the kept span (all of a failed read) become 'N'.  Nothing is loaded for it: a word
//            that lies wholly inside the range to mask is one 4-byte store, the bytes of a word that the range shares
//            with anything else (the separator, a neighbouring read, the kept span) are byte stores.  A shared word is
//            owned by nobody: every read writes its own bytes of it and never a neighbour's, so no store carries a stale
//            copy of a byte another wavefront may be rewriting, and a separator is never written.
//   totals   kept per wavefront in registers, summed per block through LDS, one 64-bit atomic per block and counter.
// Traffic: 2 bytes read (base, quality) and at most 1 written per base; no table traffic.
//
// Memory the kernel may touch: 8 bytes before and 16 bytes after the n bytes of either stream must be readable (the
// counter's pieces have HALO bytes in front and 64 behind); what is read there enters no result.
#include <hip/hip_runtime.h>

#include "np2_srqc.hpp"
#include "np2_srqc_dev.hpp"

namespace np2 {
using namespace np2srqc;
using namespace srqc_dev;

namespace {

__global__ __launch_bounds__(SRQC_BLOCK) void k_srqc(uint8_t *seq, const uint8_t *qual, const uint32_t *ends, uint32_t n_reads, Opts o,
                                                    np2_srqc_read_t *reads, unsigned long long *totals) {
    __shared__ unsigned long long s_tot[SRQC_WAVES][N_TOTALS];
    const uint32_t lane = threadIdx.x & 63, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t n_waves = gridDim.x * SRQC_WAVES;
    unsigned long long tot[N_TOTALS] = {0, 0, 0, 0, 0, 0, 0}; // (the same in every lane of the wavefront)
    for (uint32_t r = blockIdx.x * SRQC_WAVES + wv; r < n_reads; r += n_waves) {
        const uint32_t start = r ? ends[r - 1] + 1 : 0u, n = ends[r] - start;
        uint32_t a, b, n_n, lowq;
        kept_span(seq, qual, start, n, o, lane, a, b);
        span_counts(seq, qual, start, a, b, o, lane, n_n, lowq);
        const uint32_t cls = classify(b - a, n_n, lowq, o);
        if (cls == PASS) {
            mask_range(seq, start, (uint64_t)start + a, lane);
            mask_range(seq, (uint64_t)start + b, (uint64_t)start + n, lane);
        } else {
            mask_range(seq, start, (uint64_t)start + n, lane);
        }
        if (reads && lane == 0) reads[r] = np2_srqc_read_t{a, b, cls};
        tot[T_READS] += 1, tot[T_BASES_IN] += n, tot[T_BASES_OUT] += cls == PASS ? b - a : 0u;
#pragma unroll
        for (uint32_t c = 0; c < N_CLASSES; ++c) tot[T_PASS + c] += cls == c ? 1u : 0u;
    }
    if (lane == 0)
        for (uint32_t i = 0; i < N_TOTALS; ++i) s_tot[wv][i] = tot[i];
    __syncthreads();
    if (threadIdx.x < N_TOTALS) {
        unsigned long long v = 0;
        for (uint32_t w = 0; w < SRQC_WAVES; ++w) v += s_tot[w][threadIdx.x];
        if (v) atomicAdd(totals + threadIdx.x, v);
    }
}

} // namespace

void launch_srqc(hipStream_t s, uint8_t *seq, const uint8_t *qual, const uint32_t *ends, uint32_t n_reads, const Opts &o,
                 np2_srqc_read_t *reads, uint64_t *totals) {
    if (!n_reads) return;
    const uint32_t want = (n_reads + SRQC_WAVES - 1) / SRQC_WAVES;
    hipLaunchKernelGGL(k_srqc, dim3(want < 2048u ? want : 2048u), dim3(SRQC_BLOCK), 0, s, seq, qual, ends, n_reads, o, reads,
                       reinterpret_cast<unsigned long long *>(totals));
}

} // namespace np2
