// The tag kernels (gfx950): MD, the short cs and the = / X CIGAR of aligned records.  The rule: include/np2_io.h,
// np2_map_align_*, "Tags"; every decision is np2_aligntags_core.hpp's text, shared with the host twin.
//
//   k_align_tags_size, _emit      around three scans: one wavefront per record, like k_align_ops_emit.  The 64 lanes take an M
//                                 word's columns 64 at a time: each compares one column (consecutive reference bytes, and
//                                 consecutive read bytes in either direction), the ballot of the mismatches is the same 64-bit
//                                 mask in every lane, and its few set bits are consumed in order, which advances MD's counter,
//                                 cs's run and the open = / X run in all lanes alike; lane 0 writes the digits and the single
//                                 letters, all lanes copy the letters of a D or I word.  A read of len columns with e events
//                                 costs about len / 64 + e steps.  No atomics; every store is a lane's own.
#include "np2_aligntags.hpp"

namespace np2 {
using namespace np2aln;

namespace {

__device__ __forceinline__ TagIn tag_in(const TagJob &j, uint32_t i) {
    TagIn in{};
    if (j.from_aligner) {
        const uint32_t rd = j.g0 + i;
        const Rec rec = j.c.recs[rd];
        if (rec.tid < 0) return in; // (n_cigar 0)
        const Seqs s = seqs_of(j.c, rd);
        in.t = s.t + rec.pos, in.q = s.q, in.qlen = s.qlen, in.rev = s.rev;
        in.cigar = j.c.b + 2 * (uint64_t)j.c.ooff[rd] + 2 * (uint64_t)i, in.n_cigar = rec.n_cigar;
    } else {
        in.t = j.ref + j.t_off[i], in.q = j.reads + j.q_off[i];
        in.cigar = j.cigar + j.cig_off[i], in.n_cigar = (uint32_t)(j.cig_off[i + 1] - j.cig_off[i]);
    }
    return in;
}

struct WaveBallot {
    __device__ __forceinline__ uint64_t operator()(bool b) const { return __ballot(b); }
};

} // namespace

__global__ __launch_bounds__(64) void k_align_tags_size(TagJob j) {
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    TagOut out{};
    if (i < j.n) {
        const TagIn in = tag_in(j, i);
        tag_walk(in, out, lane, 64u, WaveBallot());
    }
    if (lane == 0) {
        j.n_md[i] = j.flags & ALN_MD ? out.n_md : 0u;
        j.n_cs[i] = j.flags & ALN_CS ? out.n_cs : 0u;
        j.n_eqx[i] = j.flags & ALN_EQX ? out.n_eqx : 0u;
    }
}

__global__ __launch_bounds__(64) void k_align_tags_emit(TagJob j) {
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    const TagIn in = tag_in(j, i);
    TagOut out{};
    out.md = j.flags & ALN_MD ? j.md + j.md_off[i] : nullptr;
    out.cs = j.flags & ALN_CS ? j.cs + j.cs_off[i] : nullptr;
    out.eqx = j.flags & ALN_EQX ? j.eqx + j.eqx_off[i] : nullptr;
    tag_walk(in, out, lane, 64u, WaveBallot());
}

void launch_align_tags_size(hipStream_t s, const TagJob &j) {
    hipLaunchKernelGGL(k_align_tags_size, dim3(j.n + 1), dim3(64), 0, s, j);
}
void launch_align_tags_emit(hipStream_t s, const TagJob &j) {
    if (j.n == 0) return;
    hipLaunchKernelGGL(k_align_tags_emit, dim3(j.n), dim3(64), 0, s, j);
}

} // namespace np2
