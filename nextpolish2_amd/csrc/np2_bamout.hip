// A resident, coordinate-sorted SAM -> the bytes of a BAM and the entries of its .bai, on the device (include/np2_io.h has the
// rule; the per-record arithmetic is np2_bamout_core.hpp, which the host twin runs too).
//
//   k_bam_sizes   a lane per record: the record's bytes in the stream, its reference span (a walk over its CIGAR words), its
//                 bin and last window, and the refusals (atomicMin of the record's ordinal).  A scan of the sizes gives off[].
//   k_bam_emit    one range of the stream.  The value of every byte of a record is a function of its index in the record
//                 (np2bam::rec_byte), so a record cut by a block's or a batch's edge needs no path of its own: a wavefront
//                 takes a record that intersects the range (the first one by binary search on off[]) and its lanes write the
//                 4-byte words of the destination that lie inside both, one word a lane a step; the words cut by the record's
//                 or the range's edge go out byte by byte.  The run of 0xFF bytes of a lean record, two thirds of it, costs no
//                 load; packed SEQ, the quality bytes and the optional fields of a full record (NP2_SAM_KEEP_ALL: they lie in
//                 the record's tail) are loaded as aligned words and shifted into place.
//   k_bai_voff    after the blocks' compressed sizes were scanned into file offsets: the two virtual offsets of a record, and
//                 whether it opens a run of records of one (tid, bin)
//   k_bai_chunks  a run's key, first beg and last end; rocPRIM's stable sort orders the runs by key afterwards
//   k_bai_linear  records are in file order, beg ascends with them: atomicMin of beg over the windows a record overlaps
//                 leaves each window the first record that overlaps it.
// Plain vector stores throughout; integer atomics on the refusals, the per-reference window counts and the windows.
#include "np2_bamout.hpp"
#include "np2_sam.hpp"
#include "np2_samtail_core.hpp"

namespace np2 {

namespace {
using np2bam::Rec;
constexpr uint32_t BLOCK = 256;

__device__ __forceinline__ Rec load_rec(const BamSrc &src, const uint32_t *__restrict__ be, uint64_t i) {
    const uint32_t *w = src.recs + i * SAM_REC_WORDS;
    const uint64_t nr = src.name_ref[i];
    Rec r;
    r.tid = src.tids[i], r.pos = (int32_t)w[0];
    r.flag = w[1] & 0xFFFFu, r.mapq = (w[1] >> 16) & 0xFFu, r.n_cigar = w[2], r.l_seq = w[6];
    r.name_len = np2bam::name_len(nr), r.bin = be ? be[i] & 0xFFFFu : 0u;
    r.name = src.names + np2bam::name_off(nr);
    r.cigar = src.cigar + ((uint64_t)w[4] | (uint64_t)w[5] << 32);
    r.seq = src.seq4 + ((uint64_t)w[8] | (uint64_t)w[9] << 32);
    r.tail = nullptr, r.has_qual = 0u, r.aux_len = 0u;
    if (src.tails) { // the full stream (uniform across the launch)
        const uint64_t tr = src.tail_ref[i];
        r.tail = src.tails + np2tail::tail_off(tr), r.has_qual = np2tail::tail_has_qual(tr) ? 1u : 0u;
        r.aux_len = *reinterpret_cast<const uint32_t *>(r.tail + 12); // (a tail begins at a word)
    }
    return r;
}

// The four bytes at p, from the two aligned words that hold them, combined by a byte shift: adjacent lanes then share every
// word they load, where four byte loads would each be a request of their own.  The word behind p's is read whole even when
// p is aligned: the SEQ bytes and the tails have 16 bytes of room behind their last byte.
__device__ __forceinline__ uint32_t load_bytes4(const uint8_t *p) {
    const uint32_t *a = reinterpret_cast<const uint32_t *>((uintptr_t)p & ~(uintptr_t)3);
    const uint32_t sh = 8u * (uint32_t)((uintptr_t)p & 3u);
    return (uint32_t)(((uint64_t)a[1] << 32 | a[0]) >> sh);
}

__global__ __launch_bounds__(BLOCK) void k_bam_sizes(BamSrc src, uint32_t *__restrict__ sz, uint32_t *__restrict__ be,
                                                      np2bam::Refusals *__restrict__ ref, uint32_t *__restrict__ n_intv) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i == src.n) sz[i] = 0u; // the scan's closing entry
    if (i >= src.n) return;
    const Rec r = load_rec(src, nullptr, i);
    uint32_t bytes = 0, packed = 0;
    if (r.n_cigar > np2bam::CIGAR_MAX) {
        atomicMin(&ref->big_cigar, i);
    } else if (r.pos < 0) {
        atomicMin(&ref->neg_pos, i);
    } else {
        const uint64_t span = np2bam::cigar_span(r.cigar, r.n_cigar), end = (uint64_t)r.pos + (span ? span : 1u);
        if (end > np2bam::REF_MAX) {
            atomicMin(&ref->far_end, i);
        } else {
            const uint32_t last = (uint32_t)(end - 1u) >> np2bam::WIN_SHIFT; // below 2^15
            bytes = (uint32_t)np2bam::rec_bytes(r.name_len, r.n_cigar, r.l_seq, r.aux_len); // (l_seq and aux_len are below 2^31 each)
            packed = np2bam::reg2bin((uint32_t)r.pos, (uint32_t)end) | last << 16;
            atomicMax(&n_intv[r.tid], last + 1u);
        }
    }
    sz[i] = bytes, be[i] = packed;
}

__global__ __launch_bounds__(BLOCK) void k_bam_emit(BamSrc src, const uint64_t *__restrict__ off, const uint32_t *__restrict__ be, uint64_t b0,
                                                     uint64_t b1, uint8_t *__restrict__ dst) {
    const uint32_t wave = (blockIdx.x * BLOCK + threadIdx.x) >> 6, lane = threadIdx.x & 63u, n_waves = gridDim.x * (BLOCK / 64u);
    // the record that holds byte b0: the largest i with off[i] <= b0 (off[0] = 0, b0 < off[n])
    uint32_t lo = 0, hi = src.n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (off[mid] <= b0) lo = mid;
        else hi = mid;
    }
    for (uint64_t i = (uint64_t)lo + wave; i < src.n; i += n_waves) { // (uniform across the wavefront)
        const uint64_t o = off[i];
        if (o >= b1) break;
        const Rec r = load_rec(src, be, i);
        const uint64_t a = o > b0 ? o : b0, e = off[i + 1], b = e < b1 ? e : b1;
        uint8_t *p = dst + (a - b0), *q = dst + (b - b0); // the record's bytes [a - o, b - o) go to [p, q), inside dst[0, b1 - b0)
        const int64_t idx_p = (int64_t)(a - o);
        // the regions with a word path: packed SEQ without the masked last byte of an odd read, the quality bytes (or the run of
        // 0xFF), the optional fields.  With qualities the last two lie next to each other in the tail, as they do in the record.
        const int64_t seq = (int64_t)np2bam::seq_begin(r), qual = (int64_t)np2bam::qual_begin(r), seq_end = qual - (int64_t)(r.l_seq & 1u);
        const int64_t aux = qual + (int64_t)r.l_seq;
        uint8_t *w0 = p - ((uintptr_t)p & 3u);
        for (uint8_t *w = w0 + 4u * lane; w < q; w += 256u) {
            const int64_t idx = idx_p + (w - p); // the record's byte at w; negative only for bytes in front of p
            if (w >= p && w + 4 <= q) { // (the four bytes are inside the record: idx + 4 <= its size)
                uint32_t x;
                if (idx >= seq && idx + 4 <= seq_end) x = load_bytes4(r.seq + (idx - seq));
                else if (idx >= qual && r.has_qual) x = load_bytes4(r.tail + np2bam::TAIL_HEAD + (idx - qual));
                else if (idx >= qual && idx + 4 <= aux) x = 0xFFFFFFFFu;
                else if (idx >= aux) x = load_bytes4(r.tail + np2bam::TAIL_HEAD + (idx - aux));
                else
                    x = (uint32_t)np2bam::rec_byte(r, (uint64_t)idx) | (uint32_t)np2bam::rec_byte(r, (uint64_t)idx + 1u) << 8 |
                        (uint32_t)np2bam::rec_byte(r, (uint64_t)idx + 2u) << 16 | (uint32_t)np2bam::rec_byte(r, (uint64_t)idx + 3u) << 24;
                *reinterpret_cast<uint32_t *>(w) = x;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (w + k >= p && w + k < q) w[k] = np2bam::rec_byte(r, (uint64_t)(idx + k));
            }
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_bai_voff(BamSrc src, const uint64_t *__restrict__ off, const uint32_t *__restrict__ be, uint64_t hdr,
                                                     const uint64_t *__restrict__ C, uint64_t *__restrict__ beg, uint64_t *__restrict__ end,
                                                     uint32_t *__restrict__ head) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i == src.n) head[i] = 0u; // the scan's closing entry
    if (i >= src.n) return;
    beg[i] = np2bam::voff(C, hdr + off[i]), end[i] = np2bam::voff(C, hdr + off[i + 1]);
    head[i] = i == 0u || src.tids[i] != src.tids[i - 1] || (be[i] & 0xFFFFu) != (be[i - 1] & 0xFFFFu) ? 1u : 0u;
}

__global__ __launch_bounds__(BLOCK) void k_bai_chunks(BamSrc src, const uint32_t *__restrict__ be, const uint64_t *__restrict__ beg,
                                                       const uint64_t *__restrict__ end, const uint32_t *__restrict__ head,
                                                       const uint32_t *__restrict__ run, uint64_t *__restrict__ key, uint64_t *__restrict__ rbeg,
                                                       uint64_t *__restrict__ rend, uint32_t *__restrict__ val) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= src.n) return;
    const uint32_t r = run[i] + head[i] - 1u; // the run record i is in (head[0] = 1)
    if (head[i]) key[r] = (uint64_t)(uint32_t)src.tids[i] << 32 | (be[i] & 0xFFFFu), rbeg[r] = beg[i], val[r] = r;
    if (head[i + 1] || i + 1u == src.n) rend[r] = end[i];
}

__global__ __launch_bounds__(BLOCK) void k_bai_linear(BamSrc src, const uint32_t *__restrict__ be, const uint64_t *__restrict__ beg,
                                                       const uint32_t *__restrict__ win_off, unsigned long long *__restrict__ win) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= src.n) return;
    const uint32_t first = (uint32_t)src.recs[(uint64_t)i * SAM_REC_WORDS] >> np2bam::WIN_SHIFT, last = be[i] >> 16; // last < n_intv[tid]
    unsigned long long *w = win + win_off[src.tids[i]];
    for (uint32_t k = first; k <= last; ++k) atomicMin(w + k, (unsigned long long)beg[i]);
}

inline dim3 lane_grid(uint64_t lanes) { return dim3((uint32_t)((lanes + BLOCK - 1) / BLOCK)); }

} // namespace

void launch_bam_sizes(hipStream_t s, BamSrc src, uint32_t *sz, uint32_t *be, np2bam::Refusals *ref, uint32_t *n_intv) {
    hipLaunchKernelGGL(k_bam_sizes, lane_grid((uint64_t)src.n + 1), dim3(BLOCK), 0, s, src, sz, be, ref, n_intv);
}
void launch_bam_emit(hipStream_t s, BamSrc src, const uint64_t *off, const uint32_t *be, uint64_t b0, uint64_t b1, uint8_t *dst, uint32_t n_blocks) {
    if (src.n && b1 > b0) hipLaunchKernelGGL(k_bam_emit, dim3(n_blocks ? n_blocks : 1u), dim3(BLOCK), 0, s, src, off, be, b0, b1, dst);
}
void launch_bai_voff(hipStream_t s, BamSrc src, const uint64_t *off, const uint32_t *be, uint64_t hdr, const uint64_t *C, uint64_t *beg,
                     uint64_t *end, uint32_t *head) {
    hipLaunchKernelGGL(k_bai_voff, lane_grid((uint64_t)src.n + 1), dim3(BLOCK), 0, s, src, off, be, hdr, C, beg, end, head);
}
void launch_bai_chunks(hipStream_t s, BamSrc src, const uint32_t *be, const uint64_t *beg, const uint64_t *end, const uint32_t *head,
                       const uint32_t *run, uint64_t *key, uint64_t *rbeg, uint64_t *rend, uint32_t *val) {
    if (src.n) hipLaunchKernelGGL(k_bai_chunks, lane_grid(src.n), dim3(BLOCK), 0, s, src, be, beg, end, head, run, key, rbeg, rend, val);
}
void launch_bai_linear(hipStream_t s, BamSrc src, const uint32_t *be, const uint64_t *beg, const uint32_t *win_off, unsigned long long *win) {
    if (src.n) hipLaunchKernelGGL(k_bai_linear, lane_grid(src.n), dim3(BLOCK), 0, s, src, be, beg, win_off, win);
}

} // namespace np2
