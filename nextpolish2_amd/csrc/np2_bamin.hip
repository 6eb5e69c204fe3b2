// An inflated, unindexed BAM stream -> the resident arrays of the SAM handle (include/np2_io.h: "BAM input"; the per-record rule
// is np2_bamin_core.hpp).  A piece is whole BGZF blocks inflated behind the bytes of a record the piece before did not finish:
//
//   k_bamin_walk    one lane follows the chain of block_size words: a record's length says where the next begins, so the walk
//                   is exact and serial; 4 bytes read per record.  It lists the record starts and says where an unfinished
//                   record begins.
//   k_bamin_fields  a wavefront per record: every lane reads the fixed fields (one address: a broadcast), the lanes stride
//                   over the CIGAR words and the quality bytes, lane 0 walks the types of the optional fields.  Sizes for the scans.
//   k_bamin_pack    after the scans placed the kept records: a wavefront per kept record writes the record, tid and sort key,
//                   the CIGAR words, and copies name, SEQ, quality bytes and optional fields.  The copies store whole words at
//                   the destination's alignment; a word comes from the two aligned source words it straddles.  These streams
//                   are nearly all of the input.
// Plain vector stores throughout; one integer atomicMin per refused record.
#include "np2_bamin.hpp"

namespace np2 {

namespace {
namespace bi = np2bamin;

__device__ __forceinline__ uint32_t wave_add(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor(v, o);
    return v;
}

// n bytes src -> dst by one wavefront.  Up to 3 bytes bring dst to a word; then words, each made of the aligned source words
// it straddles (the load may reach 7 bytes behind src + n: inside BAMIN_PAD; before src the stream holds the record's own
// fixed fields); then up to 3 bytes.
__device__ __forceinline__ void wave_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t n, uint32_t lane) {
    uint32_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
    head = head < n ? head : n;
    if (lane < head) dst[lane] = src[lane];
    dst += head, src += head, n -= head;
    const uint32_t n_w = n >> 2, mis = (uint32_t)((uintptr_t)src & 3u), sh = 8u * mis;
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(src - mis);
    uint32_t *dw = reinterpret_cast<uint32_t *>(dst);
    for (uint32_t j = lane; j < n_w; j += 64u) {
        const uint32_t lo = sw[j];
        dw[j] = mis ? lo >> sh | sw[j + 1] << (32u - sh) : lo;
    }
    if (lane < (n & 3u)) dst[4u * n_w + lane] = src[4u * n_w + lane];
}

__global__ __launch_bounds__(64) void k_bamin_walk(const uint8_t *__restrict__ stream, uint32_t start, uint32_t n, uint32_t limit,
                                                   uint32_t *__restrict__ starts, BaminCtr *__restrict__ ctr) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t at = start < n ? start : n, cnt = 0, flags = 0;
    while (n - at >= 4u) { // every listed start is at least 36 bytes behind the one before: cnt stays below n / 36 + 2
        const uint32_t bs = bi::rd32(stream + at);
        if (bs < bi::FIXED || bs > limit - 4u) { // (limit is at least 36)
            starts[cnt++] = at;
            flags = bs < bi::FIXED ? BAMIN_WALK_SHORT : BAMIN_WALK_PIECE;
            break;
        }
        if (bs + 4u > n - at) break;
        starts[cnt++] = at;
        at += bs + 4u;
    }
    ctr->count = cnt, ctr->flags = flags, ctr->tail_at = at;
}

__global__ __launch_bounds__(SAM_BLOCK) void k_bamin_fields(const uint8_t *__restrict__ stream, const uint32_t *__restrict__ starts, uint32_t n_recs,
                                                             uint32_t walk_flags, uint32_t n_ref, uint32_t flags, uint32_t *__restrict__ info,
                                                             uint32_t *__restrict__ kept, uint32_t *__restrict__ n_cig, uint32_t *__restrict__ n_seq,
                                                             uint32_t *__restrict__ n_name, uint32_t *__restrict__ t_size, BaminCtr *__restrict__ ctr) {
    const uint32_t r = (blockIdx.x * SAM_BLOCK + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    const bool names = (flags & (bi::KEEP_NAMES | bi::KEEP_ALL)) != 0u, all = (flags & bi::KEEP_ALL) != 0u;
    if (r == n_recs && lane == 0) { // the scans' closing entries
        kept[r] = n_cig[r] = n_seq[r] = 0u;
        if (names) n_name[r] = 0u;
        if (all) t_size[r] = 0u;
    }
    if (r >= n_recs) return; // (uniform across the wavefront, as is all below)
    const uint8_t *p = stream + starts[r];
    bi::Rec rc;
    rc.kept = false, rc.n_cigar = rc.l_seq = rc.l_name = rc.aux_len = 0;
    bool hq = false;
    uint32_t w;
    if (r == n_recs - 1u && walk_flags) { // only its block_size word is known to be there
        w = walk_flags & BAMIN_WALK_SHORT ? bi::W_SHORT : bi::W_PIECE;
    } else {
        w = bi::fixed(p, n_ref, flags, &rc);
        if (bi::structural(w)) rc.kept = false;
        if (rc.kept) {
            bool bad = false;
            for (uint32_t j = lane; j < rc.n_cigar; j += 64u) bad = bad || !bi::cigar_word_ok(bi::rd32(p + rc.cig_at + 4u * j));
            if (__ballot(bad)) w = bi::first(w, bi::W_CIGAR);
            if (all) {
                uint32_t n_ff = 0, n_high = 0;
                for (uint32_t j = lane; j < rc.l_seq; j += 64u) {
                    const uint8_t q = p[rc.qual_at + j];
                    n_ff += q == 0xFFu ? 1u : 0u, n_high += q != 0xFFu && q > 93u ? 1u : 0u;
                }
                w = bi::first(w, bi::qual_kind(rc.l_seq, wave_add(n_ff), wave_add(n_high), &hq));
                uint32_t ok = 1u;
                if (lane == 0) ok = bi::aux_ok(p + rc.aux_at, rc.aux_len) ? 1u : 0u;
                if (!__shfl(ok, 0)) w = bi::first(w, bi::W_AUX);
            }
        }
    }
    if (lane == 0) {
        const bool k = w == bi::W_OK && rc.kept;
        info[r] = w | (k ? BAMIN_KEPT : 0u) | (k && hq ? BAMIN_HAS_QUAL : 0u);
        kept[r] = k ? 1u : 0u, n_cig[r] = k ? rc.n_cigar : 0u, n_seq[r] = k ? bi::seq_bytes(rc) : 0u;
        if (names) n_name[r] = k ? rc.l_name - 1u : 0u;
        if (all) t_size[r] = k ? np2tail::pad4(bi::tail_size(rc, hq)) : 0u;
        if (w != bi::W_OK) atomicMin(&ctr->first_err, r);
    }
}

__global__ __launch_bounds__(SAM_BLOCK) void k_bamin_pack(const uint8_t *__restrict__ stream, const uint32_t *__restrict__ starts,
                                                           const uint32_t *__restrict__ info, uint32_t n_recs, uint32_t n_ref, uint32_t flags,
                                                           uint32_t tie_by_strand, BaminOut o) {
    const uint32_t r = (blockIdx.x * SAM_BLOCK + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (r >= n_recs) return; // (uniform across the wavefront, as is the next one)
    const uint32_t inf = info[r];
    if (!(inf & BAMIN_KEPT)) return;
    const uint8_t *p = stream + starts[r];
    bi::Rec rc;
    (void)bi::fixed(p, n_ref, flags, &rc); // (k_bamin_fields found it good)
    const uint64_t k = o.rec_base + o.kept_off[r], co = o.cig_base + o.cig_off[r], so = o.seq_base + o.seq_off[r];
    if (lane < SAM_REC_WORDS) o.recs[k * SAM_REC_WORDS + lane] = bi::rec_word(rc, co, so, lane);
    if (lane == 0) {
        o.tids[k] = rc.tid;
        o.keys[k] = np2sam::sort_key(rc.tid, rc.pos, rc.flag, tie_by_strand);
    }
    for (uint32_t j = lane; j < rc.n_cigar; j += 64u) o.cigar[co + j] = bi::rd32(p + rc.cig_at + 4u * j);
    const uint32_t n_sb = bi::seq_bytes(rc), odd = rc.l_seq & 1u;
    wave_copy(o.seq4 + so, p + rc.seq_at, n_sb - odd, lane);
    if (odd && lane == 0) o.seq4[so + n_sb - 1u] = bi::seq_byte(p, rc, n_sb - 1u);
    if (flags & (bi::KEEP_NAMES | bi::KEEP_ALL)) {
        const uint64_t to = o.name_base + o.name_off[r];
        const uint32_t len = rc.l_name - 1u;
        for (uint32_t j = lane; j < len; j += 64u) o.names[to + j] = p[36u + j];
        if (lane == 0) o.name_ref[k] = to << 8 | len;
    }
    if (flags & bi::KEEP_ALL) {
        const bool hq = (inf & BAMIN_HAS_QUAL) != 0u;
        const uint64_t to = o.tail_base + o.tail_off[r]; // a multiple of 4
        uint8_t *t = o.tails + to;
        const uint32_t n_q = hq ? rc.l_seq : 0u, size = bi::tail_size(rc, hq);
        if (lane < 4u) {
            const uint32_t v = lane == 0 ? (uint32_t)rc.next_tid : lane == 1 ? (uint32_t)rc.next_pos : lane == 2 ? (uint32_t)rc.tlen : rc.aux_len;
            reinterpret_cast<uint32_t *>(t)[lane] = v;
        }
        wave_copy(t + np2tail::HEAD_BYTES, p + rc.qual_at, n_q, lane);
        wave_copy(t + np2tail::HEAD_BYTES + n_q, p + rc.aux_at, rc.aux_len, lane);
        if (lane < np2tail::pad4(size) - size) t[size + lane] = 0;
        if (lane == 0) o.tail_ref[k] = np2tail::tail_ref(to, hq);
    }
}

inline dim3 wave_grid(uint64_t waves) { return dim3((uint32_t)((waves * 64u + SAM_BLOCK - 1) / SAM_BLOCK)); }

} // namespace

void launch_bamin_walk(hipStream_t s, const uint8_t *stream, uint32_t start, uint32_t n, uint32_t limit, uint32_t *starts, BaminCtr *ctr) {
    hipLaunchKernelGGL(k_bamin_walk, dim3(1), dim3(64), 0, s, stream, start, n, limit < 36u ? 36u : limit, starts, ctr);
}
void launch_bamin_fields(hipStream_t s, const uint8_t *stream, const uint32_t *starts, uint32_t n_recs, uint32_t walk_flags, uint32_t n_ref,
                         uint32_t flags, uint32_t *info, uint32_t *kept, uint32_t *n_cig, uint32_t *n_seq, uint32_t *n_name, uint32_t *t_size,
                         BaminCtr *ctr) {
    hipLaunchKernelGGL(k_bamin_fields, wave_grid((uint64_t)n_recs + 1), dim3(SAM_BLOCK), 0, s, stream, starts, n_recs, walk_flags, n_ref, flags, info,
                       kept, n_cig, n_seq, n_name, t_size, ctr);
}
void launch_bamin_pack(hipStream_t s, const uint8_t *stream, const uint32_t *starts, const uint32_t *info, uint32_t n_recs, uint32_t n_ref,
                       uint32_t flags, uint32_t tie_by_strand, const BaminOut &out) {
    if (n_recs)
        hipLaunchKernelGGL(k_bamin_pack, wave_grid(n_recs), dim3(SAM_BLOCK), 0, s, stream, starts, info, n_recs, n_ref, flags, tie_by_strand, out);
}

} // namespace np2
