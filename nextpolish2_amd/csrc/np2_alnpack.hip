// The aligner's records packed where they lie (include/np2_io.h: np2_sam_from_reads; the arithmetic: np2_alnpack_core.hpp).
// k_align_ops_emit has just left a sub-group's records and final CIGAR words in device memory, next to the batch's read bytes:
//   k_alnpack_sizes  a lane per read: kept, CIGAR words, packed SEQ bytes, name bytes, for the scans that place them
//   k_alnpack        a wavefront per kept read: the record (ten words, one a lane), tid and key, the CIGAR words, the name, and
//                    the SEQ: a record starts at a byte, so up to three head bytes reach the next 4-byte boundary of the
//                    destination a lane each, then every lane turns eight bases (two aligned 8-byte loads and a funnel shift;
//                    the reverse strand takes them from the read's far end, complemented) into one 32-bit store, and up to four
//                    tail bytes (an odd read's last among them) go out a lane each.
#include "np2_alnpack.hpp"

namespace np2 {

namespace {
constexpr uint32_t BLOCK = 256;

__device__ __forceinline__ void read_of(const AlnPackJob &j, uint32_t i, uint32_t *from, uint32_t *len) {
    const uint32_t rd = j.r0 + i;
    *from = rd ? j.rd_ends[rd - 1] + 1u : 0u;
    *len = j.rd_ends[rd] - *from;
}
} // namespace

__global__ __launch_bounds__(BLOCK) void k_alnpack_sizes(AlnPackJob j, uint32_t *__restrict__ first_bad) {
    const uint32_t i = j.g0 + blockIdx.x * BLOCK + threadIdx.x;
    if (i > j.g1) return;
    uint32_t k = 0, nc = 0, ns = 0, nn = 0;
    if (i < j.g1) {
        const np2aln::Rec r = j.recs[i];
        if (np2pack::kept(r)) {
            uint32_t from, len;
            read_of(j, i, &from, &len);
            k = 1u, nc = r.n_cigar, ns = (len + 1u) / 2u;
            if (j.name_at) {
                nn = j.name_at[j.r0 + i + 1u] - j.name_at[j.r0 + i] - 1u; // (a '\n' ends each name)
                if (nn == 0u || nn > 254u) atomicMin(first_bad, j.r0 + i), nn = 0u;
            }
        }
    }
    const uint32_t at = i - j.g0; // (entry g1 - g0 closes the scans)
    j.kept[at] = k, j.n_cig[at] = nc, j.n_seq[at] = ns;
    if (j.name_at) j.n_name[at] = nn;
}

__global__ __launch_bounds__(BLOCK) void k_alnpack(AlnPackJob j, AlnPackOut o) {
    const uint32_t at = (blockIdx.x * BLOCK + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    const uint32_t i = j.g0 + at;
    if (i >= j.g1) return; // (uniform across the wavefront, as is the next one)
    const np2aln::Rec r = j.recs[i];
    if (!np2pack::kept(r)) return;
    uint32_t from, len;
    read_of(j, i, &from, &len);
    const uint8_t *q = j.rd_seq + from;
    const bool rev = (r.flag & 16u) != 0;
    const uint64_t k = o.rec_base + j.kept_off[at], co = o.cig_base + j.cig_off[at], so = o.seq_base + j.seq_off[at];
    if (lane < np2pack::REC_WORDS) o.recs[k * np2pack::REC_WORDS + lane] = np2pack::rec_word(r, len, co, so, lane);
    if (lane == 0) {
        o.tids[k] = r.tid;
        o.keys[k] = np2pack::rec_key(r, o.tie_by_strand);
    }
    const uint32_t *b = j.b + 2u * (uint64_t)j.ooff[i] + 2u * (uint64_t)at;
    for (uint32_t c = lane; c < r.n_cigar; c += 64u) o.cigar[co + c] = b[c];
    if (j.name_at) {
        const uint32_t n = j.name_off[at + 1u] - j.name_off[at]; // (1 .. 254: the host refuses the call otherwise)
        const uint64_t to = o.name_base + j.name_off[at];
        const uint8_t *nm = j.names_in + j.name_at[j.r0 + i];
        for (uint32_t c = lane; c < n; c += 64u) o.names[to + c] = nm[c];
        if (lane == 0) o.name_ref[k] = to << 8 | n;
    }
    // SEQ: n_bytes packed bytes from seq4 + so on
    const uint32_t n_bytes = (len + 1u) / 2u, full = len / 2u; // full: the bytes with both columns inside the read
    uint32_t head = (4u - (uint32_t)(so & 3u)) & 3u;
    head = head < n_bytes ? head : n_bytes;
    uint8_t *dst = o.seq4 + so;
    if (lane < head) dst[lane] = np2pack::seq4_byte(q, len, rev, lane);
    const uint32_t n_words = full > head ? (full - head) / 4u : 0u;
    uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head); // (so + head is a multiple of 4 wherever words are written)
    for (uint32_t w = lane; w < n_words; w += 64u) dw[w] = np2pack::seq4_word(q, len, rev, head + 4u * w);
    const uint32_t done = head + 4u * n_words; // at most three whole bytes and an odd read's last one remain
    if (done + lane < n_bytes) dst[done + lane] = np2pack::seq4_byte(q, len, rev, done + lane);
}

void launch_alnpack_sizes(hipStream_t s, const AlnPackJob &j, uint32_t *first_bad) {
    hipLaunchKernelGGL(k_alnpack_sizes, dim3((j.g1 - j.g0 + 1u + BLOCK - 1u) / BLOCK), dim3(BLOCK), 0, s, j, first_bad);
}
void launch_alnpack(hipStream_t s, const AlnPackJob &j, const AlnPackOut &o) {
    if (j.g1 <= j.g0) return;
    hipLaunchKernelGGL(k_alnpack, dim3((uint32_t)(((uint64_t)(j.g1 - j.g0) * 64u + BLOCK - 1u) / BLOCK)), dim3(BLOCK), 0, s, j, o);
}

} // namespace np2
