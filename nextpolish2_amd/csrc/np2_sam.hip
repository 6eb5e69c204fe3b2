// SAM text -> alignment records, CIGAR words and packed SEQ on the device (include/np2_io.h: np2_sam_*; the per-lane rule is
// np2_sam_core.hpp).  A piece of the text ends at a line boundary and is gone after three kernels:
//
//   k_sam_lines   16 text bytes a lane: the '\n' bytes are counted, the block scan and the decoupled look-back
//                 (np2_blockscan.hpp, np2_lookback.hpp) give the first one its ordinal, the offsets go out in order.
//                 1 byte read per byte of text.
//   k_sam_fields  a wavefront per line: 256 bytes a step, a ballot per 64 finds the first ten tabs; lanes 0 - 3 read FLAG,
//                 RNAME (through the @SQ name table), POS and MAPQ; the lanes stride over the CIGAR field, judge every byte
//                 and count the operation letters.  The optional fields and QUAL are not read: the walk ends at the tenth tab.
//   k_sam_pack    after the scans placed the kept records: a wavefront per kept line writes the record (ten words, one a
//                 lane), the CIGAR words (a lane that owns an operation letter reads the digits in front of it; its rank among
//                 the letters comes from the ballot) and the SEQ nibbles (two bases a lane a step, byte stores next to each other).
//
// With NP2_SAM_KEEP_NAMES (np2_sam_open_ex; the BAM writer, np2_bamout.hip, needs the QNAMEs) two more per piece:
//   k_sam_name_len   a wavefront per line: a kept line's first tab among its first 256 bytes, by ballot; an empty name or one
//                    above 254 bytes is the piece's first bad line by atomicMin
//   k_sam_name_copy  after the scan placed the names: the bytes, and offset << 8 | length per record
// and k_sam_gather_u64 moves those words into sorted order; the name bytes stay where they are, as SEQ does.
//
// With NP2_SAM_KEEP_ALL (the full BAM: QUAL, the mate fields and the optional fields) two more per piece, a wavefront per line:
//   k_sam_tail_len   lanes 0 - 2 read RNEXT, PNEXT and TLEN; the lanes stride over QUAL, find its end and judge its bytes; the
//                    tabs behind it are found by ballot, 64 a pass, and every lane takes one optional field TAG:TYPE:VALUE: its
//                    binary size and whether it is well formed (np2_samtail_core.hpp).  The size of a Z or H value comes from
//                    the tab positions; one of more than 64 bytes is judged by the whole wavefront.  The sizes are summed.
//   k_sam_tail_emit  after the scan placed the tails: the three mate words and aux_len, the quality bytes minus 33 (all lanes),
//                    the optional fields at the offsets of a wave prefix sum of their sizes, one field a lane, a long Z or H
//                    value by all lanes; and offset << 1 | has_qual per record, which k_sam_gather_u64 moves as it moves name_ref.
//
// After the last piece the keys are sorted with the record ordinals as values (rocPRIM, np2_prims.hip: stable) and
//   k_sam_gather  a wavefront per record moves the record and its CIGAR words into sorted order; SEQ bytes stay where they are.
// Plain vector stores throughout; integer atomics only on the piece's three counters.
#include "np2_sam.hpp"
#include "np2_blockscan.hpp"

namespace np2 {

namespace {
using np2sam::Line;
using np2sam::NameTab;

__device__ __forceinline__ uint64_t lanes_below() { return (1ull << (threadIdx.x & 63u)) - 1ull; }

__global__ __launch_bounds__(SAM_BLOCK) void k_sam_lines(Lookback lb, const uint8_t *__restrict__ text, uint32_t n,
                                                          uint32_t *__restrict__ line_end, SamCtr *__restrict__ ctr) {
    __shared__ uint32_t sh[16];
    const uint32_t bid = lb_block_id(lb, sh);
    const uint32_t i0 = bid * SAM_TILE + threadIdx.x * SAM_STRETCH;
    uint32_t nl = 0; // bit k: text[i0 + k] is a '\n' of the piece
    if (i0 < n) {    // (the 16 bytes lie inside n + SAM_TEXT_PAD)
        const uint4 q = *reinterpret_cast<const uint4 *>(text + i0);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (uint32_t k = 0; k < SAM_STRETCH; ++k)
            if (((w[k >> 2] >> (8u * (k & 3u))) & 255u) == (uint32_t)'\n' && i0 + k < n) nl |= 1u << k;
    }
    uint32_t total, pre, unused;
    uint32_t rank = block_excl_scan<OpAdd, SAM_BLOCK / 64>((uint32_t)__builtin_popcount(nl), sh, total);
    lb_exclusive2(lb, bid, total, 0u, sh, &ctr->err, pre, unused);
    rank += pre; // lines that end before i0: at most n of them, and line_end has room for n
    while (nl) {
        line_end[rank++] = i0 + (uint32_t)__builtin_ctz(nl);
        nl &= nl - 1u;
    }
    if (bid == lb.n_blocks - 1 && threadIdx.x == 0) ctr->n_lines = pre + total;
}

__global__ __launch_bounds__(SAM_BLOCK) void k_sam_fields(const uint8_t *__restrict__ text, const uint32_t *__restrict__ line_end,
                                                           uint32_t n_lines, NameTab nt, Line *__restrict__ lines, uint32_t *__restrict__ kept,
                                                           uint32_t *__restrict__ n_cig, uint32_t *__restrict__ n_seq, SamCtr *__restrict__ ctr) {
    const uint32_t r = (blockIdx.x * SAM_BLOCK + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (r == n_lines && lane == 0) kept[r] = n_cig[r] = n_seq[r] = 0u; // the scans' closing entries
    if (r >= n_lines) return;                                          // (uniform across the wavefront)
    const uint32_t s = r ? line_end[r - 1] + 1u : 0u;
    uint32_t e = line_end[r];
    if (e > s && text[e - 1] == (uint8_t)'\r') --e;
    Line ln;
    ln.cig_a = ln.cig_b = ln.seq_a = ln.l_seq = 0, ln.tid = np2sam::TID_NONE, ln.pos = -1, ln.n_cigar = 0, ln.flag = 0, ln.mapq = 0, ln.err = np2sam::OK;
    if (e == s) {
        ln.tid = np2sam::TID_EMPTY_LINE;
    } else if (text[s] == (uint8_t)'@') {
        ln.err = np2sam::E_HEADER_LATE;
    } else {
        // lane k keeps the offset of tab k
        uint32_t n_tab = 0, my_tab = 0;
        for (uint32_t c = s; c < e && n_tab < np2sam::N_TABS; c += 256u) {
            uint8_t b[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) b[u] = c + 64u * u + lane < e ? text[c + 64u * u + lane] : (uint8_t)0;
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) {
                uint64_t m = __ballot(b[u] == (uint8_t)'\t');
                while (m && n_tab < np2sam::N_TABS) {
                    if (lane == n_tab) my_tab = c + 64u * u + (uint32_t)__builtin_ctzll(m);
                    ++n_tab;
                    m &= m - 1ull;
                }
            }
        }
        if (n_tab < np2sam::N_TABS) {
            ln.err = np2sam::E_FIELDS;
        } else {
            const uint32_t t0 = __shfl(my_tab, 0), t1 = __shfl(my_tab, 1), t2 = __shfl(my_tab, 2), t3 = __shfl(my_tab, 3),
                           t4 = __shfl(my_tab, 4), t5 = __shfl(my_tab, 5), t8 = __shfl(my_tab, 8), t9 = __shfl(my_tab, 9);
            uint32_t val = 0, err = np2sam::OK; // lane 0: FLAG, 1: tid, 2: pos, 3: MAPQ
            if (lane == 0) err = np2sam::parse_flag(text, t0 + 1u, t1, &val);
            if (lane == 1) {
                int32_t tid = 0;
                err = np2sam::parse_rname(nt, text, t1 + 1u, t2, &tid);
                val = (uint32_t)tid;
            }
            if (lane == 2) {
                int32_t pos = 0;
                err = np2sam::parse_pos(text, t2 + 1u, t3, &pos);
                val = (uint32_t)pos;
            }
            if (lane == 3) err = np2sam::parse_mapq(text, t3 + 1u, t4, &val);
            ln.flag = (uint16_t)__shfl(val, 0), ln.tid = (int32_t)__shfl(val, 1), ln.pos = (int32_t)__shfl(val, 2), ln.mapq = (uint8_t)__shfl(val, 3);
            ln.cig_a = t4 + 1u, ln.cig_b = t5;
            uint32_t cnt = 0;
            if (ln.cig_b == ln.cig_a) {
                if (lane == 4) err = np2sam::E_CIGAR;
            } else if (!(ln.cig_b - ln.cig_a == 1u && text[ln.cig_a] == (uint8_t)'*')) {
                for (uint32_t i = ln.cig_a + lane; i < ln.cig_b; i += 64u) {
                    uint32_t w;
                    const uint32_t k = np2sam::cigar_byte(text, ln.cig_a, ln.cig_b, i, &w);
                    if (k == 2u) err = np2sam::first_err(err, np2sam::E_CIGAR);
                    cnt += k == 1u ? 1u : 0u;
                }
            }
            for (int o = 32; o > 0; o >>= 1) {
                cnt += __shfl_xor(cnt, o);
                err = np2sam::first_err(err, (uint32_t)__shfl_xor(err, o));
            }
            ln.n_cigar = cnt, ln.err = (uint8_t)err;
            ln.seq_a = t8 + 1u;
            ln.l_seq = t9 - ln.seq_a == 1u && text[ln.seq_a] == (uint8_t)'*' ? 0u : t9 - ln.seq_a;
        }
    }
    if (lane == 0) {
        const bool k = np2sam::line_kept(ln);
        lines[r] = ln;
        kept[r] = k ? 1u : 0u, n_cig[r] = k ? ln.n_cigar : 0u, n_seq[r] = k ? (ln.l_seq + 1u) / 2u : 0u;
        if (ln.err != np2sam::OK) atomicMin(&ctr->first_err, r);
        if (ln.tid == np2sam::TID_EMPTY_LINE) atomicAdd(&ctr->n_empty, 1u);
    }
}

__global__ __launch_bounds__(SAM_BLOCK) void k_sam_pack(const uint8_t *__restrict__ text, const Line *__restrict__ lines, uint32_t n_lines,
                                                         const uint32_t *__restrict__ kept_off, const uint32_t *__restrict__ cig_off,
                                                         const uint32_t *__restrict__ seq_off, uint64_t rec_base, uint64_t cig_base, uint64_t seq_base,
                                                         uint32_t tie_by_strand, uint32_t *__restrict__ recs, int32_t *__restrict__ tids,
                                                         uint64_t *__restrict__ keys, uint32_t *__restrict__ cigar, uint8_t *__restrict__ seq4) {
    const uint32_t r = (blockIdx.x * SAM_BLOCK + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (r >= n_lines) return; // (uniform across the wavefront, as is the next one)
    const Line ln = lines[r];
    if (!np2sam::line_kept(ln)) return;
    const uint64_t k = rec_base + kept_off[r], co = cig_base + cig_off[r], so = seq_base + seq_off[r];
    if (lane < SAM_REC_WORDS) { // np2_bamrec_t, padding included
        const uint32_t w[SAM_REC_WORDS] = {(uint32_t)ln.pos, (uint32_t)ln.flag | (uint32_t)ln.mapq << 16, ln.n_cigar, 0u,
                                           (uint32_t)co, (uint32_t)(co >> 32), ln.l_seq, 0u, (uint32_t)so, (uint32_t)(so >> 32)};
        uint32_t v = 0;
#pragma unroll
        for (uint32_t j = 0; j < SAM_REC_WORDS; ++j) v = lane == j ? w[j] : v;
        recs[k * SAM_REC_WORDS + lane] = v;
    }
    if (lane == 0) {
        tids[k] = ln.tid;
        keys[k] = np2sam::sort_key(ln.tid, ln.pos, ln.flag, tie_by_strand);
    }
    if (ln.n_cigar) { // letters before this chunk + letters of lower lanes: below n_cigar, what k_sam_fields counted
        uint32_t done = 0;
        for (uint32_t c = ln.cig_a; c < ln.cig_b; c += 64u) {
            const uint32_t i = c + lane;
            uint32_t w = 0;
            const bool is_op = i < ln.cig_b && np2sam::cigar_byte(text, ln.cig_a, ln.cig_b, i, &w) == 1u;
            const uint64_t m = __ballot(is_op);
            if (is_op) cigar[co + done + (uint32_t)__popcll(m & lanes_below())] = w;
            done += (uint32_t)__popcll(m);
        }
    }
    const uint32_t n_bytes = (ln.l_seq + 1u) / 2u;
    for (uint32_t j = lane; j < n_bytes; j += 64u) { // seq_a + 2 j + 1 < seq_a + l_seq: inside the line
        const uint32_t hi = np2sam::base_code(text[ln.seq_a + 2u * j]);
        const uint32_t lo = 2u * j + 1u < ln.l_seq ? np2sam::base_code(text[ln.seq_a + 2u * j + 1u]) : 0u;
        seq4[so + j] = (uint8_t)(hi << 4 | lo);
    }
}

__global__ __launch_bounds__(SAM_BLOCK) void k_sam_iota(uint32_t *__restrict__ vals, uint32_t n) {
    const uint32_t i = blockIdx.x * SAM_BLOCK + threadIdx.x;
    if (i < n) vals[i] = i;
}

__global__ __launch_bounds__(SAM_BLOCK) void k_sam_sorted_sizes(const uint32_t *__restrict__ recs_in, const uint32_t *__restrict__ order, uint32_t n,
                                                                 uint32_t *__restrict__ n_cig) {
    const uint32_t i = blockIdx.x * SAM_BLOCK + threadIdx.x;
    if (i < n) n_cig[i] = recs_in[(uint64_t)order[i] * SAM_REC_WORDS + 2u]; // (order holds each of 0 .. n - 1 once)
    if (i == n) n_cig[i] = 0u;
}

__global__ __launch_bounds__(SAM_BLOCK) void k_sam_gather(const uint32_t *__restrict__ recs_in, const int32_t *__restrict__ tids_in,
                                                           const uint32_t *__restrict__ cigar_in, const uint32_t *__restrict__ order,
                                                           const uint32_t *__restrict__ cig_off, uint32_t n, uint32_t *__restrict__ recs,
                                                           int32_t *__restrict__ tids, uint32_t *__restrict__ cigar) {
    const uint32_t r = (blockIdx.x * SAM_BLOCK + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (r >= n) return; // (uniform across the wavefront)
    const uint64_t src = order[r];
    const uint32_t *in = recs_in + src * SAM_REC_WORDS;
    const uint32_t n_cigar = in[2];
    const uint64_t from = (uint64_t)in[4] | (uint64_t)in[5] << 32, to = cig_off[r];
    if (lane < SAM_REC_WORDS) {
        uint32_t v = in[lane];
        if (lane == 4) v = (uint32_t)to;
        if (lane == 5) v = 0u;
        recs[(uint64_t)r * SAM_REC_WORDS + lane] = v;
    }
    if (lane == 0) tids[r] = tids_in[src];
    for (uint32_t j = lane; j < n_cigar; j += 64u) cigar[to + j] = cigar_in[from + j];
}

// The QNAME of a kept line: the bytes before its first tab, which is among the first 255 bytes or the name is too long.
__global__ __launch_bounds__(SAM_BLOCK) void k_sam_name_len(const uint8_t *__restrict__ text, const uint32_t *__restrict__ line_end,
                                                             const Line *__restrict__ lines, uint32_t n_lines, uint32_t *__restrict__ n_name,
                                                             uint32_t *__restrict__ first_bad) {
    const uint32_t r = (blockIdx.x * SAM_BLOCK + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (r == n_lines && lane == 0) n_name[r] = 0u; // the scan's closing entry
    if (r >= n_lines) return;                      // (uniform across the wavefront, as is all below)
    uint32_t len = 0;
    if (np2sam::line_kept(lines[r])) {
        const uint32_t s = r ? line_end[r - 1] + 1u : 0u, e = line_end[r];
        uint32_t first = 256u;
        for (uint32_t u = 0; u < 4u && first == 256u; ++u) {
            const uint32_t i = s + 64u * u + lane;
            const uint64_t m = __ballot(i < e && text[i] == (uint8_t)'\t');
            if (m) first = 64u * u + (uint32_t)__builtin_ctzll(m);
        }
        if (first == 0u || first > 254u) {
            if (lane == 0) atomicMin(first_bad, r);
        } else {
            len = first;
        }
    }
    if (lane == 0) n_name[r] = len;
}

__global__ __launch_bounds__(SAM_BLOCK) void k_sam_name_copy(const uint8_t *__restrict__ text, const uint32_t *__restrict__ line_end,
                                                              const Line *__restrict__ lines, uint32_t n_lines, const uint32_t *__restrict__ kept_off,
                                                              const uint32_t *__restrict__ name_off, uint64_t rec_base, uint64_t name_base,
                                                              uint8_t *__restrict__ names, uint64_t *__restrict__ name_ref) {
    const uint32_t r = (blockIdx.x * SAM_BLOCK + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (r >= n_lines) return; // (uniform across the wavefront, as is the next one)
    if (!np2sam::line_kept(lines[r])) return;
    const uint32_t s = r ? line_end[r - 1] + 1u : 0u, len = name_off[r + 1] - name_off[r]; // (at most 254, inside the line)
    const uint64_t to = name_base + name_off[r];
    for (uint32_t j = lane; j < len; j += 64u) names[to + j] = text[s + j];
    if (lane == 0) name_ref[rec_base + kept_off[r]] = to << 8 | len;
}

__global__ __launch_bounds__(SAM_BLOCK) void k_sam_gather_u64(const uint64_t *__restrict__ in, const uint32_t *__restrict__ order, uint32_t n,
                                                               uint64_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * SAM_BLOCK + threadIdx.x;
    if (i < n) out[i] = in[order[i]]; // (order holds each of 0 .. n - 1 once)
}

// ---- NP2_SAM_KEEP_ALL: the tail of a kept line (np2_samtail_core.hpp has the rule and the one-lane walk) ----------------------
__device__ __forceinline__ uint32_t wave_first_word(uint32_t w) { // the smallest error word that is not 0
    w = w ? w : 0xFFFFFFFFu;
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t x = (uint32_t)__shfl_xor(w, o);
        w = x < w ? x : w;
    }
    return w == 0xFFFFFFFFu ? 0u : w;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_excl_sum(uint32_t v, uint32_t lane) {
    uint32_t x = v;
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up(x, o);
        if (lane >= o) x += y;
    }
    return x - v;
}

// One wavefront walks the line text[.., e) behind its CIGAR.  EMIT = false: *size, *aux_len, *has_qual and the error word are
// found (every byte of the tail's text is judged here).  EMIT = true: the line was found good, has_qual is given, and the tail
// goes to out (4-byte aligned, room for pad4(size) bytes).  All arguments and results are uniform across the wavefront.
template <bool EMIT>
__device__ __forceinline__ uint32_t tail_wave(const uint8_t *__restrict__ text, uint32_t e, const Line &ln, const NameTab &nt, uint32_t lane,
                                              uint8_t *__restrict__ out, uint32_t &size, uint32_t &aux_len, bool &has_qual) {
    namespace tl = np2tail;
    size = aux_len = 0;
    // tabs 6 and 7; tab 5 is cig_b, tab 8 is in front of SEQ
    const uint32_t t8 = ln.seq_a - 1u;
    uint32_t t6 = 0, t7 = 0, n_t = 0;
    for (uint32_t c = ln.cig_b + 1u; c < t8 && n_t < 2u; c += 64u) {
        const uint32_t i = c + lane;
        uint64_t m = __ballot(i < t8 && text[i] == (uint8_t)'\t');
        while (m && n_t < 2u) {
            const uint32_t p = c + (uint32_t)__builtin_ctzll(m);
            if (n_t == 0u) t6 = p;
            else t7 = p;
            ++n_t, m &= m - 1ull;
        }
    }
    if (n_t < 2u) return tl::err_word(tl::F_QUAL, tl::T_QUAL_LEN); // (k_sam_fields found ten tabs: not reached)
    uint32_t val = 0xFFFFFFFFu, err = 0; // lane 0: next_refID, 1: next_pos, 2: tlen
    if (lane == 0) {
        int32_t v = -1;
        err = tl::err_word(tl::F_RNEXT, tl::parse_rnext(nt, text, ln.cig_b + 1u, t6, ln.tid, &v));
        val = (uint32_t)v;
    }
    if (lane == 1) {
        int32_t v = -1;
        err = tl::err_word(tl::F_PNEXT, tl::parse_pnext(text, t6 + 1u, t7, &v));
        val = (uint32_t)v;
    }
    if (lane == 2) {
        int32_t v = 0;
        err = tl::err_word(tl::F_TLEN, tl::parse_tlen(text, t7 + 1u, t8, &v));
        val = (uint32_t)v;
    }
    // QUAL: from behind tab 9 to the next tab or the line's end
    const uint32_t tab9 = ln.l_seq ? ln.seq_a + ln.l_seq : text[ln.seq_a] == (uint8_t)'\t' ? ln.seq_a : ln.seq_a + 1u;
    const uint32_t qa = tab9 + 1u;
    uint32_t qb = qa;
    if (!EMIT) {
        bool bad = false;
        for (uint32_t c = qa;; c += 64u) {
            const uint32_t i = c + lane;
            const uint8_t b = i < e ? text[i] : (uint8_t)'\t';
            const uint64_t m = __ballot(b == (uint8_t)'\t');
            const uint32_t first = m ? (uint32_t)__builtin_ctzll(m) : 64u;
            bad = bad || (lane < first && !tl::qual_byte_ok(b));
            if (m) {
                qb = c + first;
                break;
            }
        }
        uint32_t qk = tl::qual_shape(text, qa, qb, ln.l_seq, ln.l_seq == 0u, &has_qual);
        if (has_qual && __ballot(bad)) qk = tl::T_QUAL_BYTE;
        if (lane == 3) err = tl::err_word(tl::F_QUAL, qk);
        if (qk != tl::T_OK) has_qual = false;
    } else {
        qb = has_qual ? qa + ln.l_seq : qa + 1u;
        if (has_qual)
            for (uint32_t j = lane; j < ln.l_seq; j += 64u) out[tl::HEAD_BYTES + j] = (uint8_t)(text[qa + j] - 33u);
    }
    const uint32_t n_qual = has_qual ? ln.l_seq : 0u;
    // the optional fields, 64 a pass: lane k of a pass keeps the tab in front of its field; the 65th tab opens the next pass
    uint32_t aux = 0, base = 0;
    for (uint32_t cur = qb; cur < e;) { // text[cur] is a tab
        uint32_t my_tab = 0, last = 0, n = 0;
        for (uint32_t c = cur; c < e && n < 65u; c += 64u) {
            const uint32_t i = c + lane;
            uint64_t m = __ballot(i < e && text[i] == (uint8_t)'\t');
            while (m && n < 65u) {
                const uint32_t p = c + (uint32_t)__builtin_ctzll(m);
                if (lane == n) my_tab = p;
                if (n == 64u) last = p;
                ++n, m &= m - 1ull;
            }
        }
        const uint32_t nf = n < 64u ? n : 64u;
        const uint32_t nxt = (uint32_t)__shfl(my_tab, (int)((lane + 1u) & 63u));
        const uint32_t a = my_tab + 1u, b = lane + 1u < n ? (lane == 63u ? last : nxt) : e;
        uint32_t sz = 0, fk = tl::T_OK;
        bool wide = false;
        if (lane < nf) fk = tl::field(text, a, b, &sz, &wide, nullptr);
        uint32_t off = 0;
        if (EMIT) {
            off = tl::HEAD_BYTES + n_qual + aux + wave_excl_sum(sz, lane);
            if (lane < nf) (void)tl::field(text, a, b, &sz, &wide, out + off);
        }
        // a long Z or H value: every lane takes part
        for (uint64_t wm = __ballot(lane < nf && fk == tl::T_OK && wide); wm; wm &= wm - 1ull) {
            const int src = __builtin_ctzll(wm);
            const uint32_t wa = (uint32_t)__shfl(a, src) + 5u, wb = (uint32_t)__shfl(b, src);
            if (!EMIT) {
                const bool z = text[wa - 2u] == (uint8_t)'Z';
                bool bad = false;
                for (uint32_t i = wa + lane; i < wb; i += 64u) bad = bad || !(z ? tl::z_byte_ok(text[i]) : tl::h_byte_ok(text[i]));
                if (__ballot(bad) && lane == (uint32_t)src) fk = z ? tl::T_Z : tl::T_H;
            } else {
                const uint32_t wo = (uint32_t)__shfl(off, src) + 3u;
                for (uint32_t i = wa + lane; i < wb; i += 64u) out[wo + (i - wa)] = text[i];
                if (lane == 0) out[wo + (wb - wa)] = 0;
            }
        }
        if (lane < nf) err = tl::first_word(err, tl::err_word(tl::F_OPT + base + lane, fk));
        aux += wave_sum(sz), base += nf;
        cur = n == 65u ? last : e;
    }
    aux_len = aux, size = tl::HEAD_BYTES + n_qual + aux;
    if (EMIT) {
        if (lane < 3u) reinterpret_cast<uint32_t *>(out)[lane] = val;
        if (lane == 3u) reinterpret_cast<uint32_t *>(out)[3] = aux;
        if (lane < tl::pad4(size) - size) out[size + lane] = 0;
        return 0u;
    }
    return wave_first_word(err);
}

// t_size[i]: the padded bytes of a kept line's tail (0 for a line that is not kept, and for entry n_lines); t_aux[i]: its
// aux_len | has_qual << 31.  A kept line with a bad field: *first_bad = min(*first_bad, i) (the host reads the line again).
__global__ __launch_bounds__(SAM_BLOCK) void k_sam_tail_len(const uint8_t *__restrict__ text, const uint32_t *__restrict__ line_end,
                                                             const Line *__restrict__ lines, uint32_t n_lines, NameTab nt,
                                                             uint32_t *__restrict__ t_size, uint32_t *__restrict__ t_aux, uint32_t *__restrict__ first_bad) {
    const uint32_t r = (blockIdx.x * SAM_BLOCK + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (r == n_lines && lane == 0) t_size[r] = t_aux[r] = 0u; // the scan's closing entry
    if (r >= n_lines) return;                                 // (uniform across the wavefront, as is all below)
    const Line ln = lines[r];
    uint32_t size = 0, aux = 0;
    bool has_qual = false;
    if (np2sam::line_kept(ln)) {
        const uint32_t s = r ? line_end[r - 1] + 1u : 0u;
        uint32_t e = line_end[r];
        if (e > s && text[e - 1] == (uint8_t)'\r') --e;
        const uint32_t err = tail_wave<false>(text, e, ln, nt, lane, nullptr, size, aux, has_qual);
        if (err) {
            size = aux = 0, has_qual = false;
            if (lane == 0) atomicMin(first_bad, r);
        }
    }
    if (lane == 0) t_size[r] = np2tail::pad4(size), t_aux[r] = aux | (has_qual ? 0x80000000u : 0u);
}

__global__ __launch_bounds__(SAM_BLOCK) void k_sam_tail_emit(const uint8_t *__restrict__ text, const uint32_t *__restrict__ line_end,
                                                              const Line *__restrict__ lines, uint32_t n_lines, NameTab nt,
                                                              const uint32_t *__restrict__ kept_off, const uint32_t *__restrict__ tail_off,
                                                              const uint32_t *__restrict__ t_aux, uint64_t rec_base, uint64_t tail_base,
                                                              uint8_t *__restrict__ tails, uint64_t *__restrict__ tail_ref) {
    const uint32_t r = (blockIdx.x * SAM_BLOCK + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (r >= n_lines) return; // (uniform across the wavefront, as is the next one)
    const Line ln = lines[r];
    if (!np2sam::line_kept(ln)) return;
    const uint32_t s = r ? line_end[r - 1] + 1u : 0u;
    uint32_t e = line_end[r];
    if (e > s && text[e - 1] == (uint8_t)'\r') --e;
    const uint64_t to = tail_base + tail_off[r]; // a multiple of 4; tail_off[r + 1] - tail_off[r] bytes are this line's
    bool has_qual = (t_aux[r] & 0x80000000u) != 0u;
    uint32_t size = 0, aux = 0;
    (void)tail_wave<true>(text, e, ln, nt, lane, tails + to, size, aux, has_qual);
    if (lane == 0) tail_ref[rec_base + kept_off[r]] = np2tail::tail_ref(to, has_qual);
}

inline dim3 wave_grid(uint64_t waves) { return dim3((uint32_t)((waves * 64u + SAM_BLOCK - 1) / SAM_BLOCK)); }

} // namespace

void launch_sam_tail_len(hipStream_t s, const uint8_t *text, const uint32_t *line_end, const np2sam::Line *lines, uint32_t n_lines,
                         np2sam::NameTab nt, uint32_t *t_size, uint32_t *t_aux, uint32_t *first_bad) {
    hipLaunchKernelGGL(k_sam_tail_len, wave_grid((uint64_t)n_lines + 1), dim3(SAM_BLOCK), 0, s, text, line_end, lines, n_lines, nt, t_size, t_aux,
                       first_bad);
}
void launch_sam_tail_emit(hipStream_t s, const uint8_t *text, const uint32_t *line_end, const np2sam::Line *lines, uint32_t n_lines,
                          np2sam::NameTab nt, const uint32_t *kept_off, const uint32_t *tail_off, const uint32_t *t_aux, uint64_t rec_base,
                          uint64_t tail_base, uint8_t *tails, uint64_t *tail_ref) {
    if (n_lines)
        hipLaunchKernelGGL(k_sam_tail_emit, wave_grid(n_lines), dim3(SAM_BLOCK), 0, s, text, line_end, lines, n_lines, nt, kept_off, tail_off, t_aux,
                           rec_base, tail_base, tails, tail_ref);
}

void launch_sam_lines(hipStream_t s, const Lookback &lb, const uint8_t *text, uint32_t n, uint32_t *line_end, SamCtr *ctr) {
    if (n) hipLaunchKernelGGL(k_sam_lines, dim3(sam_line_blocks(n)), dim3(SAM_BLOCK), 0, s, lb, text, n, line_end, ctr);
}
void launch_sam_fields(hipStream_t s, const uint8_t *text, const uint32_t *line_end, uint32_t n_lines, np2sam::NameTab nt,
                       np2sam::Line *lines, uint32_t *kept, uint32_t *n_cig, uint32_t *n_seq, SamCtr *ctr) {
    hipLaunchKernelGGL(k_sam_fields, wave_grid((uint64_t)n_lines + 1), dim3(SAM_BLOCK), 0, s, text, line_end, n_lines, nt, lines, kept, n_cig,
                       n_seq, ctr);
}
void launch_sam_pack(hipStream_t s, const uint8_t *text, const np2sam::Line *lines, uint32_t n_lines, const uint32_t *kept_off,
                     const uint32_t *cig_off, const uint32_t *seq_off, uint64_t rec_base, uint64_t cig_base, uint64_t seq_base,
                     uint32_t tie_by_strand, uint32_t *recs, int32_t *tids, uint64_t *keys, uint32_t *cigar, uint8_t *seq4) {
    if (n_lines)
        hipLaunchKernelGGL(k_sam_pack, wave_grid(n_lines), dim3(SAM_BLOCK), 0, s, text, lines, n_lines, kept_off, cig_off, seq_off, rec_base,
                           cig_base, seq_base, tie_by_strand, recs, tids, keys, cigar, seq4);
}
void launch_sam_name_len(hipStream_t s, const uint8_t *text, const uint32_t *line_end, const np2sam::Line *lines, uint32_t n_lines,
                         uint32_t *n_name, uint32_t *first_bad) {
    hipLaunchKernelGGL(k_sam_name_len, wave_grid((uint64_t)n_lines + 1), dim3(SAM_BLOCK), 0, s, text, line_end, lines, n_lines, n_name, first_bad);
}
void launch_sam_name_copy(hipStream_t s, const uint8_t *text, const uint32_t *line_end, const np2sam::Line *lines, uint32_t n_lines,
                          const uint32_t *kept_off, const uint32_t *name_off, uint64_t rec_base, uint64_t name_base, uint8_t *names,
                          uint64_t *name_ref) {
    if (n_lines)
        hipLaunchKernelGGL(k_sam_name_copy, wave_grid(n_lines), dim3(SAM_BLOCK), 0, s, text, line_end, lines, n_lines, kept_off, name_off, rec_base,
                           name_base, names, name_ref);
}
void launch_sam_gather_u64(hipStream_t s, const uint64_t *in, const uint32_t *order, uint32_t n, uint64_t *out) {
    if (n) hipLaunchKernelGGL(k_sam_gather_u64, dim3((n + SAM_BLOCK - 1) / SAM_BLOCK), dim3(SAM_BLOCK), 0, s, in, order, n, out);
}
void launch_sam_iota(hipStream_t s, uint32_t *vals, uint32_t n) {
    if (n) hipLaunchKernelGGL(k_sam_iota, dim3((n + SAM_BLOCK - 1) / SAM_BLOCK), dim3(SAM_BLOCK), 0, s, vals, n);
}
void launch_sam_sorted_sizes(hipStream_t s, const uint32_t *recs_in, const uint32_t *order, uint32_t n, uint32_t *n_cig) {
    hipLaunchKernelGGL(k_sam_sorted_sizes, dim3(n / SAM_BLOCK + 1), dim3(SAM_BLOCK), 0, s, recs_in, order, n, n_cig);
}
void launch_sam_gather(hipStream_t s, const uint32_t *recs_in, const int32_t *tids_in, const uint32_t *cigar_in, const uint32_t *order,
                       const uint32_t *cig_off, uint32_t n, uint32_t *recs, int32_t *tids, uint32_t *cigar) {
    if (n) hipLaunchKernelGGL(k_sam_gather, wave_grid(n), dim3(SAM_BLOCK), 0, s, recs_in, tids_in, cigar_in, order, cig_off, n, recs, tids, cigar);
}

} // namespace np2
