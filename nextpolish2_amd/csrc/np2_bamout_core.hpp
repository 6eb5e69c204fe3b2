// Per-record arithmetic of the BAM writer (np2_bamout.hip; the rule is in include/np2_io.h): the size of a record, its
// reference span, its bin, the value of byte `idx` of its encoding, and a virtual offset.  Plain integer arithmetic without
// HIP types: the same text is the kernels' inner step and the host twin (np2_bamout_host), which is the statement of what
// the kernels must produce.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NP2_BAM_HD __host__ __device__ __forceinline__
#else
#define NP2_BAM_HD inline
#endif

namespace np2bam {

static constexpr uint32_t BLOCK_BYTES = 65280;       // bytes of the stream in a BGZF block
static constexpr uint32_t FIXED_BYTES = 36;          // block_size and the fixed fields
static constexpr uint32_t QNAME_MAX = 254;          // bytes of a QNAME (l_read_name counts the NUL and is one byte)
static constexpr uint32_t CIGAR_MAX = 65535;         // n_cigar_op is 16 bits, and no CG tag is written
static constexpr uint64_t REF_MAX = 1ull << 29;      // what BAI's bins and windows address
static constexpr uint32_t WIN_SHIFT = 14;            // a window of the linear index: 16384 bases
static constexpr uint32_t NONE = 0xFFFFFFFFu;

// the first record (in the resident order) of each refusal; NONE: there is none
struct Refusals {
    uint32_t neg_pos;   // pos < 0
    uint32_t big_cigar; // n_cigar > CIGAR_MAX
    uint32_t far_end;   // pos + max(span, 1) > REF_MAX
};

NP2_BAM_HD uint32_t reg2bin(uint32_t beg, uint32_t end) { // [beg, end), end > beg, end <= REF_MAX
    --end;
    if (beg >> 14 == end >> 14) return 4681u + (beg >> 14);
    if (beg >> 17 == end >> 17) return 585u + (beg >> 17);
    if (beg >> 20 == end >> 20) return 73u + (beg >> 20);
    if (beg >> 23 == end >> 23) return 9u + (beg >> 23);
    if (beg >> 26 == end >> 26) return 1u + (beg >> 26);
    return 0u;
}

// the reference bases of CIGAR words: the lengths of M, D, N, = and X
NP2_BAM_HD uint64_t cigar_span(const uint32_t *cigar, uint32_t n) {
    uint64_t span = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t op = cigar[i] & 15u;
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) span += cigar[i] >> 4;
    }
    return span;
}

// one record as the encoder sees it; the pointers are at the record's own first name byte, CIGAR word, SEQ byte and tail byte.
// tail == nullptr is the lean record: no mate, no quality, no optional field.  Otherwise the tail (np2_samtail_core.hpp) begins
// at a 4-byte boundary: next_refID, next_pos, tlen, aux_len, then l_seq quality bytes if has_qual, then aux_len bytes.
static constexpr uint32_t TAIL_HEAD = 16;
struct Rec {
    int32_t tid, pos;
    uint32_t flag, mapq, n_cigar, l_seq, name_len, bin;
    const uint8_t *name;
    const uint32_t *cigar;
    const uint8_t *seq;
    const uint8_t *tail;
    uint32_t has_qual, aux_len;
};
NP2_BAM_HD uint32_t tail_word(const uint8_t *tail, uint32_t w) {
    const uint8_t *p = tail + 4u * w;
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// bytes of the record in the stream, its block_size word included
NP2_BAM_HD uint64_t rec_bytes(uint32_t name_len, uint32_t n_cigar, uint32_t l_seq, uint32_t aux_len = 0u) {
    return (uint64_t)FIXED_BYTES + name_len + 1u + 4ull * n_cigar + (l_seq + 1u) / 2u + l_seq + aux_len;
}

NP2_BAM_HD uint32_t fixed_word(const Rec &r, uint32_t w) {
    if (r.tail && w >= 6u) return tail_word(r.tail, w - 6u);
    switch (w) {
    case 0: return (uint32_t)(rec_bytes(r.name_len, r.n_cigar, r.l_seq, r.aux_len) - 4u);
    case 1: return (uint32_t)r.tid;
    case 2: return (uint32_t)r.pos;
    case 3: return (r.name_len + 1u) | r.mapq << 8 | r.bin << 16;
    case 4: return r.n_cigar | r.flag << 16;
    case 5: return r.l_seq;
    case 6: return 0xFFFFFFFFu; // next_refID
    case 7: return 0xFFFFFFFFu; // next_pos
    }
    return 0u; // tlen
}

// byte idx of the record, idx below rec_bytes
NP2_BAM_HD uint8_t rec_byte(const Rec &r, uint64_t idx) {
    if (idx < FIXED_BYTES) return (uint8_t)(fixed_word(r, (uint32_t)idx >> 2) >> (8u * ((uint32_t)idx & 3u)));
    idx -= FIXED_BYTES;
    if (idx <= r.name_len) return idx < r.name_len ? r.name[idx] : (uint8_t)0;
    idx -= r.name_len + 1u;
    if (idx < 4ull * r.n_cigar) return (uint8_t)(r.cigar[idx >> 2] >> (8u * ((uint32_t)idx & 3u)));
    idx -= 4ull * r.n_cigar;
    const uint32_t n_seq = (r.l_seq + 1u) / 2u;
    if (idx < n_seq) return (r.l_seq & 1u) && idx + 1u == n_seq ? (uint8_t)(r.seq[idx] & 0xF0u) : r.seq[idx];
    idx -= n_seq;
    if (idx < r.l_seq) return r.has_qual ? r.tail[TAIL_HEAD + idx] : (uint8_t)0xFF;
    return r.tail[TAIL_HEAD + (r.has_qual ? idx : idx - r.l_seq)]; // an optional field's byte: idx - l_seq below aux_len
}
// where the quality bytes, or the run of 0xFF bytes, begin; the optional fields follow l_seq bytes later
NP2_BAM_HD uint64_t qual_begin(const Rec &r) { return rec_bytes(r.name_len, r.n_cigar, r.l_seq, 0u) - r.l_seq; }
// where the packed SEQ bytes begin
NP2_BAM_HD uint64_t seq_begin(const Rec &r) { return (uint64_t)FIXED_BYTES + r.name_len + 1u + 4ull * r.n_cigar; }

// the virtual offset of stream offset u: C[b] is the file offset of BGZF block b
NP2_BAM_HD uint64_t voff(const uint64_t *C, uint64_t u) { return C[u / BLOCK_BYTES] << 16 | u % BLOCK_BYTES; }

// a record's name among the kept names: offset << 8 | length
NP2_BAM_HD uint64_t name_ref(uint64_t off, uint32_t len) { return off << 8 | len; }
NP2_BAM_HD uint64_t name_off(uint64_t ref) { return ref >> 8; }
NP2_BAM_HD uint32_t name_len(uint64_t ref) { return (uint32_t)(ref & 255u); }

} // namespace np2bam
