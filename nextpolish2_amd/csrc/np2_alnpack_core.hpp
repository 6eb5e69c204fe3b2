// The aligner's records as the resident SAM handle holds them (the rule is in include/np2_io.h: "the resident SAM straight
// from reads"): which reads are kept, a record's ten words, the bytes of its SEQ as the SAM text would print them, their
// nibbles, and the packed bytes and words.  Plain integer arithmetic without HIP types: the same text is the kernels' inner
// step (np2_alnpack.hip), the host twin (np2_align_pack_host: np2_alnpack_host.cpp) and a stand-alone program
// (tests/tools/alnpack_core_test.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "np2_align_core.hpp"
#include "np2_sam_core.hpp"

namespace np2pack {

static constexpr uint32_t REC_WORDS = 10; // np2_bamrec_t as 32-bit words, padding included

// A read is kept when it is aligned: unmapped and overflowed reads (tid -1, flag 4) are counted and dropped.
NP2_SAM_HD bool kept(const np2aln::Rec &r) { return r.tid >= 0 && !(r.flag & 4u); }

// ACGT complemented in their case; any other byte itself (np2aln::sam_seq)
NP2_SAM_HD uint8_t comp(uint8_t c) {
    const uint8_t u = c & 0xDFu, k = c & 0x20u; // (u is 'A' only for 'A' and 'a': bit 5 is the one cleared)
    uint8_t r = c;
    r = u == (uint8_t)'A' ? (uint8_t)((uint8_t)'T' | k) : r;
    r = u == (uint8_t)'C' ? (uint8_t)((uint8_t)'G' | k) : r;
    r = u == (uint8_t)'G' ? (uint8_t)((uint8_t)'C' | k) : r;
    r = u == (uint8_t)'T' ? (uint8_t)((uint8_t)'A' | k) : r;
    return r;
}

// column j of the SEQ of the read q[0, len): the read's bytes, with flag 16 reversed and complemented
NP2_SAM_HD uint8_t seq_byte(const uint8_t *q, uint32_t len, bool rev, uint32_t j) { return rev ? comp(q[len - 1u - j]) : q[j]; }
NP2_SAM_HD uint32_t seq_nibble(const uint8_t *q, uint32_t len, bool rev, uint32_t j) { return np2sam::base_code(seq_byte(q, len, rev, j)); }
// packed byte b < (len + 1) / 2: columns 2 b (high nibble) and 2 b + 1 (low; 0 behind an odd read's last base)
NP2_SAM_HD uint8_t seq4_byte(const uint8_t *q, uint32_t len, bool rev, uint32_t b) {
    const uint32_t hi = seq_nibble(q, len, rev, 2u * b), lo = 2u * b + 1u < len ? seq_nibble(q, len, rev, 2u * b + 1u) : 0u;
    return (uint8_t)(hi << 4 | lo);
}

// The eight bytes from p on, wherever p lies, as a little-endian word: two aligned 8-byte loads and a funnel shift.  Reads
// the 16 bytes from p rounded down to a multiple of 8 (8 when p is one).
NP2_SAM_HD uint64_t load8(const uint8_t *p) {
    const uintptr_t a = (uintptr_t)p;
    const uint32_t s = (uint32_t)(a & 7u) * 8u;
    const uint8_t *w = p - (a & 7u);
    uint64_t lo, hi;
    __builtin_memcpy(&lo, __builtin_assume_aligned(w, 8), 8);
    if (s == 0u) return lo;
    __builtin_memcpy(&hi, __builtin_assume_aligned(w + 8, 8), 8);
    return lo >> s | hi << (64u - s);
}
// packed bytes b0 .. b0 + 3 as one little-endian word; all eight columns lie inside the read (2 b0 + 8 <= len)
NP2_SAM_HD uint32_t seq4_word(const uint8_t *q, uint32_t len, bool rev, uint32_t b0) {
    const uint64_t v = load8(rev ? q + (len - 8u - 2u * b0) : q + 2u * b0);
    uint32_t out = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t t = 0; t < 8u; ++t) { // column 2 b0 + t: the reverse strand takes the window's bytes from its far end
        const uint8_t c = rev ? comp((uint8_t)(v >> (8u * (7u - t)))) : (uint8_t)(v >> (8u * t));
        out |= np2sam::base_code(c) << (8u * (t >> 1) + ((t & 1u) ? 0u : 4u));
    }
    return out;
}

// word j < REC_WORDS of the record of a kept read of `len` bases whose CIGAR words start at co and whose SEQ starts at byte so
NP2_SAM_HD uint32_t rec_word(const np2aln::Rec &r, uint32_t len, uint64_t co, uint64_t so, uint32_t j) {
    switch (j) {
    case 0: return r.pos;
    case 1: return (r.flag & 0xFFFFu) | (r.mapq & 0xFFu) << 16;
    case 2: return r.n_cigar;
    case 4: return (uint32_t)co;
    case 5: return (uint32_t)(co >> 32);
    case 6: return len;
    case 8: return (uint32_t)so;
    case 9: return (uint32_t)(so >> 32);
    }
    return 0u; // the pad words
}
NP2_SAM_HD uint64_t rec_key(const np2aln::Rec &r, uint32_t tie_by_strand) { return np2sam::sort_key(r.tid, (int32_t)r.pos, r.flag, tie_by_strand); }

// ---- host only: the whole rule as a plain loop ----------------------------------------------------------------------------------
// recs[n_reads], read i's CIGAR words cigar[cigar_off[i] .. cigar_off[i + 1]), the reads as a separator stream of n bytes ->
// the kept records in sorted order (REC_WORDS words each: cigar_off in sorted order, seq_off as the reads were met), their tids,
// CIGAR words and packed SEQ.  false: the stream does not hold n_reads separators or does not end in one.
inline bool pack_host(const np2aln::Rec *recs, const uint32_t *cigar, const uint64_t *cigar_off, const uint8_t *reads, uint64_t n,
                      uint64_t n_reads, uint32_t tie_by_strand, std::vector<uint32_t> &out_recs, std::vector<int32_t> &tids,
                      std::vector<uint32_t> &out_cigar, std::vector<uint8_t> &seq4) {
    std::vector<uint64_t> ends;
    if (n && reads[n - 1] != '\n') return false;
    for (uint64_t at = 0; at < n; at = ends.back() + 1) ends.push_back((uint64_t)((const uint8_t *)memchr(reads + at, '\n', n - at) - reads));
    if (ends.size() != n_reads) return false;
    struct In {
        uint64_t read, key, so;
        uint32_t len;
    };
    std::vector<In> in; // the kept reads, input order
    uint64_t from = 0;
    for (uint64_t i = 0; i < n_reads; from = ends[i] + 1, ++i) {
        if (!kept(recs[i])) continue;
        const uint32_t len = (uint32_t)(ends[i] - from);
        const bool rev = (recs[i].flag & 16u) != 0;
        in.push_back(In{i, rec_key(recs[i], tie_by_strand), (uint64_t)seq4.size(), len});
        for (uint32_t b = 0; b < (len + 1u) / 2u; ++b) seq4.push_back(seq4_byte(reads + from, len, rev, b));
    }
    std::vector<size_t> order(in.size());
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return in[a].key < in[b].key; });
    for (size_t k : order) {
        const np2aln::Rec &r = recs[in[k].read];
        const uint64_t co = out_cigar.size();
        for (uint32_t j = 0; j < REC_WORDS; ++j) out_recs.push_back(rec_word(r, in[k].len, co, in[k].so, j));
        tids.push_back(r.tid);
        out_cigar.insert(out_cigar.end(), cigar + cigar_off[in[k].read], cigar + cigar_off[in[k].read] + r.n_cigar);
    }
    return true;
}

} // namespace np2pack
