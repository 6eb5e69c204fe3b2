// Per-lane arithmetic of the k-mer counter (np2_kcount.hip): byte -> 2-bit code -> rolled forward / reverse-complement
// words -> canonical k-mer -> yak hash -> (bucket, slot key, file word), as plain integer arithmetic without HIP types.
// The same text is the count kernel's inner step and a one-lane host program (tests/tools/kcount_core_test.cpp, which
// counts a separator stream into a std::unordered_map on a machine without a GPU).
//
// Semantics are those of the reference's LOOKUP side, so that a table counted here answers KmerInfo::get as a table
// counted by yak would: iter2kmer (src/utils/kmer.rs:255-287: SEQ_NUM maps ACGTUacgtu to 0-3, any other byte resets the
// run; forward and reverse-complement word, the smaller one), to_hash (kmer.rs:102-110: yak_hash64(kmer, mask), k < 32),
// bucket = hash & 1023 and file word = (hash >> 10) << 10 | count with 10 counter bits (kmer.rs:52-58,123-170).
// A byte >= 0x80 is a non-base (SEQ_NUM has 128 entries and read files are foreign bytes).
//
// Separator stream: the reads' sequence bytes as they stand in the file with one '\n' (any non-base) after every read.
// A separator resets the run like an N, so counting needs no read offsets.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NP2_KC_HD __host__ __device__ __forceinline__
#else
#define NP2_KC_HD inline
#endif

namespace np2kc {

static constexpr uint32_t HALO = 32;         // bytes of the stream kept in front of every piece: >= k - 1 for k < 32, two 16-byte loads
static constexpr uint32_t PRE = 10;          // prefix bits: 1024 buckets
static constexpr uint32_t N_BUCKETS = 1u << PRE;
static constexpr uint32_t COUNT_BITS = 10;   // YAK_COUNTER_BITS
static constexpr uint32_t COUNT_MAX = (1u << COUNT_BITS) - 1;
static constexpr uint64_t EMPTY = ~0ULL;     // a file word never has its top bits set (hash < 2^62)

// SEQ_NUM restricted to the bases: A/a 0, C/c 1, G/g 2, T/t/U/u 3, everything else (bytes >= 0x80 included) 4
NP2_KC_HD uint32_t code(uint8_t ch) {
    const uint32_t u = (uint32_t)(ch & 0xDFu) - (uint32_t)'A'; // letters of either case -> 0 .. 25; any other byte >= 26 or a non-base letter
    const uint32_t VALID = 1u | 1u << 2 | 1u << 6 | 1u << 19 | 1u << 20; // A C G T U
    const uint64_t CODES = 1ull << 4 | 2ull << 12 | 3ull << 38 | 3ull << 40;
    if (u >= 32u || !((VALID >> u) & 1u)) return 4u;
    return (uint32_t)(CODES >> (2u * u)) & 3u;
}

// yak_hash64 (kmer.rs:223-233; np2_common.hpp holds the polish kernels' copy, which needs the HIP headers)
NP2_KC_HD uint64_t hash64(uint64_t key, uint64_t mask) {
    key = (~key + (key << 21)) & mask;
    key = key ^ key >> 24;
    key = ((key + (key << 3)) + (key << 8)) & mask;
    key = key ^ key >> 14;
    key = ((key + (key << 2)) + (key << 4)) & mask;
    key = key ^ key >> 28;
    key = (key + (key << 31)) & mask;
    return key;
}

struct Roll {
    uint64_t fw = 0, rv = 0;
    uint32_t l = 0; // bases since the last non-base, capped at k
};
NP2_KC_HD uint64_t kmer_mask(uint32_t k) { return (1ULL << (2u * k)) - 1ULL; }

// One byte of the stream.  True when the last k bytes were all bases: *hash is then the table hash of the k-mer that
// ENDS at this byte (the lane that owns a k-mer's last byte counts it).
NP2_KC_HD bool push(Roll &r, uint8_t ch, uint32_t k, uint64_t mask, uint64_t *hash) {
    const uint32_t c = code(ch);
    if (c >= 4u) {
        r.l = 0;
        return false;
    }
    r.fw = ((r.fw << 2) | (uint64_t)c) & mask;
    r.rv = (r.rv >> 2) | ((uint64_t)(3u - c) << (2u * (k - 1u)));
    if (r.l < k) ++r.l;
    if (r.l < k) return false;
    *hash = hash64(r.fw < r.rv ? r.fw : r.rv, mask);
    return true;
}

NP2_KC_HD uint32_t bucket_of(uint64_t hash) { return (uint32_t)(hash & (N_BUCKETS - 1)); }
NP2_KC_HD uint64_t key_of(uint64_t hash) { return hash >> PRE; }
NP2_KC_HD uint64_t word_of(uint64_t hash, uint32_t count) { return (hash >> PRE) << COUNT_BITS | (uint64_t)count; }
NP2_KC_HD uint32_t sat_add(uint32_t count, uint32_t add) { return count + add > COUNT_MAX ? COUNT_MAX : count + add; }

} // namespace np2kc
