// CRC-32 of gzip / BGZF (reflected polynomial 0xEDB88320, register starts at ~0, final ~), as plain integer arithmetic without
// HIP types: the same text is the device kernel's arithmetic (np2_crc32.hip: k_bgzf_crc32, one wavefront per BGZF block)
// and a one-lane host program (tests/tools/crc32_core_test.cpp against zlib on a machine without a GPU).
//
// A block is cut into 64 pieces that 64 lanes run through the table-driven register update at once; the pieces' registers
// are then joined by the algebra of the code: the register is a residue mod p(x) over GF(2), appending n bytes to a piece
// multiplies its residue by x^(8n), so for a piece A followed by a piece B of n bytes
//     reg(A || B) = mulmod(reg(A), x^(8n)) ^ reg0(B)          (reg0: the register run from 0)
// The block lies RIGHT-ALIGNED in a frame of 64 KiB: zero bytes in front of it leave a zero register zero, so the padding
// costs nothing and every piece is PIECE = 1024 bytes whatever the block's length — the six shift constants of the fold,
// x^(8 * 1024 * 2^s), are compile-time constants.  Lane l owns frame bytes [1024 l, 1024 (l + 1)); the one lane that holds
// the block's first byte starts at ~0 there, every other lane at 0.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NP2_CRC_HD __host__ __device__ __forceinline__
#else
#define NP2_CRC_HD inline
#endif

namespace np2crc {

static constexpr uint32_t POLY = 0xEDB88320u;
static constexpr uint32_t FRAME = 65536u; // the largest piece of data one call of the scheme takes (a BGZF block's bound)
static constexpr uint32_t LANES = 64u;
static constexpr uint32_t PIECE = FRAME / LANES;

// the register after `bits` zero bits (one division step per bit)
constexpr NP2_CRC_HD uint32_t shift_bits(uint32_t r, uint32_t bits) {
    for (uint32_t i = 0; i < bits; ++i) r = (r >> 1) ^ (POLY & (0u - (r & 1u)));
    return r;
}
// word `i` of slice `k` (k = 0 .. 3) of the slice-by-4 tables: the register that byte i leaves behind after k more zero bytes
constexpr NP2_CRC_HD uint32_t table_word(uint32_t k, uint32_t i) { return shift_bits(i, 8u * (k + 1u)); }

struct Tables {
    uint32_t t[1024]; // slice k at 256 k
};
constexpr Tables make_tables() {
    Tables T{};
    for (uint32_t k = 0; k < 4; ++k)
        for (uint32_t i = 0; i < 256; ++i) T.t[256u * k + i] = table_word(k, i);
    return T;
}
static constexpr Tables TABLES = make_tables(); // (host side; the kernel fills its LDS copy from table_word)
static_assert(TABLES.t[1] == 0x77073096u && TABLES.t[255] == 0x2D02EF8Du, "the CRC-32 table of gzip");

// a * b mod p in the reflected representation (bit 31 = x^0): 32 steps whatever the operands, no branch
// (zlib's multmodp leaves its loop when the rest of `a` is zero, and never does for a == 0)
constexpr NP2_CRC_HD uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32; ++i) {
        p ^= b & (0u - ((a >> (31u - i)) & 1u));
        b = (b >> 1) ^ (POLY & (0u - (b & 1u)));
    }
    return p;
}
// x^(2^k) mod p
constexpr uint32_t x_pow2(uint32_t k) {
    uint32_t v = 0x40000000u; // x^1
    for (uint32_t i = 0; i < k; ++i) v = mulmod(v, v);
    return v;
}
// fold step s joins neighbours of 2^s pieces each: the left one moves up by 8 * PIECE * 2^s = 2^(13 + s) bits
constexpr NP2_CRC_HD uint32_t fold_const(uint32_t s) {
    constexpr uint32_t K[6] = {x_pow2(13), x_pow2(14), x_pow2(15), x_pow2(16), x_pow2(17), x_pow2(18)};
    return K[s];
}
static_assert(PIECE == 1024u && LANES == 64u, "fold_const: six steps from x^8192 on");
static_assert(x_pow2(13) == shift_bits(0x80000000u, 8192u), "x^8192 by squaring = by 8192 division steps");

// register update over 4 / 1 bytes (T: 4 x 256 words, slice k at T + 256 k)
NP2_CRC_HD uint32_t step4(const uint32_t *T, uint32_t r, uint32_t w) {
    r ^= w;
    return T[768u + (r & 255u)] ^ T[512u + ((r >> 8) & 255u)] ^ T[256u + ((r >> 16) & 255u)] ^ T[r >> 24];
}
NP2_CRC_HD uint32_t step1(const uint32_t *T, uint32_t r, uint32_t byte) { return T[(r ^ byte) & 255u] ^ (r >> 8); }

// What lane `lane` does with a block of n <= FRAME bytes at d: the register of its piece of the frame.  The piece's end is
// always a piece boundary of the frame; its begin is too, except in the lane that holds the block's first byte.
// Reads d[lo, hi) only, lo >= 0, hi <= n.
struct LanePiece {
    uint32_t lo, hi; // the lane's bytes of the block (lo == hi: none)
    bool first;      // holds the block's first byte
};
NP2_CRC_HD LanePiece lane_piece(uint32_t n, uint32_t lane) {
    const uint32_t pad = FRAME - n;                       // zero bytes in front of the block
    const uint32_t f_lo = lane * PIECE, f_hi = f_lo + PIECE; // the lane's frame bytes
    LanePiece p;
    p.hi = f_hi > pad ? f_hi - pad : 0u;
    p.lo = f_lo > pad ? f_lo - pad : 0u;
    p.first = n != 0u && p.hi != 0u && p.lo == 0u;
    return p;
}
// the piece's odd bytes in front of its 16-byte chunks (only the lane that holds the block's first byte has any): the
// chunks then end on the piece's end, which every lane's tile grid is laid out from
NP2_CRC_HD uint32_t piece_head(const LanePiece p) { return (p.hi - p.lo) & 15u; }
// One lane's register: the head bytes one at a time, then 16-byte chunks through load16 (the kernel takes the same chunks,
// in the same order, out of its LDS tiles).
template <class Load16> NP2_CRC_HD uint32_t lane_reg(const uint32_t *T, const uint8_t *d, const LanePiece p, Load16 load16) {
    if (p.lo == p.hi) return 0u;
    uint32_t r = p.first ? 0xFFFFFFFFu : 0u;
    uint32_t at = p.lo;
    for (uint32_t head = piece_head(p); head; --head) r = step1(T, r, d[at++]);
    for (; at < p.hi; at += 16u) {
        uint32_t w[4];
        load16(d + at, w);
        r = step4(T, r, w[0]);
        r = step4(T, r, w[1]);
        r = step4(T, r, w[2]);
        r = step4(T, r, w[3]);
    }
    return r;
}
// step s of the fold as lane `lane` sees it: `left` is the register of lane - 2^s
NP2_CRC_HD uint32_t fold_step(uint32_t s, uint32_t lane, uint32_t mine, uint32_t left) {
    const uint32_t span = 2u << s;
    return (lane & (span - 1u)) == span - 1u ? (mulmod(left, fold_const(s)) ^ mine) : mine;
}

// The whole scheme with one lane playing all 64 (what the kernel computes, restated for the host test): CRC-32 of d[0, n).
inline uint32_t crc32_by_pieces(const uint8_t *d, uint32_t n) {
    uint32_t reg[LANES];
    for (uint32_t l = 0; l < LANES; ++l)
        reg[l] = lane_reg(TABLES.t, d, lane_piece(n, l), [](const uint8_t *p, uint32_t *w) { __builtin_memcpy(w, p, 16); });
    if (n == 0u) reg[LANES - 1u] = 0xFFFFFFFFu; // (no lane holds a first byte: the empty block's register is the start value)
    for (uint32_t s = 0; s < 6u; ++s) {
        uint32_t next[LANES];
        for (uint32_t l = 0; l < LANES; ++l) next[l] = fold_step(s, l, reg[l], l >= (1u << s) ? reg[l - (1u << s)] : 0u);
        for (uint32_t l = 0; l < LANES; ++l) reg[l] = next[l];
    }
    return ~reg[LANES - 1u];
}
// plain serial CRC-32 over the same tables (any length)
inline uint32_t crc32_serial(const uint8_t *d, uint64_t n) {
    uint32_t r = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; ++i) r = step1(TABLES.t, r, d[i]);
    return ~r;
}

} // namespace np2crc
