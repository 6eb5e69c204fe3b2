// Per-lane logic of NP2_SAM_KEEP_ALL (np2_sam.hip: k_sam_tail_len, k_sam_tail_emit; the rule is in include/np2_io.h): the mate
// fields, the QUAL check, and SAM's typed optional fields TAG:TYPE:VALUE -> BAM's binary ones.  Plain integer and double
// arithmetic without HIP types: the same text is the kernels' inner step and the host twin (np2_sam_tails_host), which walks a
// line with tail_line below the way a wavefront does with its 64 lanes.
//
// A record's tail: next_refID i32, next_pos i32, tlen i32, aux_len u32, then l_seq quality bytes if QUAL is present, then
// aux_len bytes of optional fields; zero bytes up to a multiple of 4, so that every tail begins at a word.
#pragma once
#include <cstdint>

#include "np2_sam_core.hpp"

namespace np2tail {

static constexpr uint32_t HEAD_BYTES = 16;  // the four words in front of the quality bytes
static constexpr uint32_t LANE_VALUE = 64;  // a Z or H value of more bytes is checked and copied by the whole wavefront
static constexpr uint32_t F_RNEXT = 0, F_PNEXT = 1, F_TLEN = 2, F_QUAL = 3, F_OPT = 4; // fields in line order; F_OPT + k: optional field k

// what is wrong with a field; T_WINDOW alone is NP2_E_UNSUPPORTED, the others NP2_E_ARG
enum : uint32_t {
    T_OK = 0, T_RNEXT, T_PNEXT, T_TLEN, T_QUAL_LEN, T_QUAL_BYTE, T_QUAL_NO_SEQ, T_SHORT, T_TAG, T_TYPE, T_A, T_INT, T_FLOAT, T_WINDOW, T_Z, T_H, T_B, T_QNAME
};
inline const char *kind_text(uint32_t k) {
    switch (k) {
    case T_RNEXT: return "RNEXT is neither *, = nor the name of an @SQ line";
    case T_PNEXT: return "PNEXT is not a decimal number in 0..2147483647";
    case T_TLEN: return "TLEN is not a decimal number of magnitude at most 2147483647";
    case T_QUAL_LEN: return "QUAL is not as long as SEQ";
    case T_QUAL_BYTE: return "QUAL has a byte outside '!'..'~'";
    case T_QUAL_NO_SEQ: return "QUAL is given while SEQ is *";
    case T_SHORT: return "an optional field is shorter than TAG:TYPE:";
    case T_TAG: return "an optional field does not begin with [A-Za-z][A-Za-z0-9]:TYPE:";
    case T_TYPE: return "an optional field's type is not one of A i f Z H B";
    case T_A: return "an A value is not one byte in '!'..'~'";
    case T_INT: return "an integer value is not a decimal number in -2147483648..4294967295, or outside its array's type";
    case T_FLOAT: return "a float value is not [-+]?digits[.digits]?([eE][-+]?digits)?";
    case T_WINDOW: return "a float value is inf, nan, has 2^53 or more as its digits or a decimal exponent beyond 22: only values one IEEE operation converts exactly are taken";
    case T_Z: return "a Z value has a byte outside ' '..'~'";
    case T_H: return "an H value is not an even number of hex digits";
    case T_B: return "a B value is not [cCsSiIf](,number)*";
    case T_QNAME: return "QNAME is empty or longer than 254 bytes";
    }
    return "ok";
}
// a line's error word: (field + 1) << 8 | kind; of several on one line the smallest speaks: the first field in line order
NP2_SAM_HD uint32_t err_word(uint32_t field, uint32_t kind) { return kind == T_OK ? 0u : (field + 1u) << 8 | kind; }
NP2_SAM_HD uint32_t first_word(uint32_t a, uint32_t b) { return a == 0u ? b : b == 0u ? a : a < b ? a : b; }
NP2_SAM_HD uint32_t word_kind(uint32_t w) { return w & 255u; }
NP2_SAM_HD uint32_t word_field(uint32_t w) { return (w >> 8) - 1u; }

NP2_SAM_HD bool is_alpha(uint8_t c) { return (uint8_t)((c | 0x20u) - (uint8_t)'a') < 26u; }
NP2_SAM_HD bool is_print(uint8_t c) { return c >= (uint8_t)'!' && c <= (uint8_t)'~'; }
NP2_SAM_HD bool z_byte_ok(uint8_t c) { return c >= (uint8_t)' ' && c <= (uint8_t)'~'; }
NP2_SAM_HD bool h_byte_ok(uint8_t c) { return np2sam::is_digit(c) || (uint8_t)((c | 0x20u) - (uint8_t)'a') < 6u; }

// ---- RNEXT, PNEXT, TLEN ---------------------------------------------------------------------------------------------------
NP2_SAM_HD uint32_t parse_rnext(const np2sam::NameTab &nt, const uint8_t *t, uint32_t a, uint32_t b, int32_t own_tid, int32_t *tid) {
    if (b - a == 1u && t[a] == (uint8_t)'=') {
        *tid = own_tid;
        return T_OK;
    }
    if (a >= b) return T_RNEXT;
    *tid = np2sam::name_lookup(nt, t, a, b);
    return *tid == np2sam::TID_UNKNOWN ? T_RNEXT : T_OK;
}
NP2_SAM_HD uint32_t parse_pnext(const uint8_t *t, uint32_t a, uint32_t b, int32_t *pos) {
    uint64_t v = 0;
    if (!np2sam::parse_dec(t, a, b, 2147483647u, &v)) return T_PNEXT;
    *pos = (int32_t)v - 1;
    return T_OK;
}
NP2_SAM_HD uint32_t parse_tlen(const uint8_t *t, uint32_t a, uint32_t b, int32_t *tlen) {
    const bool neg = a < b && t[a] == (uint8_t)'-';
    if (a < b && (t[a] == (uint8_t)'-' || t[a] == (uint8_t)'+')) ++a;
    uint64_t v = 0;
    if (!np2sam::parse_dec(t, a, b, 2147483647u, &v)) return T_TLEN;
    *tlen = neg ? -(int32_t)v : (int32_t)v;
    return T_OK;
}

// ---- numbers ---------------------------------------------------------------------------------------------------------------
// [-+]?digits with a magnitude of at most 2^32 (more saturates there): false for anything else
NP2_SAM_HD bool parse_int(const uint8_t *t, uint32_t a, uint32_t b, bool *neg, uint64_t *mag) {
    *neg = a < b && t[a] == (uint8_t)'-';
    if (a < b && (t[a] == (uint8_t)'-' || t[a] == (uint8_t)'+')) ++a;
    if (a >= b) return false;
    uint64_t x = 0;
    for (uint32_t i = a; i < b; ++i) {
        if (!np2sam::is_digit(t[i])) return false;
        x = x * 10u + (uint64_t)(t[i] - (uint8_t)'0');
        if (x > (1ull << 32)) x = 1ull << 32;
    }
    *mag = x;
    return true;
}
// the smallest BAM type of the integer: one of cCsSiI, 0 when none holds it
NP2_SAM_HD uint8_t int_type(bool neg, uint64_t mag) {
    if (!neg || mag == 0u) return mag <= 255u ? 'C' : mag <= 65535u ? 'S' : mag <= 0xFFFFFFFFull ? 'I' : 0;
    return mag <= 128u ? 'c' : mag <= 32768u ? 's' : mag <= (1ull << 31) ? 'i' : 0;
}
NP2_SAM_HD bool int_fits(uint8_t type, bool neg, uint64_t mag) {
    if (neg && mag) return type == 'c' ? mag <= 128u : type == 's' ? mag <= 32768u : type == 'i' ? mag <= (1ull << 31) : false;
    return type == 'c' ? mag <= 127u : type == 'C' ? mag <= 255u : type == 's' ? mag <= 32767u : type == 'S' ? mag <= 65535u :
           type == 'i' ? mag <= 0x7FFFFFFFull : mag <= 0xFFFFFFFFull;
}
NP2_SAM_HD uint32_t type_bytes(uint8_t type) { return type == 'c' || type == 'C' || type == 'A' ? 1u : type == 's' || type == 'S' ? 2u : 4u; }
NP2_SAM_HD uint32_t int_bits(bool neg, uint64_t mag) { return neg ? (uint32_t)(0u - (uint32_t)mag) : (uint32_t)mag; }

NP2_SAM_HD bool word_is(const uint8_t *t, uint32_t a, uint32_t b, const char *w, uint32_t n) {
    if (b - a != n) return false;
    for (uint32_t i = 0; i < n; ++i)
        if ((uint8_t)(t[a + i] | 0x20u) != (uint8_t)w[i]) return false;
    return true;
}
// [-+]?digits[.digits]?([eE][-+]?digits)? -> the float's bits.  M: all the digits read as an integer, e: the exponent minus
// the number of fraction digits.  Taken only when M < 2^53 and |e| <= 22: M and 10^|e| are then exact doubles, and one IEEE
// multiplication or division rounds their product or quotient correctly, which is the double strtod gives.
NP2_SAM_HD uint32_t parse_float(const uint8_t *t, uint32_t a, uint32_t b, uint32_t *bits) {
    uint32_t i = a;
    const bool neg = i < b && t[i] == (uint8_t)'-';
    if (i < b && (t[i] == (uint8_t)'-' || t[i] == (uint8_t)'+')) ++i;
    if (word_is(t, i, b, "inf", 3) || word_is(t, i, b, "infinity", 8) || word_is(t, i, b, "nan", 3)) return T_WINDOW;
    uint64_t M = 0;
    bool big = false;
    uint32_t n_int = 0, n_fra = 0;
    for (; i < b && np2sam::is_digit(t[i]); ++i, ++n_int) {
        M = M * 10u + (uint64_t)(t[i] - (uint8_t)'0');
        if (M >= (1ull << 53)) big = true, M = 1ull << 53;
    }
    if (!n_int) return T_FLOAT;
    if (i < b && t[i] == (uint8_t)'.') {
        for (++i; i < b && np2sam::is_digit(t[i]); ++i, ++n_fra) {
            M = M * 10u + (uint64_t)(t[i] - (uint8_t)'0');
            if (M >= (1ull << 53)) big = true, M = 1ull << 53;
        }
        if (!n_fra) return T_FLOAT;
    }
    int64_t ex = 0;
    if (i < b && (t[i] | 0x20u) == (uint8_t)'e') {
        ++i;
        const bool eneg = i < b && t[i] == (uint8_t)'-';
        if (i < b && (t[i] == (uint8_t)'-' || t[i] == (uint8_t)'+')) ++i;
        uint32_t n_exp = 0;
        for (; i < b && np2sam::is_digit(t[i]); ++i, ++n_exp) {
            ex = ex * 10 + (int64_t)(t[i] - (uint8_t)'0');
            if (ex > 100000) ex = 100000;
        }
        if (!n_exp) return T_FLOAT;
        if (eneg) ex = -ex;
    }
    if (i != b) return T_FLOAT;
    const int64_t e = ex - (int64_t)(n_fra > 100000u ? 100000u : n_fra);
    if (big || e > 22 || e < -22) return T_WINDOW;
    const double P[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    // One correctly rounded IEEE operation: the library is built without fast-math, and this line needs that (a reciprocal
    // and a multiplication in place of the division would round twice).
    const double d = e >= 0 ? (double)M * P[e] : (double)M / P[-e];
    const float f = (float)(neg ? -d : d);
    union { float f; uint32_t u; } cv;
    cv.f = f;
    *bits = cv.u;
    return T_OK;
}

NP2_SAM_HD void put(uint8_t *out, uint32_t v, uint32_t n_bytes) {
    for (uint32_t k = 0; k < n_bytes; ++k) out[k] = (uint8_t)(v >> (8u * k));
}
// one number of type `type` (one of cCsSiIf) from text[a, b): its bits, or what is wrong
NP2_SAM_HD uint32_t parse_number(uint8_t type, const uint8_t *t, uint32_t a, uint32_t b, uint32_t *bits) {
    if (type == 'f') return parse_float(t, a, b, bits);
    bool neg;
    uint64_t mag = 0;
    if (!parse_int(t, a, b, &neg, &mag) || !int_fits(type, neg, mag)) return T_INT;
    *bits = int_bits(neg, mag);
    return T_OK;
}

// ---- one optional field text[a, b) -----------------------------------------------------------------------------------------
// Its binary size and what is wrong with it.  *wide: a Z or H value of more than LANE_VALUE bytes, whose bytes have NOT been
// looked at: the caller checks them (z_byte_ok / h_byte_ok) and copies them itself.  out != nullptr: the field is written
// there too (of a wide value only TAG and type; the caller adds the value and its NUL).
NP2_SAM_HD uint32_t field(const uint8_t *t, uint32_t a, uint32_t b, uint32_t *size, bool *wide, uint8_t *out) {
    *size = 0, *wide = false;
    if (b - a < 5u) return T_SHORT;
    if (!is_alpha(t[a]) || !(is_alpha(t[a + 1]) || np2sam::is_digit(t[a + 1])) || t[a + 2] != (uint8_t)':' || t[a + 4] != (uint8_t)':') return T_TAG;
    const uint8_t type = t[a + 3];
    const uint32_t v = a + 5u, n = b - v;
    if (out) out[0] = t[a], out[1] = t[a + 1];
    switch (type) {
    case 'A':
        if (n != 1u || !is_print(t[v])) return T_A;
        *size = 4u;
        if (out) out[2] = 'A', out[3] = t[v];
        return T_OK;
    case 'i': {
        bool neg;
        uint64_t mag = 0;
        if (!parse_int(t, v, b, &neg, &mag)) return T_INT;
        const uint8_t bt = int_type(neg, mag);
        if (!bt) return T_INT;
        *size = 3u + type_bytes(bt);
        if (out) out[2] = bt, put(out + 3, int_bits(neg, mag), type_bytes(bt));
        return T_OK;
    }
    case 'f': {
        uint32_t bits = 0;
        const uint32_t k = parse_float(t, v, b, &bits);
        if (k != T_OK) return k;
        *size = 7u;
        if (out) out[2] = 'f', put(out + 3, bits, 4u);
        return T_OK;
    }
    case 'Z':
    case 'H':
        if (type == 'H' && (n & 1u)) return T_H;
        *size = 3u + n + 1u;
        if (out) out[2] = type;
        if (n > LANE_VALUE) {
            *wide = true;
            return T_OK;
        }
        for (uint32_t i = 0; i < n; ++i) {
            if (!(type == 'Z' ? z_byte_ok(t[v + i]) : h_byte_ok(t[v + i]))) return type == 'Z' ? T_Z : T_H;
            if (out) out[3u + i] = t[v + i];
        }
        if (out) out[3u + n] = 0;
        return T_OK;
    case 'B': {
        if (n < 1u) return T_B;
        const uint8_t sub = t[v];
        if (!(sub == 'c' || sub == 'C' || sub == 's' || sub == 'S' || sub == 'i' || sub == 'I' || sub == 'f')) return T_B;
        const uint32_t w = type_bytes(sub);
        uint32_t count = 0, i = v + 1u;
        while (i < b) { // every element: a comma, then a number up to the next comma
            if (t[i] != (uint8_t)',') return T_B;
            uint32_t j = i + 1u;
            while (j < b && t[j] != (uint8_t)',') ++j;
            uint32_t bits = 0;
            const uint32_t k = parse_number(sub, t, i + 1u, j, &bits);
            if (k != T_OK) return k;
            if (out) put(out + 8u + w * count, bits, w);
            ++count, i = j;
        }
        *size = 8u + w * count;
        if (out) out[2] = 'B', out[3] = sub, put(out + 4, count, 4u);
        return T_OK;
    }
    }
    return T_TYPE;
}

// ---- QUAL text[a, b) of a record with l_seq bases; seq_star: SEQ is "*" or empty ---------------------------------------------
// what the length says; the bytes are checked apart (qual_byte_ok), by the lanes that copy them
NP2_SAM_HD uint32_t qual_shape(const uint8_t *t, uint32_t a, uint32_t b, uint32_t l_seq, bool seq_star, bool *has_qual) {
    *has_qual = false;
    if (b - a == 1u && t[a] == (uint8_t)'*') return T_OK;
    if (seq_star) return T_QUAL_NO_SEQ;
    if (b - a != l_seq) return T_QUAL_LEN;
    *has_qual = true;
    return T_OK;
}
NP2_SAM_HD bool qual_byte_ok(uint8_t c) { return is_print(c); }

NP2_SAM_HD uint32_t pad4(uint32_t n) { return (n + 3u) & ~3u; }
// tail_ref of a record: offset << 1 | has_qual
NP2_SAM_HD uint64_t tail_ref(uint64_t off, bool has_qual) { return off << 1 | (has_qual ? 1u : 0u); }
NP2_SAM_HD uint64_t tail_off(uint64_t ref) { return ref >> 1; }
NP2_SAM_HD bool tail_has_qual(uint64_t ref) { return (ref & 1u) != 0; }

// where the fields behind CIGAR lie in a line that k_sam_fields took (ln.cig_b is tab 5, ln.seq_a - 1 tab 8)
struct Spots {
    uint32_t rnext_a, rnext_b, pnext_a, pnext_b, tlen_a, tlen_b, qual_a, qual_b; // qual_b: the tab behind QUAL, or the line's end
    bool seq_star;
};
// One lane's walk: false when the line has fewer tabs than k_sam_fields found (it cannot).
NP2_SAM_HD bool find_spots(const uint8_t *t, uint32_t e, const np2sam::Line &ln, Spots *sp) {
    uint32_t i = ln.cig_b + 1u;
    sp->rnext_a = i;
    while (i < e && t[i] != (uint8_t)'\t') ++i;
    sp->rnext_b = i, sp->pnext_a = ++i;
    while (i < e && t[i] != (uint8_t)'\t') ++i;
    sp->pnext_b = i, sp->tlen_a = i + 1u, sp->tlen_b = ln.seq_a - 1u;
    if (sp->tlen_a > sp->tlen_b) return false;
    const uint32_t tab9 = ln.l_seq ? ln.seq_a + ln.l_seq : t[ln.seq_a] == (uint8_t)'\t' ? ln.seq_a : ln.seq_a + 1u;
    sp->seq_star = ln.l_seq == 0u;
    sp->qual_a = tab9 + 1u;
    i = sp->qual_a;
    while (i < e && t[i] != (uint8_t)'\t') ++i;
    sp->qual_b = i;
    return sp->qual_a <= e;
}

// The tail of the line text[.., e) that parse_line took as `ln`, by one lane: *size = its bytes before padding, *aux_len, the
// error word (0: none).  out != nullptr (room for pad4(*size) bytes): the tail is written too.  The order of the steps and
// every rule are the wavefront's (k_sam_tail_len, k_sam_tail_emit).
NP2_SAM_HD uint32_t tail_line(const uint8_t *t, uint32_t e, const np2sam::Line &ln, const np2sam::NameTab &nt, uint32_t *size, uint32_t *aux_len,
                              bool *has_qual, uint8_t *out) {
    Spots sp;
    *size = 0, *aux_len = 0, *has_qual = false;
    if (!find_spots(t, e, ln, &sp)) return err_word(F_QUAL, T_QUAL_LEN);
    int32_t ntid = -1, npos = -1, tlen = 0;
    uint32_t err = 0;
    err = first_word(err, err_word(F_RNEXT, parse_rnext(nt, t, sp.rnext_a, sp.rnext_b, ln.tid, &ntid)));
    err = first_word(err, err_word(F_PNEXT, parse_pnext(t, sp.pnext_a, sp.pnext_b, &npos)));
    err = first_word(err, err_word(F_TLEN, parse_tlen(t, sp.tlen_a, sp.tlen_b, &tlen)));
    uint32_t qk = qual_shape(t, sp.qual_a, sp.qual_b, ln.l_seq, sp.seq_star, has_qual);
    if (*has_qual)
        for (uint32_t i = sp.qual_a; i < sp.qual_b; ++i)
            if (!qual_byte_ok(t[i])) qk = T_QUAL_BYTE;
    err = first_word(err, err_word(F_QUAL, qk));
    const uint32_t n_qual = *has_qual && qk == T_OK ? ln.l_seq : 0u;
    if (out && qk == T_OK)
        for (uint32_t i = 0; i < n_qual; ++i) out[HEAD_BYTES + i] = (uint8_t)(t[sp.qual_a + i] - 33u);
    uint32_t aux = 0, k = 0;
    for (uint32_t a = sp.qual_b; a < e; ++k) { // a: the tab in front of optional field k
        uint32_t b = ++a;
        while (b < e && t[b] != (uint8_t)'\t') ++b;
        uint32_t sz = 0;
        bool wide = false;
        uint8_t *to = out && err == 0u ? out + HEAD_BYTES + n_qual + aux : nullptr;
        uint32_t fk = field(t, a, b, &sz, &wide, to);
        if (fk == T_OK && wide) {
            const bool z = t[a + 3] == (uint8_t)'Z';
            for (uint32_t i = a + 5u; i < b; ++i) {
                if (!(z ? z_byte_ok(t[i]) : h_byte_ok(t[i]))) fk = z ? T_Z : T_H;
                if (to) to[3u + (i - a - 5u)] = t[i];
            }
            if (to) to[sz - 1u] = 0;
        }
        err = first_word(err, err_word(F_OPT + k, fk));
        aux += sz, a = b;
    }
    *aux_len = aux, *size = HEAD_BYTES + n_qual + aux;
    if (out && err == 0u) {
        put(out, (uint32_t)ntid, 4u), put(out + 4, (uint32_t)npos, 4u), put(out + 8, (uint32_t)tlen, 4u), put(out + 12, aux, 4u);
        for (uint32_t i = *size; i < pad4(*size); ++i) out[i] = 0;
    }
    return err;
}

} // namespace np2tail
