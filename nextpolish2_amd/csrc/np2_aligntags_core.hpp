// The aligner's opt-in outputs as plain integer arithmetic without HIP types (the rule's text: include/np2_io.h, np2_map_align_*,
// "Tags"): one walk over a record's final CIGAR against the reference from pos on and the read as aligned, which yields the MD
// text, the short cs text and the CIGAR with every M word split into = and X runs.  The same text is the kernels' inner step
// (np2_aligntags.hip), the host twin (np2_align_tags_host, np2_map_align_host_x) and a stand-alone program
// (tests/tools/aligntags_core_test.cpp).
//
// The fine points, each decided here:
//   Size and emit are one function.  tag_walk with null output pointers counts, with pointers it writes; a decimal's width
//     (dec_len) is computed once and used by both, so the two passes agree byte for byte.
//   Callers.  n_lanes callers walk one record together (lane: this caller); every caller keeps the whole state, which depends
//     only on the CIGAR words and on ballot()'s masks, and so is the same in all of them.  The columns of an M word are taken
//     n_lanes at a time: each caller compares one column, ballot(mismatch) gives all callers the mask of the mismatching
//     callers (bit l: caller l), and the few set bits are consumed in order.  Caller 0 writes numbers and single letters; the
//     letters of a D or I word are dealt out to all callers.  One caller (0, 1) with ballot(b) = b has the walk whole.
//   A match column: np2aln::eq of the two bytes' codes, the predicate of score_ops, so NM = X columns + I bases + D bases.
//   The read as aligned: with rev its reverse complement, ACGT complemented in their case and any other byte kept (sam_seq).
//   Limits.  Only M, I, D and S words; a record's texts and words are counted in 32 bits (a read has fewer than 2^31 bases).
#pragma once
#include <cstdint>

#include "np2_align_core.hpp"

namespace np2aln {

enum : uint32_t { OP_EQ = 7, OP_X = 8 };
enum : uint32_t { ALN_QUAL = 1, ALN_MD = 2, ALN_CS = 4, ALN_EQX = 8, ALN_FLAGS = 15 };

NP2_KC_HD uint8_t comp_byte(uint8_t b) {
    switch (b) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    case 'a': return 't';
    case 'c': return 'g';
    case 'g': return 'c';
    case 't': return 'a';
    default: return b;
    }
}
// MD's letter: A-Z kept, a-z upper-cased, any other byte N.  cs's: letters lower-cased, any other byte n.
NP2_KC_HD char md_letter(uint8_t b) { return b >= 'A' && b <= 'Z' ? (char)b : b >= 'a' && b <= 'z' ? (char)(b - 32) : 'N'; }
NP2_KC_HD char cs_letter(uint8_t b) { return b >= 'a' && b <= 'z' ? (char)b : b >= 'A' && b <= 'Z' ? (char)(b + 32) : 'n'; }

NP2_KC_HD uint32_t dec_len(uint32_t v) {
    uint32_t n = 1;
    while (v >= 10u) v /= 10u, ++n;
    return n;
}
NP2_KC_HD void put_dec(char *p, uint32_t v, uint32_t n) { // n = dec_len(v)
    while (n-- > 0) p[n] = (char)('0' + v % 10u), v /= 10u;
}

struct TagIn {
    const uint8_t *t;    // the reference from the record's pos on
    const uint8_t *q;    // the read's bytes as they are stored
    uint32_t qlen, rev;  // rev: it is aligned as its reverse complement
    const uint32_t *cigar;
    uint32_t n_cigar;    // 0: no text at all (an unmapped record)
    NP2_KC_HD uint8_t qb(uint32_t i) const { return rev ? comp_byte(q[qlen - 1u - i]) : q[i]; }
};
struct TagOut { // a null pointer: that output is counted only
    char *md, *cs;
    uint32_t *eqx;
    uint32_t n_md, n_cs, n_eqx;
};

struct TagWalk {
    TagOut o;
    uint32_t lane, n_lanes;
    uint32_t c = 0, run = 0; // MD's match counter; cs's match run inside one M word
    uint32_t x_op = 0, x_len = 0; // the open = / X run
    NP2_KC_HD TagWalk(const TagOut &out, uint32_t l, uint32_t n) : o(out), lane(l), n_lanes(n) { o.n_md = o.n_cs = o.n_eqx = 0; }
    NP2_KC_HD void md_put(char ch) {
        if (o.md && lane == 0) o.md[o.n_md] = ch;
        ++o.n_md;
    }
    NP2_KC_HD void md_num(uint32_t v) {
        const uint32_t n = dec_len(v);
        if (o.md && lane == 0) put_dec(o.md + o.n_md, v, n);
        o.n_md += n;
    }
    NP2_KC_HD void cs_put(char ch) {
        if (o.cs && lane == 0) o.cs[o.n_cs] = ch;
        ++o.n_cs;
    }
    NP2_KC_HD void cs_flush() {
        if (!run) return;
        cs_put(':');
        const uint32_t n = dec_len(run);
        if (o.cs && lane == 0) put_dec(o.cs + o.n_cs, run, n);
        o.n_cs += n, run = 0;
    }
    NP2_KC_HD void x_flush() {
        if (!x_len) return;
        if (o.eqx && lane == 0) o.eqx[o.n_eqx] = x_len << 4 | x_op;
        ++o.n_eqx, x_len = 0;
    }
    NP2_KC_HD void x_push(uint32_t op, uint32_t len) {
        if (!len) return;
        if (x_len && x_op == op) {
            x_len += len;
            return;
        }
        x_flush();
        x_op = op, x_len = len;
    }
    NP2_KC_HD void x_word(uint32_t w) { // a word that is kept as it is
        x_flush();
        if (o.eqx && lane == 0) o.eqx[o.n_eqx] = w;
        ++o.n_eqx;
    }
    NP2_KC_HD void matches(uint32_t n) { c += n, run += n, x_push(OP_EQ, n); }
    NP2_KC_HD void mismatch(uint8_t tb, uint8_t qb) {
        md_num(c), md_put(md_letter(tb)), c = 0;
        cs_flush();
        cs_put('*'), cs_put(cs_letter(tb)), cs_put(cs_letter(qb));
        x_push(OP_X, 1u);
    }
};

// ballot(bool) -> uint64_t: bit l is set where caller l passed true
template <class Ballot> NP2_KC_HD void tag_walk(const TagIn &in, TagOut &out, uint32_t lane, uint32_t n_lanes, Ballot ballot) {
    TagWalk w(out, lane, n_lanes);
    uint32_t r = 0, q = 0;
    for (uint32_t x = 0; x < in.n_cigar; ++x) {
        const uint32_t op = in.cigar[x] & 15u, len = in.cigar[x] >> 4;
        if (op == OP_M) {
            for (uint32_t base = 0; base < len; base += n_lanes) {
                const uint32_t col = base + lane;
                const bool mis = col < len && !eq(np2map::code(in.t[r + col]), np2map::code(in.qb(q + col)));
                uint64_t mask = ballot(mis);
                const uint32_t n = len - base < n_lanes ? len - base : n_lanes;
                uint32_t prev = 0;
                while (mask) {
                    const uint32_t p = (uint32_t)__builtin_ctzll(mask);
                    mask &= mask - 1;
                    w.matches(p - prev);
                    w.mismatch(in.t[r + base + p], in.qb(q + base + p));
                    prev = p + 1u;
                }
                w.matches(n - prev);
            }
            w.cs_flush(), w.x_flush();
            r += len, q += len;
        } else if (op == OP_D) {
            w.md_num(w.c), w.md_put('^'), w.c = 0;
            w.cs_put('-');
            for (uint32_t i = lane; i < len; i += n_lanes) {
                const uint8_t tb = in.t[r + i];
                if (w.o.md) w.o.md[w.o.n_md + i] = md_letter(tb);
                if (w.o.cs) w.o.cs[w.o.n_cs + i] = cs_letter(tb);
            }
            w.o.n_md += len, w.o.n_cs += len;
            w.x_word(in.cigar[x]);
            r += len;
        } else if (op == OP_I) {
            w.cs_put('+');
            for (uint32_t i = lane; i < len && w.o.cs; i += n_lanes) w.o.cs[w.o.n_cs + i] = cs_letter(in.qb(q + i));
            w.o.n_cs += len;
            w.x_word(in.cigar[x]);
            q += len;
        } else { // S
            w.x_word(in.cigar[x]);
            q += len;
        }
    }
    if (in.n_cigar) w.md_num(w.c);
    out = w.o;
}

// what the doors check of a caller's CIGAR before any walk: only M, I, D, S words; *t_span, *q_span: the reference and read
// bytes its columns touch
NP2_KC_HD bool tag_cigar_spans(const uint32_t *cigar, uint64_t n, uint64_t *t_span, uint64_t *q_span) {
    uint64_t t = 0, q = 0;
    for (uint64_t x = 0; x < n; ++x) {
        const uint32_t op = cigar[x] & 15u, len = cigar[x] >> 4;
        if (op == OP_M) t += len, q += len;
        else if (op == OP_D) t += len;
        else if (op == OP_I || op == OP_S) q += len;
        else return false;
    }
    *t_span = t, *q_span = q;
    return true;
}

} // namespace np2aln
