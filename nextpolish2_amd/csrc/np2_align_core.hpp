// The aligner's rule as plain integer arithmetic without HIP types (the rule's text: include/np2_io.h, np2_map_align_*): the
// pins of a primary chain, a segment's trim and class, one cell of the banded affine recurrence and its traceback bits, the
// walk back through them, the choice of an end extension's cell, and a read's assembly: CIGAR words, left-alignment, pos, NM
// and AS.  The same text is the kernels' inner step (np2_align.hip), the host aligner (np2_map_align_host: np2_align_cpu.hpp)
// and a stand-alone program (tests/tools/align_core_test.cpp).
//
// The fine points, each decided here:
//   Matrix.  Row i = 0 .. ql counts read bases taken, column j = 0 .. tl reference bases; a cell's diagonal is j - i.  A band is
//     the diagonals lo .. lo + W - 1; a cell outside it or outside the matrix holds NEG.  cells = (ql + 1) * W.
//   Recurrence.  E (deletion: a reference base against nothing) = max(E(i, j-1), H(i, j-1) - gap_open) - gap_ext; F
//     (insertion) likewise from (i-1, j); H = max(H(i-1, j-1) + s, E, F), s = +match or -mismatch.  H(0, 0) = 0; row 0 is one
//     deletion, column 0 one insertion.
//   Preference.  H takes the diagonal, then E, then F, of equal values; E and F continue an open gap (take E(i, j-1), F(i-1, j))
//     rather than open a new one, of equal values.  The walk starts in H at the end cell and follows these bits.
//   Extension.  The best cell is the largest H; of equal cells the smallest row, then the smallest column (the origin, 0, is a
//     cell).  The read-end cell exists only when every remaining read base is in the matrix (remainder <= ext_max and <=
//     reference left + band); it is the largest H of the last row, of equal cells the smallest column.
//   Ends of the CIGAR.  After the clips are set, an insertion that touches a clip joins it and a deletion that touches a clip is
//     dropped (pos moves past it); repeated until an M column touches the clip.
//   Left-alignment.  Gaps are visited left to right.  A gap moves one column left while the column before it is a match column of
//     an M run, that column's base equals the gap's last base, and the run is not the alignment's first M run down to one column.
//     An M run used up between two gaps of one kind merges them, and the merged gap moves on as one gap.
//   Limits.  match 1 .. 15, mismatch 0 .. 31, gap_open 0 .. 255, gap_ext 1 .. 15, band 0 .. 1023, end_bonus <= 2^16, ext_max 1 ..
//     2^20, max_cells 1 .. 2^24: every reachable cell's score then stays inside (-2^30, 2^30).  A band wider than MAX_W = 2048
//     diagonals overflows like one beyond max_cells (the device keeps one row of H and F in LDS).
#pragma once
#include <cstdint>

#include "np2_map_core.hpp"

namespace np2aln {

static constexpr int32_t NEG = -(1 << 30);
static constexpr uint32_t MAX_W = 2048;
enum : uint32_t { OP_M = 0, OP_I = 1, OP_D = 2, OP_S = 4 };
// a slot's kind: a segment as the plan leaves it (RAW) and as the classification settles it, an end extension, nothing
enum : uint32_t { K_EQUAL = 0, K_GAP = 1, K_SNV = 2, K_CORE = 3, K_HEAD = 4, K_TAIL = 5, K_EMPTY = 6, K_RAW = 7 };

struct Opts { // (the order of np2_align_opts_t)
    uint32_t match, mismatch, gap_open, gap_ext, band, end_bonus, ext_max, max_cells;
};
// One unit of work of a read: its head extension, each segment between two pins, its tail extension, in that order.  t0, q0:
// the first reference and read base of the matrix on the chain's strand; a head runs backwards from t0 - 1, q0 - 1.
struct Slot {
    uint32_t t0, q0, tl, ql, pre, suf, kind, W;
    int32_t lo;
    uint32_t over; // the band or the cell count is beyond the limits: the read is not aligned
};
struct Res { // the cell a slot's walk starts from, and its score
    int32_t score;
    uint32_t ei, ej;
};
struct Rec { // (the order of np2_align_rec_t)
    int32_t tid;
    uint32_t flag, pos, end, mapq, n_cigar, nm;
    int32_t as;
};
enum { C_PINS, C_SEGMENTS, C_EQUAL, C_GAP, C_SNV, C_CORES, C_CELLS, C_CLIPPED, C_OVERFLOW, C_N };

NP2_KC_HD const char *check_opts(const Opts &o) {
    if (o.match < 1 || o.match > 15) return "match must lie in 1 .. 15";
    if (o.mismatch > 31) return "mismatch must be at most 31";
    if (o.gap_open > 255) return "gap_open must be at most 255";
    if (o.gap_ext < 1 || o.gap_ext > 15) return "gap_ext must lie in 1 .. 15";
    if (o.band > 1023) return "band must be at most 1023";
    if (o.end_bonus > (1u << 16)) return "end_bonus must be at most 2^16";
    if (o.ext_max < 1 || o.ext_max > (1u << 20)) return "ext_max must lie in 1 .. 2^20";
    if (o.max_cells < 1 || o.max_cells > (1u << 24)) return "max_cells must lie in 1 .. 2^24";
    return nullptr;
}

// one contig and one read; the read's bases on the chain's strand
struct Seqs {
    const uint8_t *t;
    uint32_t tlen;
    const uint8_t *q;
    uint32_t qlen, rev;
    NP2_KC_HD uint32_t tc(uint32_t j) const { return np2map::code(t[j]); }
    NP2_KC_HD uint32_t qc(uint32_t i) const {
        if (!rev) return np2map::code(q[i]);
        const uint32_t c = np2map::code(q[qlen - 1u - i]);
        return c < 4u ? 3u - c : 4u;
    }
};
NP2_KC_HD bool eq(uint32_t a, uint32_t b) { return a < 4u && a == b; }
// base j / i of a slot's matrix (0-based)
NP2_KC_HD uint32_t slot_t(const Seqs &s, const Slot &x, uint32_t j) { return x.kind == K_HEAD ? s.tc(x.t0 - 1u - j) : s.tc(x.t0 + j); }
NP2_KC_HD uint32_t slot_q(const Seqs &s, const Slot &x, uint32_t i) { return x.kind == K_HEAD ? s.qc(x.q0 - 1u - i) : s.qc(x.q0 + i); }

// ---- pins --------------------------------------------------------------------------------------------------------------------
// chain: n (r, q) pairs, first to last.  pin[i] (may be null) = anchor i is a pin.  Returns the number of pins.
NP2_KC_HD uint32_t mark_pins(const uint32_t *chain, uint32_t n, uint32_t k, uint8_t *pin) {
    uint32_t np = 0, pr = 0, pq = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t r = chain[2 * i], q = chain[2 * i + 1];
        const bool is = i == 0 || (r >= pr + k && q >= pq + k); // (r - k + 1 > pr, without the unsigned wrap)
        if (pin) pin[i] = is;
        if (is) ++np, pr = r, pq = q;
    }
    return np;
}

NP2_KC_HD Slot ext_slot(uint32_t kind, uint32_t t_at, uint32_t q_at, uint32_t rem, uint32_t ref_left, const Opts &o) {
    uint32_t n = rem < o.ext_max ? rem : o.ext_max;
    if ((uint64_t)ref_left + o.band < n) n = ref_left + o.band;
    Slot x{};
    x.t0 = t_at, x.q0 = q_at, x.ql = n;
    x.tl = (uint64_t)n + o.band < ref_left ? n + o.band : ref_left;
    x.kind = n ? kind : (uint32_t)K_EMPTY;
    x.lo = -(int32_t)o.band, x.W = 2u * o.band + 1u;
    return x;
}

// a mapped read's slots: head, the raw segments between its pins, tail (pins + 1 of them); pin[] as mark_pins leaves it
NP2_KC_HD void plan_read(const uint32_t *chain, uint32_t n, uint32_t k, const uint8_t *pin, uint32_t tlen, uint32_t qlen, const Opts &o,
                         Slot *slots) {
    uint32_t s = 0, pr = 0, pq = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!pin[i]) continue;
        const uint32_t r = chain[2 * i], q = chain[2 * i + 1];
        if (s == 0) {
            slots[s++] = ext_slot(K_HEAD, r - k + 1u, q - k + 1u, q - k + 1u, r - k + 1u, o);
        } else {
            Slot x{};
            x.t0 = pr + 1u, x.q0 = pq + 1u, x.tl = r - k - pr, x.ql = q - k - pq, x.kind = K_RAW;
            slots[s++] = x;
        }
        pr = r, pq = q;
    }
    slots[s] = ext_slot(K_TAIL, pr + 1u, pq + 1u, qlen - 1u - pq, tlen - 1u - pr, o);
}

// ---- classify ----------------------------------------------------------------------------------------------------------------
// settles a slot in place; returns the cells of its matrix (0: no matrix, or over the limits)
NP2_KC_HD uint64_t classify(const Seqs &s, Slot &x, const Opts &o, uint32_t max_cells) {
    x.over = 0;
    if (x.kind == K_EMPTY) return 0;
    if (x.kind == K_RAW) {
        const uint32_t m = x.tl < x.ql ? x.tl : x.ql;
        uint32_t pre = 0, suf = 0;
        while (pre < m && eq(s.tc(x.t0 + pre), s.qc(x.q0 + pre))) ++pre;
        if (x.tl == x.ql && pre == m) {
            x.kind = K_EQUAL, x.pre = pre, x.suf = 0;
            return 0;
        }
        while (suf < m - pre && eq(s.tc(x.t0 + x.tl - 1u - suf), s.qc(x.q0 + x.ql - 1u - suf))) ++suf;
        x.pre = pre, x.suf = suf, x.t0 += pre, x.q0 += pre, x.tl -= pre + suf, x.ql -= pre + suf;
        if (x.tl == 0 || x.ql == 0) {
            x.kind = K_GAP;
            return 0;
        }
        if (x.tl == 1 && x.ql == 1) {
            x.kind = K_SNV;
            return 0;
        }
        x.kind = K_CORE;
        const int64_t d = (int64_t)x.tl - (int64_t)x.ql;
        x.lo = (int32_t)((d < 0 ? d : 0) - (int64_t)o.band);
        const uint64_t W = (uint64_t)(d < 0 ? -d : d) + 2ull * o.band + 1ull;
        x.W = W > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)W;
    }
    const uint64_t cells = ((uint64_t)x.ql + 1ull) * x.W;
    if (x.W > MAX_W || cells > max_cells) {
        x.over = 1;
        return 0;
    }
    return cells;
}

// ---- the recurrence ----------------------------------------------------------------------------------------------------------
// traceback bits of a cell: bits 0-1 H's source (0 diagonal, 1 E, 2 F), bit 2 E continues a gap, bit 3 F continues a gap
NP2_KC_HD int32_t gap_of(int32_t h_prev, int32_t g_prev, const Opts &o, uint32_t *cont) {
    const int32_t open = h_prev - (int32_t)o.gap_open;
    *cont = g_prev >= open ? 1u : 0u;
    return (g_prev >= open ? g_prev : open) - (int32_t)o.gap_ext;
}
NP2_KC_HD int32_t h_of(int32_t d, int32_t e, int32_t f, uint32_t *src) {
    if (d >= e && d >= f) return *src = 0u, d;
    if (e >= f) return *src = 1u, e;
    return *src = 2u, f;
}
NP2_KC_HD int32_t sub_score(uint32_t a, uint32_t b, const Opts &o) { return eq(a, b) ? (int32_t)o.match : -(int32_t)o.mismatch; }
// row 0 (j <= tl): H, E and the bits
NP2_KC_HD int32_t row0_h(uint32_t j, const Opts &o) { return j ? -(int32_t)(o.gap_open + j * o.gap_ext) : 0; }
NP2_KC_HD uint32_t row0_tb(uint32_t j) { return j ? (1u | (j > 1u ? 4u : 0u)) : 0u; }

// an extension's candidates: `a` is better than `b`
NP2_KC_HD bool better_cell(int32_t ha, uint32_t ia, uint32_t ja, int32_t hb, uint32_t ib, uint32_t jb) {
    return ha != hb ? ha > hb : ia != ib ? ia < ib : ja < jb;
}
// best cell (bh at bi, bj) and, with has_end, the last row's best (eh at column ej) -> the cell the walk starts from
NP2_KC_HD Res choose_end(int32_t bh, uint32_t bi, uint32_t bj, bool has_end, int32_t eh, uint32_t ej, uint32_t rows, const Opts &o) {
    if (has_end && eh + (int32_t)o.end_bonus >= bh) return Res{eh, rows, ej};
    return Res{bh, bi, bj};
}
NP2_KC_HD bool slot_has_end(const Slot &x, uint32_t rem) { return x.ql == rem; }

// the walk back from (ei, ej) to (0, 0): emit(op) per column, last column first
template <class Emit> NP2_KC_HD void tb_walk(const uint8_t *tb, uint32_t W, int32_t lo, uint32_t ei, uint32_t ej, Emit emit) {
    uint32_t i = ei, j = ej, state = 0;
    while (i > 0 || j > 0) {
        const uint32_t b = tb[(uint64_t)i * W + (uint32_t)((int32_t)j - (int32_t)i - lo)];
        if (state == 0) {
            state = b & 3u;
            if (state == 0) emit((uint32_t)OP_M), --i, --j;
        } else if (state == 1) {
            emit((uint32_t)OP_D), --j;
            if (!(b & 4u)) state = 0;
        } else {
            emit((uint32_t)OP_I), --i;
            if (!(b & 8u)) state = 0;
        }
    }
}

// ---- assembly ----------------------------------------------------------------------------------------------------------------
struct Sink { // run-length ops, adjacent equal ops merged; out may be null (count only)
    uint32_t *out;
    uint32_t n = 0, op = 0, len = 0;
    NP2_KC_HD explicit Sink(uint32_t *o) : out(o) {}
    NP2_KC_HD void flush() {
        if (!len) return;
        if (out) out[n] = len << 4 | op;
        ++n, len = 0;
    }
    NP2_KC_HD void push(uint32_t o, uint32_t l) {
        if (!l) return;
        if (len && op == o) {
            len += l;
            return;
        }
        flush();
        op = o, len = l;
    }
};

struct ReadIn {
    Seqs s;
    const uint32_t *chain;
    const uint8_t *pin;
    uint32_t n, k;      // the chain's anchors
    const Slot *slots;  // pins + 1
    const Res *res;
    const uint64_t *tb_off; // per slot: its matrix's bits are at tb + (tb_off - tb_base)
    const uint8_t *tb;
    uint64_t tb_base;
    uint32_t n_slots;
};

NP2_KC_HD bool read_over(const ReadIn &in) {
    for (uint32_t i = 0; i < in.n_slots; ++i)
        if (in.slots[i].over) return true;
    return false;
}

// Pass A: the read's raw ops into `a` (null: count only), first op first.  Returns their number; *t_start, *clip5: where the
// first column stands.  The ops are built last to first (a walk yields its last column first) and turned round at the end; the
// head's walk yields its outermost column first, so its run is turned back.
NP2_KC_HD uint32_t raw_ops(const ReadIn &in, uint32_t *a, uint32_t *t_start) {
    Sink k(a);
    const Slot &tail = in.slots[in.n_slots - 1];
    const uint32_t q_end = tail.q0; // the read base after the last pin
    if (tail.kind == K_TAIL) {
        const Res &r = in.res[in.n_slots - 1];
        k.push(OP_S, in.s.qlen - q_end - r.ei);
        tb_walk(in.tb + (in.tb_off[in.n_slots - 1] - in.tb_base), tail.W, tail.lo, r.ei, r.ej, [&](uint32_t op) { k.push(op, 1u); });
    } else {
        k.push(OP_S, in.s.qlen - q_end);
    }
    uint32_t si = in.n_slots - 1; // the slot before pin `si` (counting pins from 1)
    for (uint32_t i = in.n; i-- > 0;) {
        if (!in.pin[i]) continue;
        k.push(OP_M, in.k);
        --si;
        if (si == 0) break;
        const Slot &x = in.slots[si];
        if (x.kind == K_EQUAL) {
            k.push(OP_M, x.pre);
        } else {
            k.push(OP_M, x.suf);
            if (x.kind == K_GAP) k.push(x.tl ? (uint32_t)OP_D : (uint32_t)OP_I, x.tl ? x.tl : x.ql);
            else if (x.kind == K_SNV) k.push(OP_M, 1u);
            else tb_walk(in.tb + (in.tb_off[si] - in.tb_base), x.W, x.lo, x.ql, x.tl, [&](uint32_t op) { k.push(op, 1u); });
            k.push(OP_M, x.pre);
        }
    }
    k.flush();
    const uint32_t n_body = k.n;
    const Slot &head = in.slots[0];
    uint32_t clip5 = head.q0;
    *t_start = head.t0;
    if (head.kind == K_HEAD) {
        const Res &r = in.res[0];
        clip5 = head.q0 - r.ei, *t_start = head.t0 - r.ej;
        tb_walk(in.tb + (in.tb_off[0] - in.tb_base), head.W, head.lo, r.ei, r.ej, [&](uint32_t op) { k.push(op, 1u); });
        k.flush();
    }
    const uint32_t n_head = k.n - n_body;
    k.push(OP_S, clip5);
    k.flush();
    if (a) {
        for (uint32_t x = 0, y = k.n - 1; x < y; ++x, --y) {
            const uint32_t t = a[x];
            a[x] = a[y], a[y] = t;
        }
        const uint32_t h0 = clip5 ? 1u : 0u;
        for (uint32_t x = h0, y = h0 + n_head - 1; n_head && x < y; ++x, --y) {
            const uint32_t t = a[x];
            a[x] = a[y], a[y] = t;
        }
    }
    return k.n;
}

// Pass B: the raw ops a[0 .. n) -> the final CIGAR b (room for 2 n + 2 words) and the record's pos and n_cigar (score_ops gives
// nm, as and end).  Returns the soft-clipped bases.
NP2_KC_HD uint32_t finish_ops(const Seqs &s, const uint32_t *a, uint32_t n, uint32_t t_start, const Opts &o, uint32_t *b, Rec *rec) {
    // the ends: what touches a clip joins it (I) or is dropped (D)
    uint32_t lo = 0, hi = n, clip5 = 0, clip3 = 0;
    if (lo < hi && (a[lo] & 15u) == OP_S) clip5 = a[lo++] >> 4;
    if (lo < hi && (a[hi - 1] & 15u) == OP_S) clip3 = a[--hi] >> 4;
    while (lo < hi && (a[lo] & 15u) != OP_M) {
        if ((a[lo] & 15u) == OP_I) clip5 += a[lo] >> 4;
        else t_start += a[lo] >> 4;
        ++lo;
    }
    while (lo < hi && (a[hi - 1] & 15u) != OP_M) {
        if ((a[hi - 1] & 15u) == OP_I) clip3 += a[hi - 1] >> 4;
        --hi;
    }
    uint32_t nb = 0;
    if (clip5) b[nb++] = clip5 << 4 | OP_S;
    const uint32_t first_m = nb;
    uint32_t r = t_start, q = clip5;
    auto push = [&](uint32_t op, uint32_t len) {
        if (!len) return;
        if (nb > first_m && (b[nb - 1] & 15u) == op) b[nb - 1] += len << 4;
        else b[nb++] = len << 4 | op;
    };
    for (uint32_t x = lo; x < hi; ++x) {
        const uint32_t op = a[x] & 15u, len = a[x] >> 4;
        if (op == OP_M) {
            push(op, len), r += len, q += len;
            continue;
        }
        uint32_t L = len, gr = r, gq = q, sh = 0;
        while (nb > first_m && (b[nb - 1] & 15u) == OP_M) {
            uint32_t mlen = b[nb - 1] >> 4;
            if (nb - 1 == first_m && mlen == 1) break;
            const uint32_t tcode = s.tc(gr - 1u);
            if (!eq(tcode, s.qc(gq - 1u))) break;
            if ((op == OP_D ? s.tc(gr + L - 1u) : s.qc(gq + L - 1u)) != tcode) break;
            --gr, --gq, ++sh, --mlen;
            if (mlen) {
                b[nb - 1] = mlen << 4 | OP_M;
            } else {
                --nb;
                if (nb > first_m && (b[nb - 1] & 15u) == op) { // two gaps of one kind meet
                    const uint32_t l2 = b[--nb] >> 4;
                    L += l2;
                    if (op == OP_D) gr -= l2;
                    else gq -= l2;
                }
            }
        }
        push(op, L), push(OP_M, sh);
        if (op == OP_D) r += len;
        else q += len;
    }
    if (clip3) b[nb++] = clip3 << 4 | OP_S;
    rec->pos = t_start, rec->n_cigar = nb;
    return clip5 + clip3;
}

// NM, AS and the reference end of the final CIGAR b[0 .. nb) from pos on.  The M runs' columns are dealt out to n_lanes callers
// (lane: this caller); lane 0 also counts the gaps.  The sums over all lanes are the record's; one caller (0, 1) has them whole.
NP2_KC_HD void score_ops(const Seqs &s, const uint32_t *b, uint32_t nb, uint32_t pos, const Opts &o, uint32_t lane, uint32_t n_lanes,
                         uint32_t *nm_out, int32_t *as_out, uint32_t *end_out) {
    uint32_t nm = 0, r = pos, q = 0;
    int32_t as = 0;
    for (uint32_t x = 0; x < nb; ++x) {
        const uint32_t op = b[x] & 15u, len = b[x] >> 4;
        if (op == OP_M) {
            for (uint32_t c = lane; c < len; c += n_lanes) {
                if (eq(s.tc(r + c), s.qc(q + c))) as += (int32_t)o.match;
                else as -= (int32_t)o.mismatch, ++nm;
            }
            r += len, q += len;
        } else if (op == OP_S) {
            q += len;
        } else {
            if (lane == 0) nm += len, as -= (int32_t)(o.gap_open + len * o.gap_ext);
            if (op == OP_D) r += len;
            else q += len;
        }
    }
    *nm_out = nm, *as_out = as, *end_out = r;
}

NP2_KC_HD Rec unaligned_rec() {
    Rec r{};
    r.tid = -1, r.flag = 4;
    return r;
}

} // namespace np2aln
