// The aligner on the CPU, one read at a time, from the rule's arithmetic in np2_align_core.hpp: what np2_map_align_host runs and
// what tests/tools/align_core_test.cpp builds with a plain C++ compiler; and the SAM text both the host and the device paths
// write.  No HIP here.
#pragma once
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

#include "np2_align_core.hpp"
#include "np2_map_cpu.hpp"

namespace np2aln {

// one slot's matrix, row by row: tb gets its cells' bits (rows x W bytes); rem: the read bases beyond the slot's start
inline Res dp_slot(const Seqs &s, const Slot &x, uint32_t rem, const Opts &o, uint8_t *tb, std::vector<int32_t> &H, std::vector<int32_t> &F) {
    const uint32_t W = x.W;
    H.assign((size_t)W + 1, NEG), F.assign((size_t)W + 1, NEG);
    for (uint32_t L = 0; L < W; ++L) {
        const int64_t j = (int64_t)x.lo + L;
        const bool in = j >= 0 && j <= (int64_t)x.tl;
        if (in) H[L] = row0_h((uint32_t)j, o);
        tb[L] = in ? (uint8_t)row0_tb((uint32_t)j) : 0;
    }
    int32_t bh = 0, eh = NEG;
    uint32_t bi = 0, bj = 0, ej = 0;
    for (uint32_t i = 1; i <= x.ql; ++i) {
        int32_t hl = NEG, el = NEG;
        const uint32_t qb = slot_q(s, x, i - 1);
        for (uint32_t L = 0; L < W; ++L) {
            const int64_t j = (int64_t)i + x.lo + L;
            int32_t h = NEG, e = NEG, f = NEG;
            uint32_t bits = 0;
            if (j >= 0 && j <= (int64_t)x.tl) {
                uint32_t ce, cf, src;
                const int32_t d = j > 0 ? H[L] + sub_score(slot_t(s, x, (uint32_t)j - 1), qb, o) : NEG;
                e = gap_of(hl, el, o, &ce), f = gap_of(H[L + 1], F[L + 1], o, &cf);
                h = h_of(d, e, f, &src);
                bits = src | ce << 2 | cf << 3;
                if (h > bh) bh = h, bi = i, bj = (uint32_t)j;
                if (i == x.ql && h > eh) eh = h, ej = (uint32_t)j;
            }
            tb[(size_t)i * W + L] = (uint8_t)bits;
            H[L] = h, F[L] = f, hl = h, el = e;
        }
    }
    if (x.kind == K_CORE) return Res{H[(uint32_t)((int32_t)x.tl - (int32_t)x.ql - x.lo)], x.ql, x.tl};
    return choose_end(bh, bi, bj, slot_has_end(x, rem), eh, ej, x.ql, o);
}

struct Scratch {
    std::vector<uint8_t> pin, tb;
    std::vector<Slot> slots;
    std::vector<Res> res;
    std::vector<uint64_t> tb_off;
    std::vector<int32_t> H, F;
    std::vector<uint32_t> a, b;
};

// what np2_align_chains_* hand back for tests (np2_io.h, np2_align_probe_t): the reads' slots, the cells their walks start from and
// the traceback bytes, in read order
struct Probe {
    bool want_tb = false;
    std::vector<uint64_t> slot_off{0}, tb_off{0};
    std::vector<Slot> slots;
    std::vector<Res> res;
    std::vector<uint8_t> tb;
    void unmapped() { slot_off.push_back(slots.size()); }
    void take(const Scratch &w, uint32_t ns) {
        const uint64_t base = tb_off.back();
        slots.insert(slots.end(), w.slots.begin(), w.slots.begin() + ns), res.insert(res.end(), w.res.begin(), w.res.begin() + ns);
        for (uint32_t i = 0; i < ns; ++i) tb_off.push_back(base + w.tb_off[i + 1]);
        if (want_tb) tb.insert(tb.end(), w.tb.begin(), w.tb.begin() + (std::ptrdiff_t)w.tb_off[ns]);
        slot_off.push_back(slots.size());
    }
};

// One mapped read (hit.tid >= 0) with its chain of hit.n pairs against contig t of tlen bases -> the record, its CIGAR appended
// to `cigar`, the counts added to c[C_N].  An overflowed read is unaligned_rec().  With a probe the read's slots, cells and bits
// are appended to it, and an overflowed read's matrices within the limits are computed as the device computes them.
inline Rec align_read(const uint8_t *t, uint32_t tlen, const uint8_t *q, const np2map::Hit &hit, const uint32_t *chain, uint32_t k, const Opts &o,
                      uint32_t max_cells, Scratch &w, std::vector<uint32_t> &cigar, uint64_t *c, Probe *probe = nullptr) {
    const Seqs s{t, tlen, q, hit.qlen, hit.rev};
    w.pin.resize(hit.n);
    const uint32_t np = mark_pins(chain, hit.n, k, w.pin.data()), ns = np + 1;
    w.slots.resize(ns), w.res.assign(ns, Res{}), w.tb_off.assign((size_t)ns + 1, 0);
    plan_read(chain, hit.n, k, w.pin.data(), tlen, hit.qlen, o, w.slots.data());
    c[C_PINS] += np, c[C_SEGMENTS] += np - 1;
    bool over = false;
    for (uint32_t i = 0; i < ns; ++i) {
        Slot &x = w.slots[i];
        const uint64_t cells = classify(s, x, o, max_cells);
        w.tb_off[i + 1] = w.tb_off[i] + cells;
        over |= x.over != 0;
        if (x.kind <= K_CORE) ++c[C_EQUAL + x.kind];
        c[C_CELLS] += cells;
    }
    if (over && !probe) {
        ++c[C_OVERFLOW];
        return unaligned_rec();
    }
    w.tb.resize(w.tb_off[ns] + 1);
    for (uint32_t i = 0; i < ns; ++i)
        if (w.tb_off[i + 1] > w.tb_off[i]) {
            const Slot &x = w.slots[i];
            const uint32_t rem = x.kind == K_HEAD ? x.q0 : x.kind == K_TAIL ? hit.qlen - x.q0 : 0;
            w.res[i] = dp_slot(s, x, rem, o, w.tb.data() + w.tb_off[i], w.H, w.F);
        }
    if (probe) probe->take(w, ns);
    if (over) {
        ++c[C_OVERFLOW];
        return unaligned_rec();
    }
    const ReadIn in{s, chain, w.pin.data(), hit.n, k, w.slots.data(), w.res.data(), w.tb_off.data(), w.tb.data(), 0, ns};
    uint32_t t_start = 0;
    const uint32_t n_raw = raw_ops(in, nullptr, &t_start);
    w.a.resize((size_t)n_raw + 1), w.b.resize(2 * (size_t)n_raw + 2);
    raw_ops(in, w.a.data(), &t_start);
    Rec rec{};
    rec.tid = hit.tid, rec.flag = hit.rev ? 16u : 0u, rec.mapq = hit.mapq;
    c[C_CLIPPED] += finish_ops(s, w.a.data(), n_raw, t_start, o, w.b.data(), &rec);
    score_ops(s, w.b.data(), rec.n_cigar, rec.pos, o, 0, 1, &rec.nm, &rec.as, &rec.end);
    cigar.insert(cigar.end(), w.b.begin(), w.b.begin() + rec.n_cigar);
    return rec;
}

// ---- SAM text ----------------------------------------------------------------------------------------------------------------
inline void sam_header(std::string &out, const std::vector<std::string> &names, const std::vector<uint64_t> &lens) {
    out += "@HD\tVN:1.6\tSO:unsorted\n";
    for (size_t i = 0; i < names.size(); ++i) out += "@SQ\tSN:" + names[i] + "\tLN:" + std::to_string(lens[i]) + "\n";
    out += "@PG\tID:nextpolish2_amd.map\tPN:nextpolish2_amd.map\n";
}

// SEQ: the read's bytes; with flag 16 reversed, ACGT complemented in their case, any other byte kept
inline void sam_seq(std::string &out, const uint8_t *q, uint32_t n, bool rev) {
    if (n == 0) {
        out += '*';
        return;
    }
    if (!rev) {
        out.append((const char *)q, n);
        return;
    }
    static const struct Comp { // ACGT complemented in their case; any other byte itself
        char t[256];
        Comp() {
            for (int i = 0; i < 256; ++i) t[i] = (char)i;
            const char *a = "ACGTacgt", *b = "TGCAtgca";
            for (int i = 0; a[i]; ++i) t[(uint8_t)a[i]] = b[i];
        }
    } comp;
    const size_t at = out.size();
    out.resize(at + n);
    char *w = &out[at];
    for (uint32_t i = 0; i < n; ++i) w[i] = comp.t[q[n - 1u - i]];
}

inline void sam_line(std::string &out, const char *qname, size_t qname_n, const Rec &rec, const np2map::Hit &hit, const uint32_t *cigar,
                     const uint8_t *q, uint32_t qlen, const std::string *tname) {
    char num[160];
    out.append(qname, qname_n);
    if (rec.tid < 0) {
        out += "\t4\t*\t0\t0\t*\t*\t0\t0\t";
        sam_seq(out, q, qlen, false);
        out += "\t*\n";
        return;
    }
    int m = snprintf(num, sizeof num, "\t%u\t", rec.flag);
    out.append(num, (size_t)m);
    out += *tname;
    m = snprintf(num, sizeof num, "\t%u\t%u\t", rec.pos + 1, rec.mapq);
    out.append(num, (size_t)m);
    for (uint32_t i = 0; i < rec.n_cigar; ++i) {
        m = snprintf(num, sizeof num, "%u%c", cigar[i] >> 4, "MIDNS"[cigar[i] & 15u]);
        out.append(num, (size_t)m);
    }
    out += "\t*\t0\t0\t";
    sam_seq(out, q, qlen, (rec.flag & 16u) != 0);
    m = snprintf(num, sizeof num, "\t*\tNM:i:%u\tAS:i:%d\tcm:i:%u\ts1:i:%u\ts2:i:%u\n", rec.nm, rec.as, hit.n, hit.s1, hit.s2);
    out.append(num, (size_t)m);
}

// what the opt-in outputs add to a line (np2_map_align_files_x): QUAL (null: *), and MD:Z: then cs:Z: behind s2:i: (0 bytes: none)
struct SamExtra {
    const uint8_t *qual;
    const char *md, *cs;
    uint32_t n_md, n_cs;
    // More chains (np2_io.h): bits added to FLAG (2048 supplementary, 256 secondary) and SA:Z:'s value (null: none), the last field
    uint32_t flag_or;
    const std::string *sa;
};

// One entry of SA:Z: for a record: rname,pos,strand,CIGAR,mapq,NM; with the CIGAR in M / I / D / S form whatever the record's own
// is (= and X runs are joined into M again)
inline void sa_entry(std::string &out, const Rec &rec, const uint32_t *cigar, const std::string &tname) {
    char num[64];
    out += tname;
    int m = snprintf(num, sizeof num, ",%u,%c,", rec.pos + 1, (rec.flag & 16u) ? '-' : '+');
    out.append(num, (size_t)m);
    for (uint32_t i = 0; i < rec.n_cigar;) {
        uint32_t op = cigar[i] & 15u, len = cigar[i] >> 4;
        if (op == 7u || op == 8u) op = 0u;
        for (++i; i < rec.n_cigar && op == 0u && ((cigar[i] & 15u) == 7u || (cigar[i] & 15u) == 8u || (cigar[i] & 15u) == 0u); ++i) len += cigar[i] >> 4;
        m = snprintf(num, sizeof num, "%u%c", len, "MIDNS"[op]);
        out.append(num, (size_t)m);
    }
    m = snprintf(num, sizeof num, ",%u,%u;", rec.mapq, rec.nm);
    out.append(num, (size_t)m);
}
// sam_line with them: the CIGAR may hold = and X words; QUAL is reversed, not complemented, with flag 16, and written forward
// for an unmapped or overflowed read
inline void sam_line_x(std::string &out, const char *qname, size_t qname_n, const Rec &rec, const np2map::Hit &hit, const uint32_t *cigar,
                       const uint8_t *q, uint32_t qlen, const std::string *tname, const SamExtra &x) {
    char num[160];
    const auto put_qual = [&](bool rev) {
        if (!x.qual || qlen == 0) {
            out += '*';
            return;
        }
        if (!rev) {
            out.append((const char *)x.qual, qlen);
            return;
        }
        const size_t at = out.size();
        out.resize(at + qlen);
        char *w = &out[at];
        for (uint32_t i = 0; i < qlen; ++i) w[i] = (char)x.qual[qlen - 1u - i];
    };
    out.append(qname, qname_n);
    if (rec.tid < 0) {
        out += "\t4\t*\t0\t0\t*\t*\t0\t0\t";
        sam_seq(out, q, qlen, false);
        out += '\t';
        put_qual(false);
        out += '\n';
        return;
    }
    int m = snprintf(num, sizeof num, "\t%u\t", rec.flag | x.flag_or);
    out.append(num, (size_t)m);
    out += *tname;
    m = snprintf(num, sizeof num, "\t%u\t%u\t", rec.pos + 1, rec.mapq);
    out.append(num, (size_t)m);
    for (uint32_t i = 0; i < rec.n_cigar; ++i) {
        m = snprintf(num, sizeof num, "%u%c", cigar[i] >> 4, "MIDNSHP=X"[cigar[i] & 15u]);
        out.append(num, (size_t)m);
    }
    out += "\t*\t0\t0\t";
    sam_seq(out, q, qlen, (rec.flag & 16u) != 0);
    out += '\t';
    put_qual((rec.flag & 16u) != 0);
    m = snprintf(num, sizeof num, "\tNM:i:%u\tAS:i:%d\tcm:i:%u\ts1:i:%u\ts2:i:%u", rec.nm, rec.as, hit.n, hit.s1, hit.s2);
    out.append(num, (size_t)m);
    if (x.n_md) out += "\tMD:Z:", out.append(x.md, x.n_md);
    if (x.n_cs) out += "\tcs:Z:", out.append(x.cs, x.n_cs);
    if (x.sa) out += "\tSA:Z:", out += *x.sa;
    out += '\n';
}

} // namespace np2aln
