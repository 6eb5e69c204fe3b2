// More chains (np2_io.h, "More chains"): the units of a call or of a batch on the host, how a batch's aligned units are settled,
// and a read's SAM lines from them.  What the _m doors of np2_map_host.cpp hold and write, and what
// tests/tools/mapmulti_core_test.cpp builds with a plain C++ compiler.  No HIP here.
#pragma once
#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include "np2_align_cpu.hpp"

namespace np2aln {

// the MD and cs texts of a batch's reads: appended in read order, n_md[i], n_cs[i] bytes of read i (0: none)
struct TagTexts {
    std::vector<char> md, cs;
    std::vector<uint32_t> n_md, n_cs;
    void begin(size_t n_reads) { md.clear(), cs.clear(), n_md.assign(n_reads, 0), n_cs.assign(n_reads, 0); }
};

// the units in read order and, inside a read, the primary first and the kept further chains in selection order
struct Units {
    std::vector<np2map::Hit> hits;
    std::vector<uint8_t> cls;
    std::vector<uint32_t> parent, n_units; // n_units: per read
    std::vector<uint32_t> chain;           // the units' (r, q) pairs, when asked for
    // with the aligner on: a record per unit, the units' CIGAR words in order, and their MD / cs texts
    std::vector<Rec> recs;
    std::vector<uint32_t> cigar;
    TagTexts tt;
    void clear() {
        hits.clear(), cls.clear(), parent.clear(), n_units.clear(), chain.clear(), recs.clear(), cigar.clear();
        tt.md.clear(), tt.cs.clear(), tt.n_md.clear(), tt.n_cs.clear();
    }
    // The aligned units of a batch, settled (np2_io.h, "More chains", Alignment): a read whose primary is unmapped or
    // overflowed keeps its primary alone; a further unit that overflowed is dropped, and so is a secondary whose parent was.
    // Parents are renumbered.  Returns the further units dropped.
    uint64_t settle() {
        const bool tags = !tt.n_md.empty();
        Units out;
        size_t at = 0, cg = 0, md = 0, cs = 0;
        uint64_t dropped = 0;
        uint32_t place[np2map::MAX_CHAINS];
        for (uint32_t n : n_units) {
            uint32_t kept = 0;
            for (uint32_t u = 0; u < n; ++u, ++at) {
                const Rec &rc = recs[at];
                const uint32_t nmd = tags ? tt.n_md[at] : 0, ncs = tags ? tt.n_cs[at] : 0;
                bool keep = u == 0;
                if (u > 0 && place[0] != np2map::NO_UNIT && rc.tid >= 0)
                    keep = cls[at] != np2map::CLS_SEC || place[parent[at]] != np2map::NO_UNIT;
                if (u == 0) place[0] = rc.tid >= 0 ? 0u : np2map::NO_UNIT; // (kept either way; NO_UNIT: nothing else of the read is)
                else place[u] = keep ? kept : np2map::NO_UNIT;
                if (keep) {
                    out.hits.push_back(hits[at]), out.cls.push_back(cls[at]), out.recs.push_back(rc);
                    out.parent.push_back(u == 0 ? 0u : cls[at] == np2map::CLS_SEC ? place[parent[at]] : kept);
                    out.cigar.insert(out.cigar.end(), cigar.begin() + (ptrdiff_t)cg, cigar.begin() + (ptrdiff_t)(cg + rc.n_cigar));
                    if (tags) {
                        out.tt.n_md.push_back(nmd), out.tt.n_cs.push_back(ncs);
                        out.tt.md.insert(out.tt.md.end(), tt.md.begin() + (ptrdiff_t)md, tt.md.begin() + (ptrdiff_t)(md + nmd));
                        out.tt.cs.insert(out.tt.cs.end(), tt.cs.begin() + (ptrdiff_t)cs, tt.cs.begin() + (ptrdiff_t)(cs + ncs));
                    }
                    ++kept;
                } else {
                    ++dropped;
                }
                cg += rc.n_cigar, md += nmd, cs += ncs;
            }
            out.n_units.push_back(kept);
        }
        *this = std::move(out);
        return dropped;
    }
    // with max_chains = 1: every read is its primary
    void add_plain(const np2map::Hit *h, size_t n) {
        hits.insert(hits.end(), h, h + n), cls.insert(cls.end(), n, (uint8_t)np2map::CLS_PRIMARY);
        parent.insert(parent.end(), n, 0u), n_units.insert(n_units.end(), n, 1u);
    }
};

// where a read's settled units start in the arrays of a Units: advanced by sam_units_of_read
struct UnitAt {
    size_t unit = 0, cigar = 0, md = 0, cs = 0;
};

// One read's SAM lines from its n settled units at `at`: the records are adjacent, the primary first; FLAG gains 2048 / 256;
// when the read has two or more aligned parent-class records each of them ends in SA:Z: naming the others in unit order.
// q, qual: the read's bytes and qualities (null: *); tags: the units carry MD / cs texts.
inline void sam_units_of_read(std::string &text, const char *qname, size_t qname_n, const uint8_t *q, uint32_t qlen, const uint8_t *qual, const Units &u,
                              uint32_t n, bool tags, const std::vector<std::string> &tnames, UnitAt &at) {
    std::string sa[np2map::MAX_CHAINS];
    size_t cig_of[np2map::MAX_CHAINS];
    uint32_t n_par = 0;
    size_t c = at.cigar;
    for (uint32_t t = 0; t < n; ++t) {
        cig_of[t] = c, c += u.recs[at.unit + t].n_cigar;
        if (u.cls[at.unit + t] != np2map::CLS_SEC && u.recs[at.unit + t].tid >= 0) ++n_par;
    }
    for (uint32_t t = 0; t < n; ++t) {
        if (n_par < 2 || u.cls[at.unit + t] == np2map::CLS_SEC) continue;
        for (uint32_t v = 0; v < n; ++v)
            if (v != t && u.cls[at.unit + v] != np2map::CLS_SEC)
                sa_entry(sa[t], u.recs[at.unit + v], u.cigar.data() + cig_of[v], tnames[(size_t)u.recs[at.unit + v].tid]);
    }
    for (uint32_t t = 0; t < n; ++t) {
        const Rec &rc = u.recs[at.unit + t];
        SamExtra x{};
        x.qual = qual;
        if (tags) x.md = u.tt.md.data() + at.md, x.n_md = u.tt.n_md[at.unit + t], x.cs = u.tt.cs.data() + at.cs, x.n_cs = u.tt.n_cs[at.unit + t];
        x.flag_or = u.cls[at.unit + t] == np2map::CLS_SUPP ? 2048u : u.cls[at.unit + t] == np2map::CLS_SEC ? 256u : 0u;
        if (!sa[t].empty()) x.sa = &sa[t];
        sam_line_x(text, qname, qname_n, rc, u.hits[at.unit + t], u.cigar.data() + cig_of[t], q, qlen, rc.tid >= 0 ? &tnames[(size_t)rc.tid] : nullptr, x);
        at.md += x.n_md, at.cs += x.n_cs;
    }
    at.unit += n, at.cigar = c;
}

} // namespace np2aln
