// The tag walk (csrc/np2_aligntags_core.hpp) built with a plain C++ compiler, for tests/test_aligntags_cpu.py: with and without
// the address and undefined-behaviour sanitizers.
//   aligntags_core_test RECORDS n_lanes
// RECORDS holds three lines per record: the reference from pos on and the read as aligned, both in hex, and the CIGAR text (*:
// none).  Prints per record its MD, its cs and its split CIGAR (* when empty), one line each.
// n_lanes callers walk a record as the kernels' lanes do.  The walk asks for one ballot per step of n_lanes columns whatever the
// masks are, so a first round (every caller alone, ballots answered with 0) records what each caller would vote, the votes are
// or-ed into the masks, and then every caller walks twice more with those masks: to size, and to write into buffers of exactly
// that size, lane 0 its digits and all callers the letters they are dealt.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../nextpolish2_amd/csrc/np2_aligntags_core.hpp"

using namespace np2aln;

static std::vector<uint8_t> unhex(const std::string &s) {
    std::vector<uint8_t> out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

static std::string cigar_text(const std::vector<uint32_t> &w) {
    std::string s;
    for (uint32_t v : w) s += std::to_string(v >> 4) + "MIDNSHP=X"[v & 15u];
    return w.empty() ? "*" : s;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const uint32_t n_lanes = (uint32_t)strtoul(argv[2], nullptr, 10);
    if (n_lanes < 1 || n_lanes > 64) return 2;
    std::ifstream f(argv[1]);
    std::string lt, lq, lc;
    while (std::getline(f, lt) && std::getline(f, lq) && std::getline(f, lc)) {
        const std::vector<uint8_t> t = unhex(lt), q = unhex(lq);
        std::vector<uint32_t> cigar;
        if (lc != "*")
            for (const char *p = lc.c_str(); *p;) {
                char *e;
                const uint32_t len = (uint32_t)strtoul(p, &e, 10);
                const char *op = strchr("MIDNS", *e);
                if (!op || !*e) return 2;
                cigar.push_back(len << 4 | (uint32_t)(op - "MIDNS"));
                p = e + 1;
            }
        uint64_t ts = 0, qs = 0;
        if (!tag_cigar_spans(cigar.data(), cigar.size(), &ts, &qs) || ts > t.size() || qs > q.size()) return 3;
        // exact copies, so that a byte read beyond a record's columns is the sanitizer's
        std::vector<uint8_t> tc(t.begin(), t.begin() + (ptrdiff_t)ts), qc(q.begin(), q.begin() + (ptrdiff_t)qs);
        const TagIn in{tc.data(), qc.data(), (uint32_t)qc.size(), 0, cigar.data(), (uint32_t)cigar.size()};
        std::vector<uint64_t> masks;
        for (uint32_t lane = 0; lane < n_lanes; ++lane) {
            size_t k = 0;
            TagOut o{};
            tag_walk(in, o, lane, n_lanes, [&](bool b) {
                if (k == masks.size()) masks.push_back(0);
                masks[k++] |= (uint64_t)(b ? 1u : 0u) << lane;
                return (uint64_t)0;
            });
            if (k != masks.size()) return 4;
        }
        TagOut size{};
        for (uint32_t lane = 0; lane < n_lanes; ++lane) {
            size_t k = 0;
            TagOut o{};
            tag_walk(in, o, lane, n_lanes, [&](bool) { return masks[k++]; });
            if (lane && (o.n_md != size.n_md || o.n_cs != size.n_cs || o.n_eqx != size.n_eqx)) return 5; // (every caller has the state whole)
            size = o;
        }
        std::vector<char> md(size.n_md, '?'), cs(size.n_cs, '?');
        std::vector<uint32_t> eqx(size.n_eqx, 0xFFFFFFFFu);
        for (uint32_t lane = 0; lane < n_lanes; ++lane) {
            size_t k = 0;
            TagOut o{};
            o.md = md.data(), o.cs = cs.data(), o.eqx = eqx.data();
            tag_walk(in, o, lane, n_lanes, [&](bool) { return masks[k++]; });
            if (o.n_md != size.n_md || o.n_cs != size.n_cs || o.n_eqx != size.n_eqx) return 6; // size and emit agree
        }
        puts(std::string(md.begin(), md.end()).c_str()); // (the texts hold no NUL)
        puts(std::string(cs.begin(), cs.end()).c_str());
        puts(cigar_text(eqx).c_str());
    }
    return 0;
}
