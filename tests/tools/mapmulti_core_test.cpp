// The rule for more chains per read (csrc/np2_map_core.hpp: select_more and what it is made of, through the host program of
// csrc/np2_map_cpu.hpp) built with a plain C++ compiler, for tests/test_mapmulti_cpu.py: with the address and
// undefined-behaviour sanitizers.
//   mapmulti_core_test ASM_STREAM READ_STREAM k w max_occ lookback max_gap bandwidth min_cnt min_score
//                      max_chains supplementary secondary_n mask_pm pri_pm
// prints "selections dropped_min_cnt dropped_secondary kept_supplementary kept_secondary", then per read its unit count and
// per unit "cls parent" with the thirteen hit fields and, on the next line, the unit's chain as r:q pairs.
//   mapmulti_core_test ... pri_pm sam MAX_CELLS
// aligns every unit as np2_map_align_host_m does (the aligner's default options but for max_cells), settles the units
// (csrc/np2_map_units.hpp) and prints "further units dropped", then the SAM lines of reads r1, r2, ... on contigs ctg1, ctg2, ...
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <cstring>

#include "../../nextpolish2_amd/csrc/np2_map_units.hpp"

static bool slurp(const char *path, std::vector<uint8_t> &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return true;
}

// SA:Z: joins = and X runs into M again, whatever lies between them
static bool sa_joins_eqx() {
    const uint32_t cg[] = {5u << 4 | 4u, 10u << 4 | 7u, 1u << 4 | 8u, 4u << 4 | 7u, 2u << 4 | 1u, 3u << 4 | 7u, 1u << 4 | 2u, 7u << 4 | 8u, 6u << 4 | 4u};
    np2aln::Rec rec{};
    rec.tid = 0, rec.flag = 16u, rec.pos = 41u, rec.mapq = 60u, rec.nm = 11u, rec.n_cigar = 9u;
    std::string out;
    np2aln::sa_entry(out, rec, cg, "ctg1");
    return out == "ctg1,42,-,5S15M2I3M1D7M6S,60,11;";
}

int main(int argc, char **argv) {
    const bool sam = argc == 18 && !strcmp(argv[16], "sam");
    if (argc != 16 && !sam) {
        fprintf(stderr, "usage: mapmulti_core_test ASM_STREAM READ_STREAM k w max_occ lookback max_gap bandwidth min_cnt min_score "
                        "max_chains supplementary secondary_n mask_pm pri_pm\n");
        return 2;
    }
    std::vector<uint8_t> a, r;
    if (!slurp(argv[1], a) || !slurp(argv[2], r)) {
        fprintf(stderr, "cannot read the streams\n");
        return 2;
    }
    np2map::Opts o{};
    np2map::MultiOpts m{};
    uint32_t *fields[13] = {&o.k, &o.w, &o.max_occ, &o.lookback, &o.max_gap, &o.bandwidth, &o.min_cnt, &o.min_score,
                            &m.max_chains, &m.supplementary, &m.secondary_n, &m.mask_pm, &m.pri_pm};
    for (int i = 0; i < 13; ++i) *fields[i] = (uint32_t)strtoul(argv[3 + i], nullptr, 10);
    bool unsupported = false;
    if (const char *bad = np2map::check_opts(o, &unsupported)) {
        fprintf(stderr, "%s: %s\n", unsupported ? "unsupported" : "argument", bad);
        return 3;
    }
    if (const char *bad = np2map::check_multi(m)) {
        fprintf(stderr, "argument: %s\n", bad);
        return 3;
    }
    std::vector<uint64_t> a_ends, r_ends;
    if (!np2map::stream_ends(a.data(), a.size(), a_ends) || !np2map::stream_ends(r.data(), r.size(), r_ends)) {
        fprintf(stderr, "a stream does not end in a newline\n");
        return 3;
    }
    np2map::HostIndex ix;
    ix.build(a.data(), a_ends, o.k, o.w);
    if (sam) {
        if (!sa_joins_eqx()) {
            fprintf(stderr, "sa_entry does not join = and X into M\n");
            return 4;
        }
        np2aln::Opts ao{1, 4, 6, 2, 32, 5, 2048, (uint32_t)strtoul(argv[17], nullptr, 10)};
        if (const char *bad = np2aln::check_opts(ao)) {
            fprintf(stderr, "argument: %s\n", bad);
            return 3;
        }
        np2aln::Units u;
        np2aln::Scratch w;
        std::vector<uint32_t> ch;
        np2map::ReadCounts counts;
        np2map::MoreCounts more{};
        uint64_t from = 0;
        for (size_t i = 0; i < r_ends.size(); ++i) { // np2_map_align_host_m's loop, without tags
            np2map::Hit uh[np2map::MAX_CHAINS];
            uint32_t ucls[np2map::MAX_CHAINS], upar[np2map::MAX_CHAINS];
            ch.clear();
            const uint32_t nu = np2map::map_read_m(ix, r.data() + from, (uint32_t)(r_ends[i] - from), o, m, uh, ucls, upar, &ch, &counts, &more);
            u.n_units.push_back(nu);
            size_t ch_at = 0;
            for (uint32_t t = 0; t < nu; ++t) {
                const np2map::Hit &h = uh[t];
                u.hits.push_back(h), u.cls.push_back((uint8_t)ucls[t]), u.parent.push_back(upar[t]);
                u.recs.push_back(np2aln::unaligned_rec());
                if (h.tid < 0) continue;
                const uint64_t t_at = h.tid ? a_ends[(size_t)h.tid - 1] + 1 : 0;
                uint64_t c64[np2aln::C_N] = {};
                u.recs.back() = np2aln::align_read(a.data() + t_at, (uint32_t)(a_ends[(size_t)h.tid] - t_at), r.data() + from, h, ch.data() + ch_at, o.k, ao,
                                                   ao.max_cells, w, u.cigar, c64);
                ch_at += 2 * (size_t)h.n;
            }
            from = r_ends[i] + 1;
        }
        const uint64_t dropped = u.settle();
        std::vector<std::string> tnames;
        for (size_t i = 0; i < a_ends.size(); ++i) tnames.push_back("ctg" + std::to_string(i + 1));
        std::string text;
        np2aln::UnitAt at;
        from = 0;
        for (size_t i = 0; i < r_ends.size(); ++i) {
            const std::string qname = "r" + std::to_string(i + 1);
            np2aln::sam_units_of_read(text, qname.data(), qname.size(), r.data() + from, (uint32_t)(r_ends[i] - from), nullptr, u, u.n_units[i], false, tnames, at);
            from = r_ends[i] + 1;
        }
        printf("%llu\n", (unsigned long long)dropped);
        fputs(text.c_str(), stdout);
        return 0;
    }
    np2map::ReadCounts rc;
    np2map::MoreCounts mc{};
    std::string out;
    uint64_t from = 0;
    for (size_t i = 0; i < r_ends.size(); ++i) {
        np2map::Hit hits[np2map::MAX_CHAINS];
        uint32_t cls[np2map::MAX_CHAINS], parent[np2map::MAX_CHAINS];
        std::vector<uint32_t> chain;
        const uint32_t n = np2map::map_read_m(ix, r.data() + from, (uint32_t)(r_ends[i] - from), o, m, hits, cls, parent, &chain, &rc, &mc);
        from = r_ends[i] + 1;
        out += std::to_string(n) + "\n";
        size_t at = 0;
        for (uint32_t u = 0; u < n; ++u) {
            const np2map::Hit &h = hits[u];
            char line[320];
            snprintf(line, sizeof line, "%u %u %d %u %u %u %u %u %u %u %u %u %u %u %u\n", cls[u], parent[u], h.tid, h.qlen, h.qs, h.qe, h.rev, h.ts, h.te,
                     h.matches, h.block, h.mapq, h.n, h.s1, h.s2);
            out += line;
            const size_t pairs = h.tid >= 0 ? h.n : 0;
            for (size_t t = 0; t < pairs; ++t) out += (t ? " " : "") + std::to_string(chain[at + 2 * t]) + ":" + std::to_string(chain[at + 2 * t + 1]);
            at += 2 * pairs;
            out += "\n";
        }
    }
    printf("%u %u %u %u %u\n", mc.selections, mc.dropped_cnt, mc.dropped_pri, mc.kept_supp, mc.kept_sec);
    fputs(out.c_str(), stdout);
    return 0;
}
