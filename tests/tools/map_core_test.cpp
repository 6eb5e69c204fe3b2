// The mapper's rule (csrc/np2_map_core.hpp, through the one-read-at-a-time host program of csrc/np2_map_cpu.hpp) built with a
// plain C++ compiler, for tests/test_map_cpu.py: with and without the address and undefined-behaviour sanitizers.
//   map_core_test ASM_STREAM READ_STREAM k w max_occ lookback max_gap bandwidth min_cnt min_score
// prints "minimizers anchors dropped_occ index_minimizers", then per read its thirteen hit fields and, on the next line, its
// primary chain's r:q pairs.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../nextpolish2_amd/csrc/np2_map_cpu.hpp"

static bool slurp(const char *path, std::vector<uint8_t> &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return true;
}

int main(int argc, char **argv) {
    if (argc != 11) {
        fprintf(stderr, "usage: map_core_test ASM_STREAM READ_STREAM k w max_occ lookback max_gap bandwidth min_cnt min_score\n");
        return 2;
    }
    std::vector<uint8_t> a, r;
    if (!slurp(argv[1], a) || !slurp(argv[2], r)) {
        fprintf(stderr, "cannot read the streams\n");
        return 2;
    }
    np2map::Opts o{};
    uint32_t *fields[8] = {&o.k, &o.w, &o.max_occ, &o.lookback, &o.max_gap, &o.bandwidth, &o.min_cnt, &o.min_score};
    for (int i = 0; i < 8; ++i) *fields[i] = (uint32_t)strtoul(argv[3 + i], nullptr, 10);
    bool unsupported = false;
    if (const char *bad = np2map::check_opts(o, &unsupported)) {
        fprintf(stderr, "%s: %s\n", unsupported ? "unsupported" : "argument", bad);
        return 3;
    }
    std::vector<uint64_t> a_ends, r_ends;
    if (!np2map::stream_ends(a.data(), a.size(), a_ends) || !np2map::stream_ends(r.data(), r.size(), r_ends)) {
        fprintf(stderr, "a stream does not end in a newline\n");
        return 3;
    }
    np2map::HostIndex ix;
    ix.build(a.data(), a_ends, o.k, o.w);
    np2map::ReadCounts rc;
    std::string out;
    uint64_t from = 0;
    for (size_t i = 0; i < r_ends.size(); ++i) {
        np2map::Hit h;
        std::vector<uint32_t> chain;
        np2map::map_read(ix, r.data() + from, (uint32_t)(r_ends[i] - from), o, &h, &chain, &rc);
        from = r_ends[i] + 1;
        char line[256];
        snprintf(line, sizeof line, "%d %u %u %u %u %u %u %u %u %u %u %u %u\n", h.tid, h.qlen, h.qs, h.qe, h.rev, h.ts, h.te, h.matches, h.block,
                 h.mapq, h.n, h.s1, h.s2);
        out += line;
        for (size_t t = 0; t + 1 < chain.size(); t += 2) out += (t ? " " : "") + std::to_string(chain[t]) + ":" + std::to_string(chain[t + 1]);
        out += "\n";
    }
    printf("%llu %llu %llu %llu\n", (unsigned long long)rc.minimizers, (unsigned long long)rc.anchors, (unsigned long long)rc.dropped_occ,
           (unsigned long long)ix.mz.size());
    fputs(out.c_str(), stdout);
    return 0;
}
