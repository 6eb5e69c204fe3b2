// The weighted mapper's rule (np2map::push_w of csrc/np2_map_core.hpp, through the host program of csrc/np2_map_cpu.hpp) built
// with a plain C++ compiler, for tests/test_mapw_cpu.py: with and without the address and undefined-behaviour sanitizers.
//   mapw_core_test ASM_STREAM READ_STREAM INDEX_LIST k w max_occ lookback max_gap bandwidth min_cnt min_score
// INDEX_LIST: the listed canonical indices, one decimal number a line, ascending (an empty file: the unweighted mapper).
// Prints "minimizers anchors dropped_occ index_minimizers", the index (a line "h tid end strand" per entry, in its order),
// the words of the first sequence's first 64 bytes in hexadecimal, then per read its thirteen hit fields and, on the next
// line, its primary chain's r:q pairs.
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
    if (argc != 12) {
        fprintf(stderr, "usage: mapw_core_test ASM_STREAM READ_STREAM INDEX_LIST k w max_occ lookback max_gap bandwidth min_cnt min_score\n");
        return 2;
    }
    std::vector<uint8_t> a, r, l;
    if (!slurp(argv[1], a) || !slurp(argv[2], r) || !slurp(argv[3], l)) {
        fprintf(stderr, "cannot read the inputs\n");
        return 2;
    }
    np2map::Opts o{};
    uint32_t *fields[8] = {&o.k, &o.w, &o.max_occ, &o.lookback, &o.max_gap, &o.bandwidth, &o.min_cnt, &o.min_score};
    for (int i = 0; i < 8; ++i) *fields[i] = (uint32_t)strtoul(argv[4 + i], nullptr, 10);
    bool unsupported = false;
    if (const char *bad = np2map::check_opts(o, &unsupported)) {
        fprintf(stderr, "%s: %s\n", unsupported ? "unsupported" : "argument", bad);
        return 3;
    }
    np2map::WeightSet ws;
    l.push_back(0);
    for (const char *p = (const char *)l.data(); *p;) {
        char *e = nullptr;
        const unsigned long long v = strtoull(p, &e, 10);
        if (e == p) break;
        ws.idx.push_back((uint32_t)v);
        p = *e ? e + 1 : e;
    }
    if (!ws.idx.empty()) {
        ws.k = o.k;
        if (o.k < np2map::KW_MIN || o.k > np2map::KW_MAX) {
            fprintf(stderr, "unsupported: weights are built for 11 <= k <= 15\n");
            return 3;
        }
    }
    std::vector<uint64_t> a_ends, r_ends;
    if (!np2map::stream_ends(a.data(), a.size(), a_ends) || !np2map::stream_ends(r.data(), r.size(), r_ends)) {
        fprintf(stderr, "a stream does not end in a newline\n");
        return 3;
    }
    np2map::HostIndex ix;
    ix.build(a.data(), a_ends, o.k, o.w, &ws);
    np2map::ReadCounts rc;
    std::string out;
    char line[256];
    for (const np2map::Minimizer &m : ix.mz) {
        snprintf(line, sizeof line, "%llu %u %u %u\n", (unsigned long long)m.h, (unsigned)(m.x >> 32), (unsigned)(m.x & 0xFFFFFFFFu) >> 1,
                 (unsigned)(m.x & 1u));
        out += line;
    }
    {
        np2map::Roll roll;
        const uint64_t mask = np2map::kmer_mask(o.k);
        const uint64_t n0 = a_ends.empty() ? 0 : a_ends[0];
        for (uint64_t i = 0; i < n0 && i < 64; ++i) {
            const uint64_t w = ws.empty() ? np2map::push(roll, a[i], o.k, mask)
                                          : np2map::push_w(roll, a[i], o.k, mask, [&](uint64_t v) { return ws.listed(v); });
            snprintf(line, sizeof line, "%s%llx", i ? " " : "", (unsigned long long)w);
            out += line;
        }
        out += "\n";
    }
    uint64_t from = 0;
    for (size_t i = 0; i < r_ends.size(); ++i) {
        np2map::Hit h;
        std::vector<uint32_t> chain;
        np2map::map_read(ix, r.data() + from, (uint32_t)(r_ends[i] - from), o, &h, &chain, &rc);
        from = r_ends[i] + 1;
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
