// One lane of the repetitive k-mer list on the host: csrc/np2_rep_core.hpp (the text the count kernel and the host driver
// run) over a separator stream in a file, counters in a std::map.
//   rep_core_test STREAM K distinct F | min_count N
// prints "kmers distinct threshold listed listed_occurrences max_count" on the first line, then "INDEX\tCOUNT\tKMER" per
// listed index in ascending order.  With `distinct` the threshold is taken twice, over the (count, occurrences) list in
// one go and the way the driver does it (high halves, then low halves inside the chosen bin); they must agree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../nextpolish2_amd/csrc/np2_rep_core.hpp"

int main(int argc, char **argv) {
    if (argc != 5) return fprintf(stderr, "usage: rep_core_test STREAM K distinct F | min_count N\n"), 2;
    const uint32_t k = (uint32_t)atoi(argv[2]);
    if (k < np2rep::K_MIN || k > np2rep::K_MAX) return fprintf(stderr, "k out of range\n"), 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    std::map<uint32_t, uint64_t> count;
    np2kc::Roll r;
    const uint64_t mask = np2kc::kmer_mask(k);
    uint64_t kmers = 0;
    uint32_t v = 0;
    for (int ch; (ch = fgetc(f)) != EOF;)
        if (np2rep::push(r, (uint8_t)ch, k, mask, &v)) ++count[v], ++kmers;
    fclose(f);

    std::map<uint32_t, uint64_t> occ_of; // count value -> indices that have it
    uint32_t max_count = 0;
    for (auto &c : count) ++occ_of[(uint32_t)c.second], max_count = c.second > max_count ? (uint32_t)c.second : max_count;
    uint32_t threshold = 0;
    if (!strcmp(argv[3], "min_count")) {
        threshold = (uint32_t)strtoul(argv[4], nullptr, 10);
    } else {
        const double fr = atof(argv[4]);
        std::vector<uint32_t> values;
        std::vector<uint64_t> occ;
        for (auto &o : occ_of) values.push_back(o.first), occ.push_back(o.second);
        threshold = np2rep::threshold_of(values.data(), occ.data(), values.size(), fr);
        if (!count.empty()) { // the driver's two levels
            std::vector<uint64_t> hi(1u << 16, 0), lo(1u << 16, 0);
            for (auto &o : occ_of) hi[o.first >> 16] += o.second;
            uint64_t before = 0, before_lo = 0;
            const uint64_t target = np2rep::target_of(fr, count.size());
            const uint64_t bin = np2rep::select_entry(hi.data(), hi.size(), target, &before);
            for (auto &o : occ_of)
                if ((o.first >> 16) == bin) lo[o.first & 0xFFFFu] += o.second;
            const uint64_t l = np2rep::select_entry(lo.data(), lo.size(), target - before, &before_lo);
            if (bin >= hi.size() || l >= lo.size() || (uint32_t)(bin << 16 | l) != threshold)
                return fprintf(stderr, "two-level selection %llu:%llu disagrees with threshold %u\n", (unsigned long long)bin,
                               (unsigned long long)l, threshold), 1;
        }
    }
    uint64_t listed = 0, listed_occ = 0;
    for (auto &c : count)
        if (c.second > threshold) ++listed, listed_occ += c.second;
    printf("%llu %llu %u %llu %llu %u\n", (unsigned long long)kmers, (unsigned long long)count.size(), threshold,
           (unsigned long long)listed, (unsigned long long)listed_occ, max_count);
    char text[np2rep::K_MAX + 1];
    for (auto &c : count) {
        if (c.second <= threshold) continue;
        np2rep::index_text(c.first, k, text);
        text[k] = 0;
        printf("%u\t%llu\t%s\n", c.first, (unsigned long long)c.second, text);
    }
    return 0;
}
