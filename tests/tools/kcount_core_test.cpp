// One-lane host run of the k-mer counter's per-lane core (csrc/np2_kcount_core.hpp): a separator stream is pushed byte by
// byte through np2kc::push, the hashes are counted in a std::unordered_map, and the table is written as a yak v2 dump
// (bucket-major, ascending words inside a bucket, counts saturated at 1023, words below min_count left out).
//   kcount_core_test K MIN_COUNT OUT.yak STREAM[.gz]...      (the streams are read one after the other through zlib)
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <unordered_map>
#include <vector>

#include "../../nextpolish2_amd/csrc/np2_kcount_core.hpp"

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const uint32_t k = (uint32_t)atoi(argv[1]), min_count = (uint32_t)atoi(argv[2]);
    const uint64_t mask = np2kc::kmer_mask(k);
    std::unordered_map<uint64_t, uint32_t> counts;
    std::vector<uint8_t> buf(1 << 20);
    for (int a = 4; a < argc; ++a) {
        gzFile f = gzopen(argv[a], "rb");
        if (!f) return 3;
        np2kc::Roll r; // (a new file starts a new run: every stream ends with its separator anyway)
        uint64_t h = 0;
        int got;
        while ((got = gzread(f, buf.data(), (unsigned)buf.size())) > 0)
            for (int i = 0; i < got; ++i)
                if (np2kc::push(r, buf[i], k, mask, &h)) {
                    uint32_t &c = counts[h];
                    c = np2kc::sat_add(c, 1);
                }
        gzclose(f);
        if (got < 0) return 4;
    }
    std::vector<std::vector<uint64_t>> buckets(np2kc::N_BUCKETS);
    for (const auto &kv : counts)
        if (kv.second >= min_count) buckets[np2kc::bucket_of(kv.first)].push_back(np2kc::word_of(kv.first, kv.second));
    FILE *o = fopen(argv[3], "wb");
    if (!o) return 5;
    const uint32_t hd[3] = {k, np2kc::PRE, np2kc::COUNT_BITS};
    fwrite("YAK\2", 1, 4, o);
    fwrite(hd, 4, 3, o);
    for (auto &b : buckets) {
        std::sort(b.begin(), b.end());
        const uint32_t bh[2] = {0u, (uint32_t)b.size()};
        fwrite(bh, 4, 2, o);
        if (!b.empty()) fwrite(b.data(), 8, b.size(), o);
    }
    return fclose(o) == 0 ? 0 : 6;
}
