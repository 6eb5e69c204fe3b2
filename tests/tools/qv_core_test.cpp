// One-lane host run of the k-mer QV scan's per-lane core (csrc/np2_qv_core.hpp over csrc/np2_kcount_core.hpp): every
// sequence of a file is pushed byte by byte through np2kc::push, each hash is looked up BY BINARY SEARCH in its bucket of a
// yak v2 dump (ascending words; independent of the device's open addressing), and np2qv::tally keeps the counters.
//   qv_core_test MIN_COUNT DUMP.yak SEQS[.gz]       SEQS: FASTA (lines after a '>' line are joined) or one sequence per line
// Output: "seq <n_kmers> <n_absent>" per sequence, "hist <c> <n>" per non-empty bin, "bits <hex of the sequence's bitmap>"
// per sequence (ceil(len / 8) bytes, least significant bit first, bit e = the k-mer ending at base e is valid and absent).
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../nextpolish2_amd/csrc/np2_qv_core.hpp"

struct Dump {
    uint32_t k = 0;
    std::vector<std::vector<uint64_t>> buckets;
    bool load(const char *path) {
        FILE *f = fopen(path, "rb");
        if (!f) return false;
        char magic[4];
        uint32_t hd[3];
        bool ok = fread(magic, 1, 4, f) == 4 && memcmp(magic, "YAK\2", 4) == 0 && fread(hd, 4, 3, f) == 3 && hd[1] == np2kc::PRE &&
                  hd[2] == np2kc::COUNT_BITS;
        k = ok ? hd[0] : 0;
        buckets.resize(np2kc::N_BUCKETS);
        for (uint32_t b = 0; ok && b < np2kc::N_BUCKETS; ++b) {
            uint32_t bh[2];
            ok = fread(bh, 4, 2, f) == 2;
            if (!ok) break;
            buckets[b].resize(bh[1]);
            ok = bh[1] == 0 || fread(buckets[b].data(), 8, bh[1], f) == bh[1];
            ok = ok && std::is_sorted(buckets[b].begin(), buckets[b].end());
        }
        fclose(f);
        return ok;
    }
    // KmerInfo::get after retrieve_kmers(min_count): of the words with this key, the last one in file order that passes
    uint32_t get(uint64_t hash, uint32_t min_count) const {
        const std::vector<uint64_t> &b = buckets[np2kc::bucket_of(hash)];
        const uint64_t lo = np2kc::word_of(hash, 0);
        uint32_t c = 0;
        for (auto it = std::lower_bound(b.begin(), b.end(), lo); it != b.end() && (*it >> np2kc::COUNT_BITS) == np2kc::key_of(hash); ++it)
            if (np2qv::passing((uint32_t)(*it & np2kc::COUNT_MAX), min_count)) c = (uint32_t)(*it & np2kc::COUNT_MAX);
        return c;
    }
};

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const uint32_t min_count = (uint32_t)atoi(argv[1]);
    Dump d;
    if (!d.load(argv[2])) return 3;
    gzFile f = gzopen(argv[3], "rb");
    if (!f) return 4;
    std::string text;
    std::vector<char> buf(1 << 20);
    int got;
    while ((got = gzread(f, buf.data(), (unsigned)buf.size())) > 0) text.append(buf.data(), (size_t)got);
    if (got < 0) return 5;
    std::vector<std::string> seqs;
    bool fasta = false;
    for (size_t at = 0; at < text.size();) {
        size_t end = text.find('\n', at);
        if (end == std::string::npos) end = text.size();
        size_t n = end - at;
        while (n && text[at + n - 1] == '\r') --n;
        if (n && text[at] == '>') {
            fasta = true;
            seqs.emplace_back();
        } else if (fasta) {
            if (seqs.empty()) seqs.emplace_back();
            seqs.back().append(text, at, n);
        } else {
            seqs.emplace_back(text, at, n);
        }
        at = end + 1;
    }
    gzclose(f);

    const uint32_t k = d.k;
    const uint64_t mask = np2kc::kmer_mask(k);
    std::vector<uint64_t> hist(np2qv::QV_HIST_BINS, 0);
    std::vector<std::vector<uint8_t>> bitmaps;
    for (const std::string &s : seqs) {
        np2kc::Roll r; // no k-mer spans two sequences
        uint64_t h = 0;
        uint32_t n_kmers = 0, n_absent = 0; // (a fixture sequence is far shorter than 2^32)
        std::vector<uint8_t> bm(np2qv::bits_bytes(s.size()), 0);
        for (size_t e = 0; e < s.size(); ++e) {
            const bool valid = np2kc::push(r, (uint8_t)s[e], k, mask, &h);
            const uint32_t c = valid ? d.get(h, min_count) : 0u;
            uint32_t byte = bm[e >> 3];
            np2qv::tally(valid, c, (uint32_t)(e & 7), n_kmers, n_absent, byte);
            bm[e >> 3] = (uint8_t)byte;
            if (valid) ++hist[c];
        }
        printf("seq %u %u\n", n_kmers, n_absent);
        bitmaps.push_back(std::move(bm));
    }
    for (uint32_t c = 0; c < np2qv::QV_HIST_BINS; ++c)
        if (hist[c]) printf("hist %u %llu\n", c, (unsigned long long)hist[c]);
    for (const auto &bm : bitmaps) {
        printf("bits ");
        for (uint8_t b : bm) printf("%02x", b);
        printf("\n");
    }
    return 0;
}
