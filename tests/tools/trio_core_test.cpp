// One-lane host run of the trio scan's per-lane core (csrc/np2_trio_core.hpp over np2_qv_core.hpp and np2_kcount_core.hpp):
// every sequence of a file is pushed byte by byte through np2kc::push, each hash is looked up BY BINARY SEARCH in its
// bucket of the paternal and of the maternal yak v2 dump (ascending words; independent of the device's open addressing),
// np2trio::classify names the marker and np2trio::step keeps the counters in order.
//   trio_core_test MIN_COUNT MID_COUNT PAT.yak MAT.yak SEQS[.gz] [STRETCH]
// SEQS: FASTA (lines after a '>' line are joined) or one sequence per line.  STRETCH > 0 cuts every sequence into
// stretches of that many bases, each summed up on its own and joined to what came before through np2trio::right / join,
// as the kernel joins lanes, tiles and pieces; the answer must not depend on it.
// Output per sequence: "seq <n_kmers> <n_pat> <n_mat> <pp> <pm> <mp> <mm>", "pat <hex>" and "mat <hex>" (the marker
// bitmaps: ceil(len / 8) bytes, least significant bit first).
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../nextpolish2_amd/csrc/np2_trio_core.hpp"

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
    // the stored count: of the words with this key the last one in file order; 0 when there is none
    uint32_t get(uint64_t hash) const {
        const std::vector<uint64_t> &b = buckets[np2kc::bucket_of(hash)];
        uint32_t c = 0;
        for (auto it = std::lower_bound(b.begin(), b.end(), np2kc::word_of(hash, 0)); it != b.end() && (*it >> np2kc::COUNT_BITS) == np2kc::key_of(hash); ++it)
            c = (uint32_t)(*it & np2kc::COUNT_MAX);
        return c;
    }
};

int main(int argc, char **argv) {
    if (argc != 6 && argc != 7) return 2;
    const uint32_t min_count = (uint32_t)atoi(argv[1]), mid_count = (uint32_t)atoi(argv[2]);
    if (!np2trio::thresholds_ok(min_count, mid_count)) return 6;
    Dump pat, mat;
    if (!pat.load(argv[3]) || !mat.load(argv[4]) || pat.k != mat.k) return 3;
    const size_t stretch = argc == 7 ? (size_t)atol(argv[6]) : 0;
    gzFile f = gzopen(argv[5], "rb");
    if (!f) return 4;
    std::string text;
    std::vector<char> buf(1 << 20);
    int got;
    while ((got = gzread(f, buf.data(), (unsigned)buf.size())) > 0) text.append(buf.data(), (size_t)got);
    if (got < 0) return 5;
    gzclose(f);
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

    const uint32_t k = pat.k;
    const uint64_t mask = np2kc::kmer_mask(k);
    for (const std::string &s : seqs) {
        np2kc::Roll r; // no k-mer spans two sequences
        uint64_t h = 0;
        np2trio::Tally t; // (a fixture sequence is far shorter than 2^32)
        np2trio::Run run;
        uint32_t before = np2trio::NONE; // class of the last marker of the stretches already joined
        std::vector<uint8_t> pb(np2qv::bits_bytes(s.size()), 0), mb(pb.size(), 0);
        for (size_t e = 0; e < s.size(); ++e) {
            if (stretch && e && e % stretch == 0) { // the stretch ends: join it, start the next
                np2trio::join(t, before, run);
                before = np2trio::right(before, run.last);
                run = np2trio::Run{};
            }
            const bool valid = np2kc::push(r, (uint8_t)s[e], k, mask, &h);
            const uint32_t cls = valid ? np2trio::classify(pat.get(h), mat.get(h), min_count, mid_count) : np2trio::NONE;
            uint32_t pbyte = pb[e >> 3], mbyte = mb[e >> 3];
            np2trio::step(valid, cls, (uint32_t)(e & 7), t, run, pbyte, mbyte);
            pb[e >> 3] = (uint8_t)pbyte;
            mb[e >> 3] = (uint8_t)mbyte;
        }
        np2trio::join(t, before, run);
        printf("seq %u %u %u %u %u %u %u\n", t.n_kmers, t.n_pat, t.n_mat, t.pp, t.pm, t.mp, t.mm);
        printf("pat ");
        for (uint8_t b : pb) printf("%02x", b);
        printf("\nmat ");
        for (uint8_t b : mb) printf("%02x", b);
        printf("\n");
    }
    return 0;
}
