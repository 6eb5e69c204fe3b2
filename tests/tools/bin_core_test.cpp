// One-lane host run of the read binner's per-lane core (csrc/np2_bin_core.hpp over np2_trio_core.hpp): a PACKED separator
// stream (raw bytes, every read followed by one '\n') is cut into stretches of STRETCH bytes wherever they fall, each
// stretch is walked on its own with np2bin::walk (its k-mer run warmed up from the 32 bytes in front of it, as a lane's is
// from the halo), and the stretches are joined by the segmented exclusive scan under np2trio::seg_right, as the kernel
// joins lanes, tiles and pieces.  Hashes are looked up BY BINARY SEARCH in the two yak v2 dumps.
//   bin_core_test MIN_COUNT MID_COUNT MIN_SCORE MINOR_PERMILLE PAT.yak MAT.yak STREAM STRETCH     (STRETCH 0: one stretch)
//   bin_core_test class S_PAT S_MAT MIN_SCORE MINOR_PERMILLE
// Output per read: "read <n_kmers> <n_pat> <n_mat> <pp> <pm> <mp> <mm> <class>"; the second form prints the class byte.
// Exit 6: thresholds or minor_permille outside the rule; 7: the stream does not end in '\n'.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../nextpolish2_amd/csrc/np2_bin_core.hpp"

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
    if (argc == 6 && strcmp(argv[1], "class") == 0) {
        const uint32_t permille = (uint32_t)atol(argv[5]);
        if (!np2bin::opts_ok(permille)) return 6;
        printf("%c\n", (char)np2bin::read_class((uint32_t)atol(argv[2]), (uint32_t)atol(argv[3]), (uint32_t)atol(argv[4]), permille));
        return 0;
    }
    if (argc != 9) return 2;
    const uint32_t min_count = (uint32_t)atoi(argv[1]), mid_count = (uint32_t)atoi(argv[2]);
    const uint32_t min_score = (uint32_t)atol(argv[3]), permille = (uint32_t)atol(argv[4]);
    if (!np2trio::thresholds_ok(min_count, mid_count) || !np2bin::opts_ok(permille)) return 6;
    Dump pat, mat;
    if (!pat.load(argv[5]) || !mat.load(argv[6]) || pat.k != mat.k) return 3;
    FILE *f = fopen(argv[7], "rb");
    if (!f) return 4;
    std::string s;
    std::vector<char> buf(1 << 20);
    size_t got;
    while ((got = fread(buf.data(), 1, buf.size(), f)) > 0) s.append(buf.data(), got);
    fclose(f);
    if (!s.empty() && s.back() != '\n') return 7;
    const size_t stretch = atol(argv[8]) > 0 ? (size_t)atol(argv[8]) : std::max<size_t>(1, s.size());
    const size_t n_reads = (size_t)std::count(s.begin(), s.end(), '\n');
    std::vector<np2trio::Tally> reads(n_reads + 1); // (the last one stays empty: the stream ends in a separator)

    const uint32_t k = pat.k;
    const uint64_t mask = np2kc::kmer_mask(k);
    uint32_t prefix = 0; // the exclusive scan of the stretches' seg_word under seg_right
    size_t head_read = 0;
    for (size_t a = 0; a < s.size(); a += stretch) {
        const size_t b = std::min(s.size(), a + stretch);
        np2kc::Roll r;
        uint64_t h = 0;
        for (size_t e = a >= np2kc::HALO ? a - np2kc::HALO : 0; e < a; ++e) (void)np2kc::push(r, (uint8_t)s[e], k, mask, &h);
        np2bin::Stretch st;
        np2trio::Tally t;
        np2trio::Run run;
        for (size_t e = a; e < b; ++e) {
            const bool valid = np2kc::push(r, (uint8_t)s[e], k, mask, &h);
            const uint32_t cls = valid ? np2trio::classify(pat.get(h), mat.get(h), min_count, mid_count) : np2trio::NONE;
            np2bin::walk(st, t, run, valid, cls, s[e] == '\n', [&](uint32_t i, const np2trio::Tally &c) { np2bin::add(reads[head_read + i], c); });
        }
        np2bin::walk_end(st, t, run);
        np2bin::join_head(st, prefix);
        np2bin::add(reads[head_read], st.head);
        if (st.n_bounds) np2bin::add(reads[head_read + st.n_bounds], st.tail);
        prefix = np2trio::seg_right(prefix, np2bin::seg_word(st));
        head_read += st.n_bounds;
    }
    for (size_t i = 0; i < n_reads; ++i) {
        const np2trio::Tally &t = reads[i];
        printf("read %u %u %u %u %u %u %u %c\n", t.n_kmers, t.n_pat, t.n_mat, t.pp, t.pm, t.mp, t.mm, (char)np2bin::class_of(t, min_score, permille));
    }
    return 0;
}
