// The rule of the reads door of the resident SAM (csrc/np2_alnpack_core.hpp) and its host twin (csrc/np2_alnpack_host.cpp,
// np2_align_pack_host) built with a plain C++ compiler, for tests/test_mappolish_cpu.py: with and without the address and
// undefined-behaviour sanitizers.  Checks a handful of the rule's statements as literals, the word path (two aligned loads and a
// funnel shift) against the byte path at every alignment, length and strand, and prints "ok N" (N checks) or the first failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../nextpolish2_amd/csrc/np2_alnpack_host.cpp"

namespace np2h {
static std::string last_error;
int io_set_error(int code, const std::string &msg) {
    last_error = msg;
    return code;
}
} // namespace np2h

static int n_checks = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        ++n_checks;                                                      \
        if (!(cond)) {                                                   \
            printf("line %d: %s does not hold\n", __LINE__, #cond);     \
            return 1;                                                    \
        }                                                                \
    } while (0)

static std::vector<uint8_t> packed(const std::string &q, bool rev) {
    std::vector<uint8_t> out;
    for (uint32_t b = 0; b < (q.size() + 1) / 2; ++b) out.push_back(np2pack::seq4_byte((const uint8_t *)q.data(), (uint32_t)q.size(), rev, b));
    return out;
}

int main() {
    using namespace np2pack;
    // the complement: ACGT in their case, any other byte itself
    CHECK(comp('A') == 'T' && comp('C') == 'G' && comp('G') == 'C' && comp('T') == 'A');
    CHECK(comp('a') == 't' && comp('c') == 'g' && comp('g') == 'c' && comp('t') == 'a');
    CHECK(comp('N') == 'N' && comp('n') == 'n' && comp('R') == 'R' && comp('y') == 'y' && comp('*') == '*' && comp('=') == '=');
    CHECK(comp('U') == 'U' && comp(0) == 0 && comp(0xC1) == 0xC1 && comp(0xE1) == 0xE1); // ('A' | 0x80 is no base)
    // SEQ bytes: forward as they stand; reverse from the far end, complemented
    CHECK(packed("ACGTN", false) == (std::vector<uint8_t>{0x12, 0x48, 0xF0}));
    CHECK(packed("ACGTN", true) == (std::vector<uint8_t>{0xF1, 0x24, 0x80})); // NACGT
    CHECK(packed("acgt", true) == (std::vector<uint8_t>{0x12, 0x48}));
    CHECK(packed("Ry*=", false) == (std::vector<uint8_t>{0x5A, 0xF0}));        // R 5, Y 10, anything else 15, = 0
    CHECK(packed("Ry*=", true) == (std::vector<uint8_t>{0x0F, 0xA5}));         // =*yR: not complemented
    CHECK(packed("G", true) == (std::vector<uint8_t>{0x20}) && packed("", false).empty());
    // the word path against the byte path: every source alignment, lengths 8 .. 41, both strands, every word of the read
    {
        const char *alphabet = "ACGTacgtNnRyKm*=.";
        std::vector<uint8_t> buf(8 + 64 + 16, 0xEE); // (what lies around a read is read by the aligned loads and shifted out)
        uint32_t x = 12345;
        for (uint32_t shift = 0; shift < 8; ++shift)
            for (uint32_t len = 8; len <= 41; ++len) {
                // an 8-byte aligned base whatever the vector's own alignment
                uint8_t *base = buf.data() + ((8 - ((uintptr_t)buf.data() & 7u)) & 7u);
                uint8_t *q = base + 8 + shift;
                if (q + len + 16 > buf.data() + buf.size()) continue;
                for (uint32_t i = 0; i < len; ++i) x = x * 1103515245u + 12345u, q[i] = (uint8_t)alphabet[(x >> 16) % 17u];
                for (int rev = 0; rev < 2; ++rev)
                    for (uint32_t b0 = 0; 2 * b0 + 8 <= len; ++b0) {
                        const uint32_t w = seq4_word(q, len, rev != 0, b0);
                        uint32_t want = 0;
                        for (uint32_t t = 0; t < 4; ++t) want |= (uint32_t)seq4_byte(q, len, rev != 0, b0 + t) << (8 * t);
                        CHECK(w == want);
                    }
                memset(q, 0xEE, len);
            }
    }
    // the record words, the key and the kept predicate
    np2aln::Rec r{};
    r.tid = 2, r.flag = 16, r.pos = 499, r.end = 1099, r.mapq = 60, r.n_cigar = 3, r.nm = 1, r.as = 590;
    const uint64_t co = 0x100000007ull, so = 0x300000005ull;
    const uint32_t want_words[REC_WORDS] = {499u, 16u | 60u << 16, 3u, 0u, 7u, 1u, 601u, 0u, 5u, 3u};
    for (uint32_t j = 0; j < REC_WORDS; ++j) CHECK(rec_word(r, 601, co, so, j) == want_words[j]);
    CHECK(rec_key(r, 1) == ((uint64_t)2 << 33 | (uint64_t)500 << 1 | 1u) && rec_key(r, 0) == ((uint64_t)2 << 33 | (uint64_t)500 << 1));
    CHECK(kept(r) && !kept(np2aln::unaligned_rec()));
    r.flag = 4;
    CHECK(!kept(r));
    // the whole rule through the C entry point: three reads at one start (reverse, forward, unmapped between them)
    {
        np2_align_rec_t recs[3] = {{0, 16, 10, 15, 60, 2, 0, 5}, {-1, 4, 0, 0, 0, 0, 0, 0}, {0, 0, 10, 13, 7, 1, 0, 3}};
        const uint32_t cigar[3] = {5u << 4 | 0u, 1u << 4 | 4u, 3u << 4 | 0u};
        const uint64_t off[4] = {0, 2, 2, 3};
        const std::string reads = "AACGTT\nGGGG\nACN\n";
        for (uint32_t tie = 0; tie < 2; ++tie) {
            np2_sam_opts_t so_{tie};
            np2_bamrec_t *out = nullptr;
            int32_t *tids = nullptr;
            uint32_t *cg = nullptr;
            uint8_t *seq4 = nullptr;
            uint64_t n = 0;
            CHECK(np2_align_pack_host(recs, cigar, off, (const uint8_t *)reads.data(), reads.size(), 3, &so_, &out, &tids, &cg, &seq4, &n) == NP2_OK);
            CHECK(n == 2 && tids[0] == 0 && tids[1] == 0);
            const int fwd = tie ? 0 : 1; // by strand the forward record comes first; in input order the reverse one
            CHECK(out[fwd].flag == 0 && out[fwd].mapq == 7 && out[fwd].pos == 10 && out[fwd].l_seq == 3 && out[fwd].seq_off == 3 && out[fwd].pad == 0);
            CHECK(out[1 - fwd].flag == 16 && out[1 - fwd].mapq == 60 && out[1 - fwd].l_seq == 6 && out[1 - fwd].seq_off == 0 && out[1 - fwd].n_cigar == 2);
            CHECK(out[0].cigar_off == 0 && out[1].cigar_off == out[0].n_cigar);
            CHECK(cg[out[fwd].cigar_off] == (3u << 4) && cg[out[1 - fwd].cigar_off] == (5u << 4) && cg[out[1 - fwd].cigar_off + 1] == (1u << 4 | 4u));
            const uint8_t want_seq[5] = {0x11, 0x24, 0x88, 0x12, 0xF0}; // AACGTT reversed and complemented is itself; ACN
            CHECK(!memcmp(seq4, want_seq, 5));
            free(out), free(tids), free(cg), free(seq4);
        }
        np2_bamrec_t *out = nullptr;
        int32_t *tids = nullptr;
        uint32_t *cg = nullptr;
        uint8_t *seq4 = nullptr;
        uint64_t n = 0;
        const uint64_t bad[4] = {0, 1, 1, 2};
        CHECK(np2_align_pack_host(recs, cigar, bad, (const uint8_t *)reads.data(), reads.size(), 3, nullptr, &out, &tids, &cg, &seq4, &n) == NP2_E_ARG);
        CHECK(np2h::last_error.find("cigar_off") != std::string::npos && !out && !seq4);
        CHECK(np2_align_pack_host(recs, cigar, off, (const uint8_t *)reads.data(), reads.size() - 1, 3, nullptr, &out, &tids, &cg, &seq4, &n) == NP2_E_ARG);
        CHECK(np2_align_pack_host(nullptr, nullptr, off, nullptr, 0, 0, nullptr, &out, &tids, &cg, &seq4, &n) == NP2_OK && n == 0 && !out);
    }
    printf("ok %d\n", n_checks);
    return 0;
}
