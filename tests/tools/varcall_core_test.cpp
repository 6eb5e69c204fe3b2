// Host run of the variant caller's rule (csrc/np2_varcall_core.hpp): codes, admission, the event rule and both left shifts,
// the key's order, the call tests at their boundaries, and call_contig on a hand-written contig.
//   varcall_core_test            exit 0 and "ok <checks>" when every case holds; 1 and the failed case otherwise
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../nextpolish2_amd/csrc/np2_varcall_core.hpp"

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        ++g_checks;                               \
        if (!(cond)) {                            \
            ++g_failed;                           \
            fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);         \
            fprintf(stderr, "\n");                \
        }                                         \
    } while (0)

static uint32_t op(char c, uint32_t len) {
    const char *ops = "MIDNSHP=X";
    uint32_t k = 0;
    while (ops[k] != c) ++k;
    return len << 4 | k;
}

struct Input {
    std::vector<np2_bamrec_t> recs;
    std::vector<uint32_t> cigar;
    std::vector<uint8_t> seq;
    void add(int32_t pos, uint32_t flag, uint32_t mapq, const std::vector<uint32_t> &cg, const std::string &s) {
        np2_bamrec_t r{};
        r.pos = pos, r.flag = (uint16_t)flag, r.mapq = (uint8_t)mapq, r.n_cigar = (uint32_t)cg.size(), r.cigar_off = cigar.size();
        r.l_seq = (uint32_t)s.size(), r.seq_off = seq.size();
        cigar.insert(cigar.end(), cg.begin(), cg.end());
        const std::string nib = "=ACMGRSVTWYHKDBN";
        for (size_t i = 0; i < s.size(); i += 2) {
            const uint32_t hi = (uint32_t)nib.find(s[i]), lo = i + 1 < s.size() ? (uint32_t)nib.find(s[i + 1]) : 0u;
            seq.push_back((uint8_t)(hi << 4 | lo));
        }
        recs.push_back(r);
    }
};

static np2vc::Rule rule(uint32_t min_depth = 1, uint32_t min_alt = 1, uint32_t hom = 800, uint32_t het = 250, uint32_t max_indel = 28) {
    return np2vc::Rule{0.0, 0xF04, 5, min_depth, min_alt, hom, het, max_indel};
}

int main() {
    using namespace np2vc;
    // codes
    CHECK(ref_code('A') == 0 && ref_code('c') == 1 && ref_code('G') == 2 && ref_code('t') == 3 && ref_code('N') == 4 && ref_code('n') == 4 && ref_code(0) == 4 && ref_code('!') == 4 && ref_code(1) == 4, "ref codes");
    for (uint32_t n = 0; n < 16; ++n) CHECK(nib_code(n) == (n == 1 ? 0u : n == 2 ? 1u : n == 4 ? 2u : n == 8 ? 3u : 4u), "nibble %u", n);
    const uint8_t two[2] = {0x12, 0x4F};
    CHECK(read_code(two, 0) == 0 && read_code(two, 1) == 1 && read_code(two, 2) == 2 && read_code(two, 3) == 4, "high nibble first");
    // rule_ok
    CHECK(rule_ok(rule()) && rule_ok(rule(0, 1, 1000, 1000)) && rule_ok(rule(0, 1, 0, 0)), "rules that hold");
    CHECK(!rule_ok(rule(1, 1, 1001, 250)) && !rule_ok(rule(1, 1, 500, 501)) && !rule_ok(rule(1, 1, 800, 250, 0)) && !rule_ok(rule(1, 1, 800, 250, 29)) && !rule_ok(rule(1, 0)), "rules refused");
    // the call tests at their boundaries: c * 1000 == pm * d exactly and one below
    CHECK(reaches(16, 20, 800) && !reaches(15, 20, 800) && reaches(5, 20, 250) && !reaches(4, 20, 250) && reaches(0, 0, 1000), "reaches");
    CHECK(reaches(0xFFFFFFFFu, 0xFFFFFFFFu, 1000) && !reaches(0xFFFFFFFEu, 0xFFFFFFFFu, 1000), "no 32-bit overflow");
    const Rule r8 = rule(8, 3);
    CHECK(judge(20, 16, r8) == GT_HOM && judge(20, 15, r8) == GT_HET && judge(20, 5, r8) == GT_HET && judge(20, 4, r8) == GT_NONE, "judge thresholds");
    CHECK(judge(8, 8, r8) == GT_HOM && judge(7, 7, r8) == GT_NONE && judge(8, 3, r8) == GT_HET && judge(8, 2, r8) == GT_NONE, "judge depth and count");
    CHECK(judge(20, 15, rule(8, 3, 800, 800)) == GT_NONE, "het_pm = hom_pm: homozygous only");
    // SNV ties: the smaller code; the reference base is never chosen
    uint32_t b, c;
    const uint32_t a1[4] = {0, 0, 3, 3}, a2[4] = {0, 5, 0, 0}, a3[4] = {0, 0, 0, 0};
    best_snv(a1, 1, b, c);
    CHECK(b == 2 && c == 3, "tie G < T");
    best_snv(a2, 0, b, c);
    CHECK(b == 1 && c == 5, "C");
    best_snv(a3, 0, b, c);
    CHECK(b == 1 && c == 0, "nothing: the first alt base");
    // key order = (anchor, kind, n, bases)
    CHECK(key_hi(5, KEY_DEL, 28) < key_hi(5, KEY_INS, 1) && key_hi(5, KEY_INS, 28) < key_hi(6, KEY_DEL, 1) && key_hi(5, KEY_INS, 1) < key_hi(5, KEY_INS, 2), "key order");
    CHECK(key_anchor(key_hi(0xFFFEFFFFu, 1, 28)) == 0xFFFEFFFFu && key_kind(key_hi(7, 1, 28)) == 1 && key_n(key_hi(7, 1, 28)) == 28 && key_hi(0xFFFFFFFFu, 1, 31) < (1ull << KEY_HI_BITS), "key fields");

    //                  0         1         2         3
    //                  0123456789012345678901234567890123456789
    const std::string ref = "GATCGATTACAAAAAAGCTCGTGTGTGTCAGGCATTCAGA";
    const uint32_t L = (uint32_t)ref.size();
    auto read_for = [&](int pos, const std::vector<uint32_t> &cg, const std::string &ins) {
        std::string s;
        size_t p = (size_t)pos;
        for (uint32_t w : cg) {
            const uint32_t o = w & 15, n = w >> 4;
            if (o == 0) s += ref.substr(p, n), p += n;
            else if (o == 1 || o == 4) s += ins.substr(0, n);
            else if (o == 2) p += n;
        }
        return s;
    };
    {
        // one more A in the run 10..15 at six offsets: all on anchor 9; a read that starts inside the run stops at m - 1; a read
        // mismatch stops the shift; a GT out of (GT)4 at three offsets: all on anchor 19
        Input in;
        for (uint32_t k = 1; k <= 6; ++k) in.add(2, 0, 60, {op('M', 8 + k), op('I', 1), op('M', 20)}, read_for(2, {op('M', 8 + k), op('I', 1), op('M', 20)}, "A"));
        in.add(12, 0, 60, {op('M', 4), op('I', 1), op('M', 10)}, read_for(12, {op('M', 4), op('I', 1), op('M', 10)}, "A"));
        std::string s = read_for(2, {op('M', 14), op('I', 1), op('M', 20)}, "A");
        s[11] = 'C';
        in.add(2, 0, 60, {op('M', 14), op('I', 1), op('M', 20)}, s);
        for (uint32_t k = 0; k <= 4; k += 2) in.add(5, 0, 60, {op('M', 17 + k), op('D', 2), op('M', 10)}, read_for(5, {op('M', 17 + k), op('D', 2), op('M', 10)}, ""));
        Contig out;
        CHECK(call_contig((const uint8_t *)ref.data(), L, in.recs.data(), (uint32_t)in.recs.size(), in.cigar.data(), in.seq.data(), in.seq.size(), rule(1, 1, 1000, 0), out), "call_contig");
        CHECK(out.stats.records_counted == 11 && out.stats.events == 11 && out.stats.alleles == 4, "events %llu alleles %llu", (unsigned long long)out.stats.events, (unsigned long long)out.stats.alleles);
        CHECK(out.alt[4 * 13 + 1] == 1, "the mismatch at 13");
        uint64_t alt_sum = 0;
        for (uint32_t v : out.alt) alt_sum += v;
        CHECK(alt_sum == 1, "no other mismatch: the shifts change no column");
        // het_pm 0: SNV at 13 (1 of 8), INS at 9 (6), 12 (1), 13 (1), DEL at 19 (3)
        CHECK(out.calls.size() == 5, "%zu calls", out.calls.size());
        if (out.calls.size() == 5) {
            const np2_varcall_t *v = out.calls.data();
            CHECK(v[0].pos == 9 && v[0].kind == INS && v[0].count == 6 && v[0].len == 1 && v[0].bases == 0 && v[0].depth == 10, "INS at 9: count %u depth %u", v[0].count, v[0].depth);
            CHECK(v[1].pos == 12 && v[1].kind == INS && v[1].count == 1, "INS at 12");
            CHECK(v[2].pos == 13 && v[2].kind == SNV && v[2].alt_code == 1 && v[2].count == 1, "SNV before INS at 13");
            CHECK(v[3].pos == 13 && v[3].kind == INS && v[3].count == 1, "INS at 13");
            CHECK(v[4].pos == 19 && v[4].kind == DEL && v[4].count == 3 && v[4].len == 2 && v[4].gt == GT_HET, "DEL at 19");
        }
        // cov: a deletion covers
        CHECK(out.cov[0] == 0 && out.cov[2] == 7 && out.cov[5] == 10 && out.cov[12] == 11, "cov %u %u %u %u", out.cov[0], out.cov[2], out.cov[5], out.cov[12]);
    }
    {
        // admission and the records that are not events
        Input in;
        const std::string m30 = ref.substr(0, 30);
        in.add(0, 0, 60, {op('M', 30)}, m30);
        in.add(0, 0x100, 60, {op('M', 30)}, m30);                               // secondary
        in.add(0, 0, 4, {op('M', 30)}, m30);                                    // mapq
        in.add(-1, 0, 60, {op('M', 30)}, m30), in.add((int32_t)L, 0, 60, {op('M', 30)}, m30);
        in.add(0, 0, 60, {op('M', 30)}, m30.substr(0, 29));                     // l_seq short
        in.add(0, 0, 60, {op('M', 30)}, "");                                    // SEQ *
        in.add(0, 0, 60, {op('M', 10), op('N', 5), op('M', 10)}, ref.substr(0, 20));
        in.add(0, 0, 60, {op('I', 2), op('M', 10), op('D', 2)}, "CC" + ref.substr(0, 10));           // leading, trailing
        in.add(0, 0, 60, {op('S', 2), op('I', 2), op('M', 10), op('D', 1), op('S', 1)}, "GGCC" + ref.substr(0, 10) + "T"); // next to clips
        in.add(0, 0, 60, {op('M', 5), op('I', 1), op('D', 1), op('M', 5)}, ref.substr(0, 5) + "C" + ref.substr(6, 5));     // adjacent
        in.add(0, 0, 60, {op('M', 5), op('I', 2), op('M', 5)}, ref.substr(0, 5) + "NC" + ref.substr(5, 5));                 // N inserted
        in.add((int32_t)L - 6, 0, 60, {op('M', 5), op('D', 2), op('M', 3)}, ref.substr(L - 6, 5) + "AAA");                  // a + n = L
        in.add((int32_t)L - 6, 0, 60, {op('M', 6), op('I', 1), op('M', 3)}, ref.substr(L - 6, 6) + "CAAA");                 // a + 1 = L
        Contig out;
        CHECK(call_contig((const uint8_t *)ref.data(), L, in.recs.data(), (uint32_t)in.recs.size(), in.cigar.data(), in.seq.data(), in.seq.size(), rule(), out), "call_contig");
        CHECK(out.stats.records_seen == 14 && out.stats.records_counted == 7 && out.stats.records_no_seq == 2 && out.stats.records_skipped == 1, "admission %llu %llu %llu",
              (unsigned long long)out.stats.records_counted, (unsigned long long)out.stats.records_no_seq, (unsigned long long)out.stats.records_skipped);
        CHECK(out.stats.events == 0, "%llu events", (unsigned long long)out.stats.events);
        // a record whose SEQ lies outside the buffer is refused
        Contig bad;
        CHECK(!call_contig((const uint8_t *)ref.data(), L, in.recs.data(), 1, in.cigar.data(), in.seq.data(), 14, rule(), bad), "SEQ outside the buffer");
    }
    {
        // L = 0 and no records
        Contig out;
        CHECK(call_contig(nullptr, 0, nullptr, 0, nullptr, nullptr, 0, rule(), out) && out.calls.empty() && out.cov.empty(), "L = 0");
        CHECK(call_contig((const uint8_t *)ref.data(), L, nullptr, 0, nullptr, nullptr, 0, rule(0, 1, 0, 0), out) && out.calls.empty() && out.stats.callable == L, "no records");
    }
    if (g_failed) return 1;
    printf("ok %d\n", g_checks);
    return 0;
}
