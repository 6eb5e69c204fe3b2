// Host run of the assembly-to-reference caller's rule (csrc/np2_asmcall_core.hpp): codes, the owned SAM interval, admission, the
// key and the footprint test, every refusal of check(), and call_all on hand-written alignments.
//   asmcall_core_test            exit 0 and "ok <checks>" when every case holds; 1 and the failed case otherwise
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../nextpolish2_amd/csrc/np2_asmcall_core.hpp"

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
    std::string refs, query;
    std::vector<uint64_t> ref_off{0};
    std::vector<np2_asmaln_t> alns;
    std::vector<uint32_t> cigar;
    void ref(const std::string &s) { refs += s, ref_off.push_back(refs.size()); }
    np2_asmaln_t &add(int32_t tid, uint32_t pos, uint32_t flag, const std::vector<uint32_t> &cg, const std::string &fwd, uint32_t lo, uint32_t hi,
                      uint32_t mapq = 60) {
        np2_asmaln_t a{};
        a.tid = tid, a.pos = pos, a.flag = flag, a.mapq = mapq, a.n_cigar = (uint32_t)cg.size(), a.q_len = (uint32_t)fwd.size();
        a.own_lo = lo, a.own_hi = hi, a.cigar_off = cigar.size(), a.q_off = query.size();
        cigar.insert(cigar.end(), cg.begin(), cg.end());
        query += fwd;
        alns.push_back(a);
        return alns.back();
    }
    const char *check(std::vector<uint8_t> *adm, bool *unsupported, uint32_t min_mapq = 5, uint32_t min_aln = 4) const {
        uint32_t bad;
        return np2ac::check(ref_off.data(), (uint32_t)ref_off.size() - 1, query.size(), alns.data(), (uint32_t)alns.size(), cigar.data(), cigar.size(),
                            min_mapq, min_aln, adm, unsupported, &bad);
    }
    bool run(np2ac::Result &r, uint32_t min_aln = 4) const {
        std::vector<uint8_t> adm;
        bool u;
        if (check(&adm, &u, 5, min_aln)) return false;
        np2ac::call_all((const uint8_t *)refs.data(), ref_off.data(), (uint32_t)ref_off.size() - 1, (const uint8_t *)query.data(), alns.data(),
                        (uint32_t)alns.size(), cigar.data(), adm, r);
        return true;
    }
};

static std::string revcomp(const std::string &s) {
    std::string o(s.rbegin(), s.rend());
    for (char &c : o) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
    return o;
}

int main() {
    using namespace np2ac;
    CHECK(code('A') == 0 && code('c') == 1 && code('G') == 2 && code('t') == 3 && code('N') == 4 && code(0) == 4 && code('!') == 4, "codes");
    CHECK(comp(0) == 3 && comp(1) == 2 && comp(2) == 1 && comp(3) == 0 && comp(4) == 4, "complements");
    {
        np2_asmaln_t a{};
        a.q_len = 10, a.own_lo = 2, a.own_hi = 7;
        uint32_t lo, hi;
        owned_sam(a, lo, hi);
        CHECK(lo == 2 && hi == 7, "owned forward");
        a.flag = 16;
        owned_sam(a, lo, hi);
        CHECK(lo == 3 && hi == 8, "owned reverse");
        const uint8_t q[4] = {'A', 'C', 'n', 'T'};
        CHECK(sam_code(q, 4, false, 1) == 1 && sam_code(q, 4, true, 0) == 0 && sam_code(q, 4, true, 2) == 2 && sam_code(q, 4, true, 1) == 4, "SAM bases");
        CHECK(fwd_snv(10, true, 0) == 9 && fwd_ins(10, true, 2, 3) == 5 && fwd_del(10, true, 4) == 6 && fwd_del(10, false, 10) == 10, "forward indices");
    }
    CHECK(admit(4, 60, 1, false, 100, 5, 10) == ALN_UNALIGNED && admit(0, 60, 0, false, 100, 5, 10) == ALN_UNALIGNED, "unaligned");
    CHECK(admit(0, 4, 1, true, 1, 5, 10) == ALN_LOW_MAPQ && admit(0, 5, 1, true, 1, 5, 10) == ALN_SKIPPED && admit(0, 5, 1, false, 9, 5, 10) == ALN_SHORT &&
              admit(16, 5, 1, false, 10, 5, 10) == ALN_ADMITTED, "the first failing test names the outcome");
    CHECK(key(5, INS) > key(5, DEL) && key(5, DEL) > key(5, SNV) && key(6, SNV) > key(5, INS) && (key(0xFFFF0000ull, INS) >> KEY_BITS) == 0, "keys");
    {
        const uint32_t cov[6] = {1, 1, 2, 1, 1, 1}, ones[6] = {1, 2, 2, 3, 4, 5};
        CHECK(kept(SNV, 0, 1, 6, cov, ones) && !kept(SNV, 2, 1, 6, cov, ones), "SNV footprint");
        CHECK(kept(DEL, 3, 2, 6, cov, ones) && !kept(DEL, 0, 2, 6, cov, ones) && !kept(DEL, 1, 1, 6, cov, ones) && kept(DEL, 0, 1, 6, cov, ones), "DEL footprint");
        CHECK(kept(INS, 0, 9, 6, cov, ones) && !kept(INS, 1, 1, 6, cov, ones) && kept(INS, 5, 1, 6, cov, ones) && kept(INS, 1, 1, 2, cov, ones), "INS footprint");
    }
    // refusals
    {
        bool u;
        Input in;
        in.ref("ACGTACGTAC");
        in.add(0, 0, 0, {op('M', 10)}, "ACGTACGTAC", 0, 10);
        CHECK(in.check(nullptr, &u) == nullptr, "a plain alignment passes");
        Input b = in;
        b.alns[0].tid = 1;
        CHECK(b.check(nullptr, &u) && !u, "tid outside");
        b = in, b.alns[0].tid = -1;
        CHECK(b.check(nullptr, &u) && !u, "tid negative");
        b = in, b.alns[0].pos = 1;
        CHECK(b.check(nullptr, &u) && !u, "beyond the end");
        b = in, b.alns[0].q_len = 9, b.alns[0].own_hi = 9;
        CHECK(b.check(nullptr, &u) && !u, "query length");
        b = in, b.alns[0].own_hi = 11;
        CHECK(b.check(nullptr, &u) && !u, "own_hi beyond q_len");
        b = in, b.alns[0].own_lo = 6, b.alns[0].own_hi = 5;
        CHECK(b.check(nullptr, &u) && !u, "own_lo above own_hi");
        b = in, b.alns[0].cigar_off = 1;
        CHECK(b.check(nullptr, &u) && !u, "CIGAR outside");
        b = in, b.alns[0].q_off = 1;
        CHECK(b.check(nullptr, &u) && !u, "query outside");
        b = in, b.ref_off[0] = 1;
        CHECK(b.check(nullptr, &u) && !u, "ref_off[0]");
        b = in, b.ref_off.push_back(5);
        CHECK(b.check(nullptr, &u) && !u, "ref_off descending");
        b = in, b.alns[0].flag = 4, b.alns[0].tid = -1, b.alns[0].pos = 999;
        CHECK(b.check(nullptr, &u) == nullptr, "an unaligned record's tid and pos are not read");
        b = in, b.cigar[0] = op('N', 10), b.alns[0].tid = 7;
        std::vector<uint8_t> adm;
        CHECK(b.check(&adm, &u) == nullptr && adm[0] == ALN_SKIPPED, "an N operation: skipped, nothing else is checked");
        const uint64_t big[2] = {0, 0xFFFF0001ull};
        uint32_t bad;
        CHECK(check(big, 1, 0, nullptr, 0, nullptr, 0, 5, 5, nullptr, &u, &bad) && u, "too many reference bases");
        const uint64_t ok[2] = {0, 0xFFFF0000ull};
        CHECK(check(ok, 1, 0, nullptr, 0, nullptr, 0, 5, 5, nullptr, &u, &bad) == nullptr, "the largest total passes");
        CHECK(check(ok, 1, 0xFFFF0000ull, nullptr, 0, nullptr, 1, 5, 5, nullptr, &u, &bad) && u, "too many query bytes and CIGAR words");
    }
    // one alignment of each kind on each strand: ref ACGTACGTACGTTTGACC, query with an SNV at 2, 2 bases deleted after 5, 1 inserted after 11
    for (int rev = 0; rev < 2; ++rev) {
        Input in;
        in.ref("ACGTACGTACGTTTGACC");
        const std::string sam = std::string("ACTTAC") + "ACGT" + "A" + "TTGACC"; // 6M 2D 4M 1I 6M: 17 bases
        in.add(0, 0, rev ? 16 : 0, {op('M', 6), op('D', 2), op('M', 4), op('I', 1), op('M', 6)}, rev ? revcomp(sam) : sam, 0, 17);
        Result r;
        CHECK(in.run(r), "runs");
        CHECK(r.stats.alns_admitted == 1 && r.runs.size() == 1 && r.runs[0].tid == 0 && r.runs[0].start == 0 && r.runs[0].end == 18, "one run over the reference");
        CHECK(r.vars.size() == 3, "three events, got %zu", r.vars.size());
        if (r.vars.size() == 3) {
            const np2_asmvar_t &s = r.vars[0], &d = r.vars[1], &i = r.vars[2];
            CHECK(s.kind == SNV && s.pos == 2 && s.ref_code == 2 && s.alt_code == 3 && s.q_pos == (rev ? 14u : 2u) && s.rev == rev, "SNV");
            CHECK(d.kind == DEL && d.pos == 5 && d.len == 2 && d.q_pos == (rev ? 11u : 6u), "DEL q_pos %u", d.q_pos);
            CHECK(i.kind == INS && i.pos == 11 && i.len == 1 && i.q_pos == (rev ? 6u : 10u), "INS q_pos %u", i.q_pos);
        }
        CHECK(r.stats.kept[SNV] == 1 && r.stats.kept[DEL] == 1 && r.stats.kept[INS] == 1 && r.stats.del_bases == 2 && r.stats.ins_bases == 1 &&
                  r.stats.r_bases == 18 && r.stats.cov0_bases == 0 && r.stats.cov2_bases == 0, "stats");
        // ownership: the D's anchor is SAM column 5; owning [0, 5) drops it and its cover, owning [0, 6) keeps both
        in.alns[0].own_lo = rev ? 12 : 0, in.alns[0].own_hi = rev ? 17 : 5;
        CHECK(in.run(r, 0) && r.vars.size() == 1 && r.runs.size() == 1 && r.runs[0].end == 5, "anchor outside: the D does not belong");
        in.alns[0].own_lo = rev ? 11 : 0, in.alns[0].own_hi = rev ? 17 : 6;
        CHECK(in.run(r, 0) && r.vars.size() == 2 && r.runs[0].end == 8, "anchor is the last owned column: the D belongs and covers");
        in.alns[0].own_lo = in.alns[0].own_hi = 3;
        CHECK(in.run(r, 0) && r.vars.empty() && r.runs.empty() && r.stats.alns_admitted == 1 && r.stats.cov0_bases == 18, "an empty owned interval");
    }
    // two alignments overlapping: coverage 2 drops their events; runs do not cross a joint; no alignments; a reference of one base
    {
        Input in;
        in.ref("ACGTACGT"), in.ref("A"), in.ref("ACGT");
        in.add(0, 0, 0, {op('M', 8)}, "ACGAACGT", 0, 8);
        in.add(0, 2, 0, {op('M', 4)}, "GAAC", 0, 4);
        in.add(1, 0, 0, {op('M', 1)}, "C", 0, 1);
        in.add(2, 0, 0, {op('M', 4)}, "ACGA", 0, 4);
        Result r;
        CHECK(in.run(r, 0), "runs");
        CHECK(r.stats.found[SNV] == 4 && r.vars.size() == 2 && r.vars[0].tid == 1 && r.vars[1].tid == 2 && r.vars[1].pos == 3, "coverage 2 drops both SNVs at 3");
        CHECK(r.runs.size() == 4 && r.runs[1].start == 6 && r.runs[2].tid == 1 && r.runs[2].end == 1 && r.runs[3].tid == 2 && r.runs[3].start == 0,
              "runs stop at coverage 2 and at the joints");
        CHECK(r.stats.cov2_bases == 4 && r.stats.r_bases == 9, "coverage totals");
        Input none;
        none.ref("ACGT");
        CHECK(none.run(r) && r.runs.empty() && r.vars.empty() && r.stats.cov0_bases == 4, "no alignments");
        Input empty;
        CHECK(empty.run(r) && r.cov.empty(), "no references");
    }
    if (g_failed) return fprintf(stderr, "%d of %d checks failed\n", g_failed, g_checks), 1;
    printf("ok %d\n", g_checks);
    return 0;
}
