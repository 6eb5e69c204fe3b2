// The short-read adapter rule's core (csrc/np2_sradapt_core.hpp) as a stand-alone host program: judge_pair / judge_single
// over a text file of reads and options.  Built with -fsanitize=address,undefined by tests/test_sradapt_cpu.py, which compares
// what it prints with the plain-Python model of tests/sradapt_model.py.
//
// Input: line 1 holds the nine quality options (trim_front trim_tail cut_window cut_mean_q n_base_limit qualified_q
// unqualified_percent min_len flags), the four adapter options (flags overlap_min overlap_diff overlap_diff_percent) and the
// two adapter strings ("-": none).  Every read follows as two lines, bases and qualities (either may be empty); in pair
// mode mate 1 and mate 2 alternate.  Output: "begin end cls how insert" per read, then "totals" and the fourteen totals; or
// "invalid <why>" when the options are refused.
#include "../../nextpolish2_amd/csrc/np2_sradapt_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace np2sradapt;

// exact-size heap copies: a read past either end is the sanitizer's to report
static std::vector<uint8_t> bytes(const std::string &s) { return std::vector<uint8_t>(s.begin(), s.end()); }

int main(int argc, char **argv) {
    if (argc != 2) return std::fprintf(stderr, "usage: sradapt_core_test cases.txt\n"), 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::string line;
    if (!in || !std::getline(in, line)) return std::fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    np2srqc::Opts qc;
    uint32_t flags, o_min, o_diff, o_pct;
    std::string a1, a2;
    std::istringstream hd(line);
    hd >> qc.trim_front >> qc.trim_tail >> qc.cut_window >> qc.cut_mean_q >> qc.n_base_limit >> qc.qualified_q >> qc.unqualified_percent >> qc.min_len >>
        qc.flags >> flags >> o_min >> o_diff >> o_pct >> a1 >> a2;
    if (!hd) return std::fprintf(stderr, "bad option line\n"), 2;
    Opts o;
    const char *why = np2srqc::invalid(qc);
    if (!why) why = make_opts(flags, o_min, o_diff, o_pct, a1 == "-" ? nullptr : a1.c_str(), a2 == "-" ? nullptr : a2.c_str(), o);
    if (why) return std::printf("invalid %s\n", why), 0;
    std::vector<std::vector<uint8_t>> s, q;
    std::string ql;
    while (std::getline(in, line)) {
        if (!std::getline(in, ql) || ql.size() != line.size()) return std::fprintf(stderr, "read %zu: bad quality line\n", s.size() + 1), 2;
        s.push_back(bytes(line)), q.push_back(bytes(ql));
    }
    const bool paired = (o.flags & PAIRED) != 0;
    if (paired && s.size() % 2) return std::fprintf(stderr, "an odd number of reads in pair mode\n"), 2;
    uint64_t t[N_TOTALS] = {};
    auto out = [&](const Read &r, size_t i) {
        uint32_t a0, b0;
        (void)np2srqc::judge_serial(s[i].data(), q[i].data(), (uint32_t)s[i].size(), qc, a0, b0);
        add_read(t, r, (uint32_t)s[i].size(), b0);
        std::printf("%u %u %u %u %u\n", r.begin, r.end, r.cls, r.how, r.insert);
    };
    for (size_t i = 0; i < s.size(); i += paired ? 2 : 1) {
        if (paired) {
            Read r1, r2;
            judge_pair(s[i].data(), q[i].data(), (uint32_t)s[i].size(), s[i + 1].data(), q[i + 1].data(), (uint32_t)s[i + 1].size(), qc, o, r1, r2);
            out(r1, i), out(r2, i + 1);
            uint32_t a, b1, b2;
            (void)np2srqc::judge_serial(s[i].data(), q[i].data(), (uint32_t)s[i].size(), qc, a, b1);
            const uint32_t n1 = b1 - a;
            (void)np2srqc::judge_serial(s[i + 1].data(), q[i + 1].data(), (uint32_t)s[i + 1].size(), qc, a, b2);
            t[T_PAIRS] += 1, t[T_PAIRS_OVERLAP] += r1.insert || r2.insert || r1.how == HOW_OVERLAP ? 1 : 0, t[T_PAIRS_UNSEARCHED] += past_cap(n1, b2 - a);
        } else {
            out(judge_single(s[i].data(), q[i].data(), (uint32_t)s[i].size(), qc, o), i);
        }
    }
    std::printf("totals");
    for (uint32_t i = 0; i < N_TOTALS; ++i) std::printf(" %llu", (unsigned long long)t[i]);
    std::printf("\n");
    return 0;
}
