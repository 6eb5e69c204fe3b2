// Host run of the edit rule's one-lane program (csrc/np2_edits_core.hpp: edits_host), the text the kernels of
// np2_edits.hip share.  Stand-alone, so that it runs under a host sanitizer.
//   edits_core_test CASE       CASE: uint32 L, uint32 n, ref[L], bases[n], uint32 pos[n] (little endian)
// prints "ERR <word>" for a violated precondition, else one line per edit
//   E ref_pos ref_len out_off alt_len kind REF ALT        ('.' for an empty string)
// and a last line
//   T has_span first last raw_runs same_runs snv mnv ins del cpx bases_inserted bases_deleted outside
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../nextpolish2_amd/csrc/np2_edits_core.hpp"

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: edits_core_test CASE\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    uint32_t hd[2] = {0, 0};
    if (fread(hd, 4, 2, f) != 2) return 2;
    const uint32_t L = hd[0], n = hd[1];
    std::vector<uint8_t> ref(L), bases(n);
    std::vector<uint32_t> pos(n);
    if ((L && fread(ref.data(), 1, L, f) != L) || (n && fread(bases.data(), 1, n, f) != n) || (n && fread(pos.data(), 4, n, f) != n)) {
        fprintf(stderr, "short case file\n");
        return 2;
    }
    fclose(f);
    const np2edits::HostResult h = np2edits::edits_host(ref.data(), L, bases.data(), pos.data(), n);
    if (h.err) {
        printf("ERR %u\n", h.err);
        return 0;
    }
    for (size_t i = 0; i < h.edits.size(); ++i) {
        const np2edits::Edit &e = h.edits[i];
        std::string r(h.ref_pool.begin() + h.ref_off[i], h.ref_pool.begin() + h.ref_off[i + 1]);
        std::string a(h.alt_pool.begin() + h.alt_off[i], h.alt_pool.begin() + h.alt_off[i + 1]);
        printf("E %u %u %u %u %u %s %s\n", e.ref_pos, e.ref_len, e.out_off, e.alt_len, e.kind, r.empty() ? "." : r.c_str(), a.empty() ? "." : a.c_str());
    }
    const np2edits::Totals &t = h.t;
    printf("T %u %u %u %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", t.has_span, t.first, t.last, (unsigned long long)t.raw_runs,
           (unsigned long long)t.same_runs, (unsigned long long)t.n_kind[0], (unsigned long long)t.n_kind[1], (unsigned long long)t.n_kind[2],
           (unsigned long long)t.n_kind[3], (unsigned long long)t.n_kind[4], (unsigned long long)t.bases_inserted,
           (unsigned long long)t.bases_deleted, (unsigned long long)t.outside);
    return 0;
}
