// The .bai parser of the product (csrc/np2_bai_core.hpp) as a stand-alone program, for the address and undefined-behaviour
// sanitizers (tests/test_bai_forms_cpu.py builds and runs it).  Every parse gets its bytes in a heap block of exactly their
// length, so that a read past them is a report.
//   bai_core_test <file.bai> <n_ref of the BAM> parse         the derived values: per reference "ref r start end n_intv",
//                                                             "lin r v ..." and "zone r v ..." (bai_zone_start at every
//                                                             window boundary 0, 16384, ... up to one past the last window)
//   ...                                        truncations   every prefix of 0 .. n-1 bytes: "parsed k" for those that parse
//   ...                                        counts        each of n_ref, every n_bin, n_chunk and n_intv overwritten with
//                                                             0x7FFFFFFF and 0xFFFFFFFF: "parsed <field> <offset> <value>" for
//                                                             those that parse
// The last line is "done <number of parses>".
#include "np2_bai_core.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

static const char *parse_copy(const uint8_t *d, size_t n, uint32_t n_ref, np2h::BaiIndex &out) {
    std::unique_ptr<uint8_t[]> heap(new uint8_t[n]); // (n == 0: a block of no bytes)
    if (n) memcpy(heap.get(), d, n);
    return np2h::bai_parse(heap.get(), n, n_ref, out);
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> d;
    for (int c; (c = fgetc(f)) != EOF;) d.push_back((uint8_t)c);
    fclose(f);
    const uint32_t n_ref = (uint32_t)strtoul(argv[2], nullptr, 10);
    const std::string cmd = argv[3];
    np2h::BaiIndex ix;
    if (cmd == "parse") {
        if (const char *why = parse_copy(d.data(), d.size(), n_ref, ix)) {
            printf("error %s\n", why);
            return 0;
        }
        for (uint32_t r = 0; r < n_ref; ++r) {
            printf("ref %u %" PRIu64 " %" PRIu64 " %zu\n", r, ix.ref_start[r], ix.ref_end[r], ix.lin[r].size());
            printf("lin %u", r);
            for (uint64_t v : ix.lin[r]) printf(" %" PRIu64, v);
            printf("\nzone %u", r);
            for (size_t w = 0; w <= ix.lin[r].size() + 1; ++w) printf(" %" PRIu64, np2h::bai_zone_start(ix.lin[r], ix.ref_start[r], (uint32_t)(w << 14)));
            printf("\n");
        }
        printf("done 1\n");
        return 0;
    }
    if (cmd == "truncations") {
        for (size_t k = 0; k < d.size(); ++k)
            if (!parse_copy(d.data(), k, n_ref, ix)) printf("parsed %zu\n", k);
        printf("done %zu\n", d.size());
        return 0;
    }
    if (cmd == "counts") {
        if (parse_copy(d.data(), d.size(), n_ref, ix)) return 3; // (the file itself must be whole: its fields are found by walking it)
        std::vector<std::pair<std::string, size_t>> fields{{"n_ref", 4}};
        size_t p = 8;
        const uint32_t n_ref_i = np2h::bai_le32(d.data() + 4);
        for (uint32_t r = 0; r < n_ref_i; ++r) {
            fields.emplace_back("n_bin", p);
            const uint32_t n_bin = np2h::bai_le32(d.data() + p);
            p += 4;
            for (uint32_t b = 0; b < n_bin; ++b) {
                fields.emplace_back("n_chunk", p + 4);
                p += 8 + (size_t)np2h::bai_le32(d.data() + p + 4) * 16;
            }
            fields.emplace_back("n_intv", p);
            p += 4 + (size_t)np2h::bai_le32(d.data() + p) * 8;
        }
        size_t n = 0;
        for (const auto &fl : fields)
            for (uint32_t v : {0x7FFFFFFFu, 0xFFFFFFFFu}) {
                std::vector<uint8_t> e(d);
                for (int k = 0; k < 4; ++k) e[fl.second + k] = (uint8_t)(v >> (8 * k));
                if (!parse_copy(e.data(), e.size(), n_ref, ix)) printf("parsed %s %zu %u\n", fl.first.c_str(), fl.second, v);
                ++n;
            }
        printf("done %zu\n", n);
        return 0;
    }
    return 2;
}
