// The per-lane logic of the SAM reader (csrc/np2_sam_core.hpp) as a one-lane host program, for tests/test_sam_cpu.py:
//   sam_core_test FILE TIE
// walks FILE the way the reader does (header lines on the host, then every line through parse_line / pack_line) and prints
//   REFS <name>:<len>,...
//   then per line behind the header:  S  (no byte)  |  E <code>  |  R <kept> <tid> <pos> <flag> <mapq> <n_cigar> <l_seq> <key> <words,> <seq4 hex>
// or, for a header line that is refused,  HERR <1-based line> <message>  and nothing more.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../nextpolish2_amd/csrc/np2_sam_core.hpp"

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: sam_core_test FILE TIE\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    std::vector<uint8_t> text;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.insert(text.end(), buf, buf + got);
    fclose(f);
    if (!text.empty() && text.back() != '\n') text.push_back('\n'); // a last line needs no newline
    const uint32_t tie = (uint32_t)atoi(argv[2]);

    np2sam::Refs refs;
    size_t at = 0, line_no = 0;
    while (at < text.size()) { // the header
        const size_t nl = (const uint8_t *)memchr(text.data() + at, '\n', text.size() - at) - text.data();
        const size_t end = nl > at && text[nl - 1] == '\r' ? nl - 1 : nl;
        if (end > at && text[at] != '@') break;
        if (end > at) {
            const std::string bad = np2sam::header_line(text.data(), at, end, refs);
            if (!bad.empty()) {
                printf("HERR\t%zu\t%s\n", line_no + 1, bad.c_str());
                return 0;
            }
        }
        at = nl + 1, ++line_no;
    }
    printf("REFS\t");
    for (size_t i = 0; i < refs.names.size(); ++i) printf("%s%s:%u", i ? "," : "", refs.names[i].c_str(), refs.lens[i]);
    printf("\n");
    const np2sam::NameTabHost tab(refs);
    const np2sam::NameTab nt = tab.view();
    std::vector<uint32_t> cigar;
    std::vector<uint8_t> seq4;
    while (at < text.size()) {
        const size_t nl = (const uint8_t *)memchr(text.data() + at, '\n', text.size() - at) - text.data();
        const size_t end = nl > at && text[nl - 1] == '\r' ? nl - 1 : nl;
        const np2sam::Line ln = np2sam::parse_line(text.data(), (uint32_t)at, (uint32_t)end, nt);
        at = nl + 1;
        if (ln.tid == np2sam::TID_EMPTY_LINE) {
            printf("S\n");
            continue;
        }
        if (ln.err != np2sam::OK) {
            printf("E\t%u\n", (unsigned)ln.err);
            continue;
        }
        cigar.assign(ln.n_cigar, 0u), seq4.assign((ln.l_seq + 1u) / 2u, 0);
        np2sam::pack_line(text.data(), ln, cigar.data(), seq4.data());
        const bool kept = np2sam::line_kept(ln);
        printf("R\t%d\t%d\t%d\t%u\t%u\t%u\t%u\t%llu\t", kept ? 1 : 0, ln.tid, ln.pos, (unsigned)ln.flag, (unsigned)ln.mapq, ln.n_cigar, ln.l_seq,
               kept ? (unsigned long long)np2sam::sort_key(ln.tid, ln.pos, ln.flag, tie) : 0ull);
        for (size_t i = 0; i < cigar.size(); ++i) printf("%s%u", i ? "," : "", cigar[i]);
        printf("\t");
        for (uint8_t b : seq4) printf("%02x", b);
        printf("\n");
    }
    return 0;
}
