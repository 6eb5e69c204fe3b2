// The per-lane logic of NP2_SAM_KEEP_ALL (csrc/np2_samtail_core.hpp) as a one-lane host program, for tests/test_bamfull_cpu.py:
//   samtail_core_test FILE
// walks FILE the way np2_sam_tails_host does (header lines, then every line through parse_line and tail_line) and prints per
// line behind the header:  S (no byte) | L <code> (the lean parse refuses it) | U (not kept) | E <error word> |
// T <has_qual> <aux_len> <the tail, hex>.  The text and every tail lie in heap blocks of exactly their size, so that a read or
// a write one byte outside them is the address sanitizer's to find.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../nextpolish2_amd/csrc/np2_samtail_core.hpp"

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: samtail_core_test FILE\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    std::vector<uint8_t> in;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
    if (!in.empty() && in.back() != '\n') in.push_back('\n'); // a last line needs no newline
    const size_t n = in.size();
    uint8_t *text = (uint8_t *)malloc(n ? n : 1);
    memcpy(text, in.data(), n);

    np2sam::Refs refs;
    size_t at = 0;
    while (at < n) { // the header
        const size_t nl = (const uint8_t *)memchr(text + at, '\n', n - at) - text;
        const size_t end = nl > at && text[nl - 1] == '\r' ? nl - 1 : nl;
        if (end > at && text[at] != '@') break;
        if (end > at && !np2sam::header_line(text, at, end, refs).empty()) {
            printf("HERR\n");
            free(text);
            return 0;
        }
        at = nl + 1;
    }
    const np2sam::NameTabHost tab(refs);
    const np2sam::NameTab nt = tab.view();
    while (at < n) {
        const size_t nl = (const uint8_t *)memchr(text + at, '\n', n - at) - text;
        const size_t end = nl > at && text[nl - 1] == '\r' ? nl - 1 : nl;
        const uint32_t e = (uint32_t)(end - at);
        std::unique_ptr<uint8_t, void (*)(void *)> own((uint8_t *)malloc(e ? e : 1), free); // the line alone, in a block of its size
        memcpy(own.get(), text + at, e);
        const uint8_t *line = own.get();
        const np2sam::Line ln = np2sam::parse_line(line, 0, e, nt);
        at = nl + 1;
        if (ln.tid == np2sam::TID_EMPTY_LINE) {
            printf("S\n");
        } else if (ln.err != np2sam::OK) {
            printf("L\t%u\n", (unsigned)ln.err);
        } else if (!np2sam::line_kept(ln)) {
            printf("U\n");
        } else {
            uint32_t size = 0, aux = 0;
            bool hq = false;
            const uint32_t w = np2tail::tail_line(line, e, ln, nt, &size, &aux, &hq, nullptr);
            if (w) {
                printf("E\t%u\n", w);
                continue;
            }
            uint8_t *out = (uint8_t *)malloc(np2tail::pad4(size));
            uint32_t size2 = 0, aux2 = 0;
            bool hq2 = false;
            if (np2tail::tail_line(line, e, ln, nt, &size2, &aux2, &hq2, out) != 0u || size2 != size || aux2 != aux || hq2 != hq) {
                fprintf(stderr, "the two walks of one line differ\n");
                return 1;
            }
            printf("T\t%d\t%u\t", hq ? 1 : 0, aux);
            for (uint32_t i = 0; i < np2tail::pad4(size); ++i) printf("%02x", out[i]);
            printf("\n");
            free(out);
        }
    }
    free(text);
    return 0;
}
