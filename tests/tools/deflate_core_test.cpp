// The DEFLATE encoder core (csrc/np2_deflate_core.hpp) as a plain host program that steps the 64 lanes of every phase in
// turn, against zlib's inflater.  Built with -fsanitize=address,undefined: the output buffer is exactly one BGZF slot and
// the token scratch exactly TOK_WORDS words, so a write past either is reported.
//   deflate_core_test CORPUS     CORPUS: cases as [uint32 n][n bytes] ...; prints the number of cases that checked out
// Every case is encoded at each byte alignment of the stream's first bit inside its word (and at a BGZF block's, 144), over scratch and output filled
// with two different bytes: the streams must be identical (nothing is read that this call did not write), at most n + 5
// bytes, and inflate to the input with zlib, which must end exactly at the stream's last byte.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <zlib.h>
#include "../../nextpolish2_amd/csrc/np2_deflate_core.hpp"

static std::vector<uint8_t> encode(const std::vector<uint8_t> &in, uint32_t bit0, int poison) {
    std::vector<uint32_t> words(np2def::SLOT_BYTES / 4), tok(np2def::TOK_WORDS);
    memset(words.data(), poison, words.size() * 4);
    memset(tok.data(), poison, tok.size() * 4);
    // (the input in a buffer of its own exact size: a read past it is reported)
    std::vector<uint8_t> src(in);
    np2def::HostMachine m;
    memset(&m, poison, sizeof m);
    np2def::Shared *S = (np2def::Shared *)malloc(sizeof(np2def::Shared));
    memset(S, poison, sizeof *S);
    const uint32_t n = np2def::deflate_block(m, *S, src.data(), (uint32_t)src.size(), words.data(), bit0, tok.data());
    free(S);
    const uint8_t *p = (const uint8_t *)words.data() + bit0 / 8;
    return std::vector<uint8_t>(p, p + n);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int cases = 0;
    for (;;) {
        uint32_t n;
        if (fread(&n, 4, 1, f) != 1) break;
        if (n > np2def::MAX_BLOCK) return 3;
        std::vector<uint8_t> in(n);
        if (n && fread(in.data(), 1, n, f) != n) return 3;
        std::vector<uint8_t> ref;
        for (uint32_t bit0 : {0u, 8u, 16u, 24u, 144u})
            for (int poison : {0x00, 0xA5}) {
                std::vector<uint8_t> z = encode(in, bit0, poison);
                if (z.size() > (size_t)n + 5) {
                    fprintf(stderr, "case %d (n = %u): %zu bytes, more than n + 5\n", cases, n, z.size());
                    return 1;
                }
                if (bit0 == 0 && poison == 0) ref = z;
                else if (z != ref) {
                    fprintf(stderr, "case %d (n = %u): the stream depends on alignment %u or on what memory held (%#x)\n", cases, n, bit0, poison);
                    return 1;
                }
            }
        std::vector<uint8_t> back(n + 16);
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) return 4;
        zs.next_in = ref.data(), zs.avail_in = (uInt)ref.size();
        zs.next_out = back.data(), zs.avail_out = (uInt)back.size();
        const int rc = inflate(&zs, Z_FINISH);
        const bool ok = rc == Z_STREAM_END && zs.total_out == n && zs.avail_in == 0 && (n == 0 || memcmp(back.data(), in.data(), n) == 0);
        inflateEnd(&zs);
        if (!ok) {
            fprintf(stderr, "case %d (n = %u): zlib: rc %d, %lu bytes out, %u bytes of %zu left (%s)\n", cases, n, rc, zs.total_out, zs.avail_in, ref.size(), zs.msg ? zs.msg : "");
            return 1;
        }
        ++cases;
    }
    fclose(f);
    printf("%d\n", cases);
    return 0;
}
