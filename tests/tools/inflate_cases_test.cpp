// The hand-built DEFLATE streams of tests/inflate_cases.py through the stream loop of the GPU inflater
// (csrc/np2_inflate_core.hpp: inflate_stream) with the one-lane machine of inflate_core_test.cpp, built under the address and
// undefined-behaviour sanitizers by tests/test_inflate_cases_cpu.py.  The output buffer of a case is a heap block of exactly
// ISIZE bytes: a stream, malformed or not, that writes past its ISIZE or reads before its output ends the program.
// argv[1]: records of '<II' clen, isize and the payload.  Prints "status crc32" per record (the CRC of the ISIZE bytes
// where the status is 0, else 0).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <zlib.h>
#include "../../nextpolish2_amd/csrc/np2_inflate_core.hpp"

using namespace np2inf;

struct HostMachine {
    const uint8_t *in;
    uint32_t clen;
    uint8_t *out; // exactly isize bytes
    uint8_t lens_[384];
    uint32_t lt[1 << LBITS], dt[1 << DBITS];
    uint16_t ls[MAXL], ds[MAXD], sc[MAXBITS + 2];
    Code lc, dc;
    uint32_t uni(uint32_t v) { return v; }
    bool leader() { return true; }
    uint32_t lane() { return 0; }
    uint32_t lanes() { return 1; }
    void sync() {}
    uint32_t in32(uint32_t off) {
        uint32_t v = 0;
        for (int i = 0; i < 4; ++i)
            if (off + i < clen) v |= (uint32_t)in[off + i] << (8 * i);
        return v;
    }
    void put(uint32_t o, uint32_t b) { out[o] = (uint8_t)b; }
    uint32_t lit_room(uint32_t o, uint32_t isize) { return isize - o < 64u - (o & 63u) ? isize - o : 64u - (o & 63u); } // (the device's rule)
    void put_fast(uint32_t o, uint32_t b) { out[o] = (uint8_t)b; }
    void copy(uint32_t o, uint32_t len, uint32_t dist) {
        for (uint32_t k = 0; k < len; ++k) out[o + k] = out[o - dist + (dist >= len ? k : k % dist)];
    }
    uint32_t fast(uint64_t &, uint32_t &, uint32_t &, uint32_t &, uint32_t, uint32_t) { return ST_OK; } // (no wide step)
    void tick(int) {}
    uint32_t slow(int mode, uint32_t bits) { return mode == MODE_LITLEN ? code_slow(lc, ls, bits, mode) : code_slow(dc, ds, bits, mode); }
    uint8_t *lens() { return lens_; }
    uint32_t *lit_table() { return lt; }
    uint32_t *dist_table() { return dt; }
    uint16_t *lit_sym() { return ls; }
    uint16_t *dist_sym() { return ds; }
    uint16_t *scratch16() { return sc; }
    Code &lit_code() { return lc; }
    Code &dist_code() { return dc; }
};

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t h[2];
    while (fread(h, 4, 2, f) == 2) {
        const uint32_t clen = h[0], isize = h[1];
        if (clen > 65536u || isize > 65536u) return 2; // (the kernel refuses such a block before it looks at its bytes)
        uint8_t *z = (uint8_t *)malloc(clen); // (exactly clen bytes too: reads beyond the payload are the machine's to refuse)
        if (clen && fread(z, 1, clen, f) != clen) return 2;
        uint8_t *out = (uint8_t *)malloc(isize); // (ISIZE 0: a block of no bytes, every access to it is reported)
        if (isize) memset(out, 0xA5, isize);
        HostMachine *m = new HostMachine;
        m->in = z, m->clen = clen, m->out = out;
        const uint32_t st = inflate_stream(*m, clen, isize);
        printf("%u %lu\n", st, st == ST_OK ? (unsigned long)crc32(crc32(0L, Z_NULL, 0), out, isize) : 0ul);
        delete m;
        free(out);
        free(z);
    }
    fclose(f);
    return 0;
}
