// Host twin of the GPU CRC kernel (csrc/np2_crc32.hip: k_bgzf_crc32): the SAME piece layout, table steps, mulmod and fold
// (csrc/np2_crc32_core.hpp) with one lane playing all 64, against crc32() of zlib on the lengths where the layout has its
// edges (empty, shorter than a 16-byte load, around one piece, around two, one short of the frame, the whole frame) and on
// seeded random lengths, over zeros, 0xFF, random bytes and packed nucleotides.
// Built and run by tests/test_crc32_cpu.py; prints the number of buffers checked.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include <zlib.h>
#include "../../nextpolish2_amd/csrc/np2_crc32_core.hpp"

using namespace np2crc;

static int fails = 0;
static void expect(bool ok, const char *what, uint32_t a, uint32_t b) {
    if (ok) return;
    if (++fails <= 20) fprintf(stderr, "FAIL %s: %08x vs %08x\n", what, a, b);
}

int main() {
    // mulmod: a zero operand gives zero (and the call returns); x^0 is the unit; it commutes; the fold constants are what
    // 8192 * 2^s division steps make of x^0
    std::mt19937 rng(20240611u);
    for (int i = 0; i < 1000; ++i) {
        const uint32_t a = rng(), b = rng();
        expect(mulmod(0u, a) == 0u && mulmod(a, 0u) == 0u, "mulmod zero", mulmod(0u, a), mulmod(a, 0u));
        expect(mulmod(0x80000000u, a) == a && mulmod(a, 0x80000000u) == a, "mulmod unit", mulmod(0x80000000u, a), a);
        expect(mulmod(a, b) == mulmod(b, a), "mulmod commutes", mulmod(a, b), mulmod(b, a));
        expect(mulmod(a, 0x40000000u) == shift_bits(a, 1u), "mulmod by x", mulmod(a, 0x40000000u), shift_bits(a, 1u));
    }
    for (uint32_t s = 0; s < 6; ++s) expect(fold_const(s) == shift_bits(0x80000000u, 8192u << s), "fold constant", fold_const(s), shift_bits(0x80000000u, 8192u << s));
    // the combine rule itself, on pieces of any length: reg(A || B) = mulmod(reg(A), x^(8 |B|)) ^ reg0(B)
    for (int i = 0; i < 200; ++i) {
        std::vector<uint8_t> d(1 + rng() % 5000);
        for (auto &c : d) c = (uint8_t)rng();
        const uint32_t cut = rng() % (uint32_t)(d.size() + 1), nb = (uint32_t)d.size() - cut;
        uint32_t ra = 0xFFFFFFFFu, rb = 0u;
        for (uint32_t k = 0; k < cut; ++k) ra = step1(TABLES.t, ra, d[k]);
        for (uint32_t k = cut; k < d.size(); ++k) rb = step1(TABLES.t, rb, d[k]);
        const uint32_t got = ~(mulmod(ra, shift_bits(0x80000000u, 8u * nb)) ^ rb);
        expect(got == (uint32_t)crc32(0L, d.data(), (uInt)d.size()), "combine rule", got, (uint32_t)crc32(0L, d.data(), (uInt)d.size()));
    }

    std::vector<uint32_t> lens = {0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 65279, 65280, 65535, 65536};
    for (int i = 0; i < 300; ++i) lens.push_back(rng() % 65537u);
    for (int i = 0; i < 100; ++i) lens.push_back(rng() % 3000u);
    size_t checked = 0;
    std::vector<uint8_t> store(65536 + 64);
    for (uint32_t n : lens) {
        for (int kind = 0; kind < 4; ++kind) {
            // (the data at a different misalignment each time: the 16-byte loads are unaligned ones)
            uint8_t *d = store.data() + (checked % 16);
            for (uint32_t k = 0; k < n; ++k) {
                if (kind == 0) d[k] = 0;
                else if (kind == 1) d[k] = 0xFF;
                else if (kind == 2) d[k] = (uint8_t)rng();
                else d[k] = (uint8_t)((1u << (rng() & 3u)) << 4 | (1u << (rng() & 3u))); // BAM's 4-bit nucleotides: 1, 2, 4, 8
            }
            const uint32_t want = (uint32_t)crc32(0L, d, (uInt)n);
            expect(crc32_by_pieces(d, n) == want, "64 pieces + fold", crc32_by_pieces(d, n), want);
            expect(crc32_serial(d, n) == want, "serial", crc32_serial(d, n), want);
            ++checked;
        }
    }
    if (fails) {
        fprintf(stderr, "%d failures\n", fails);
        return 1;
    }
    printf("%zu buffers checked\n", checked);
    return 0;
}
