// The BGZF header parser every reader shares (nextpolish2_amd/csrc/np2_bgzf.hpp) without a device or a file: hand-built
// headers, each in a heap buffer of exactly the bytes the parser is told it may read, so that a read beyond them is the
// address sanitizer's to catch.  Every case expects exact numbers, an exact message or an exact request for more bytes.
// Built with the address and undefined-behaviour sanitizers (tests/test_bgzf_cpu.py).
//
//     bgzf_test accept | reject | need
//
// Prints "ok" and exits 0, or names the failed checks and exits 1.
#include "../../nextpolish2_amd/csrc/np2_bgzf.hpp"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace np2h;
typedef std::vector<uint8_t> Bytes;

static int failures = 0;
#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

static void put16(Bytes &b, uint32_t v) { b.push_back(v & 255), b.push_back((v >> 8) & 255); }
static void put32(Bytes &b, uint32_t v) { put16(b, v & 0xFFFF), put16(b, v >> 16); }
static Bytes subfield(char a, char c, const Bytes &val) {
    Bytes s{(uint8_t)a, (uint8_t)c};
    put16(s, (uint32_t)val.size());
    s.insert(s.end(), val.begin(), val.end());
    return s;
}
static Bytes cat(std::initializer_list<Bytes> parts) {
    Bytes r;
    for (const Bytes &p : parts) r.insert(r.end(), p.begin(), p.end());
    return r;
}
// a block with this extra field and payload; bc_at: where in the extra field the BSIZE - 1 value lies (SIZE_MAX: nowhere)
static Bytes block(Bytes extra, size_t bc_at, const Bytes &payload, uint32_t crc, uint32_t isize) {
    const size_t bsize = 12 + extra.size() + payload.size() + 8;
    if (bc_at != SIZE_MAX) extra[bc_at] = (bsize - 1) & 255, extra[bc_at + 1] = (uint8_t)((bsize - 1) >> 8);
    Bytes b{31, 139, 8, 4, 0, 0, 0, 0, 0, 255};
    put16(b, (uint32_t)extra.size());
    b.insert(b.end(), extra.begin(), extra.end());
    b.insert(b.end(), payload.begin(), payload.end());
    put32(b, crc), put32(b, isize);
    return b;
}
static const Bytes BC = subfield('B', 'C', {0, 0});

// the first n bytes of v, alone on the heap
static std::unique_ptr<uint8_t[]> exactly(const Bytes &v, size_t n) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
    if (n) memcpy(p.get(), v.data(), n);
    return p;
}
static void expect_block(const Bytes &b, uint64_t left, uint32_t hdr_len, uint32_t bsize, uint32_t clen, uint32_t crc, uint32_t isize) {
    const auto p = exactly(b, b.size());
    const BgzfHeader h = bgzf_header(p.get(), b.size(), left);
    CHECK(h.need == 0 && h.hdr_len == hdr_len && h.bsize == bsize && h.clen == clen);
    // ... and from the header alone, the payload not in reach
    const auto q = exactly(b, hdr_len);
    const BgzfHeader h2 = bgzf_header(q.get(), hdr_len, left);
    CHECK(h2.need == 0 && h2.hdr_len == hdr_len && h2.bsize == bsize && h2.clen == clen);
    const auto t = exactly(Bytes(b.begin() + hdr_len + clen, b.end()), 8);
    const BgzfTrailer tr = bgzf_trailer(t.get());
    CHECK(tr.crc == crc && tr.isize == isize);
}
static void expect_error(const Bytes &b, size_t avail, uint64_t left, const char *msg) {
    const auto p = exactly(b, avail);
    try {
        (void)bgzf_header(p.get(), avail, left);
        CHECK(!"an error was expected");
    } catch (const Np2Error &e) {
        CHECK(e.code == NP2_E_ARG);
        if (strcmp(e.what(), msg) != 0) {
            fprintf(stderr, "expected \"%s\", got \"%s\"\n", msg, e.what());
            ++failures;
        }
    }
}
static void expect_need(const Bytes &b, size_t avail, uint64_t left, uint32_t need) {
    const auto p = exactly(b, avail);
    const BgzfHeader h = bgzf_header(p.get(), avail, left);
    CHECK(h.need == need);
}

static const Bytes STORED_A{1, 1, 0, 0xFE, 0xFF, 'A'}; // a stored DEFLATE block of one byte
static const uint32_t CRC_A = 0xD3D99E8Bu;               // CRC-32 of "A"

static void accept() {
    // the end-of-file marker, byte for byte
    const Bytes eof{31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(eof.size() == 28);
    expect_block(eof, 28, 18, 28, 2, 0, 0);
    CHECK(block(BC, 4, {3, 0}, 0, 0) == eof); // (the builder writes what the format says)
    // a stored block of 1 byte
    expect_block(block(BC, 4, STORED_A, CRC_A, 1), 32, 18, 32, 6, CRC_A, 1);
    expect_block(block(BC, 4, STORED_A, CRC_A, 1), 1000, 18, 32, 6, CRC_A, 1); // (other blocks follow)
    // BC preceded by another subfield, and followed by one
    const Bytes xy = subfield('X', 'Y', {7, 8, 9});
    expect_block(block(cat({xy, BC, xy}), 7 + 4, STORED_A, CRC_A, 1), 46, 12 + 20, 46, 6, CRC_A, 1);
    // BC as the last subfield, ending exactly at XLEN
    expect_block(block(cat({xy, BC}), 7 + 4, STORED_A, CRC_A, 1), 39, 12 + 13, 39, 6, CRC_A, 1);
    // BC with SLEN 3 is not the block size: the BC with SLEN 2 behind it is
    const Bytes bc3 = subfield('B', 'C', {0xFF, 0xFF, 0xFF});
    expect_block(block(cat({bc3, BC}), 7 + 4, STORED_A, CRC_A, 1), 39, 12 + 13, 39, 6, CRC_A, 1);
    // XLEN 300: a subfield of 290 bytes in front of BC
    const Bytes big = subfield('Z', 'Z', Bytes(290, 0x42));
    const Bytes b300 = block(cat({big, BC}), 294 + 4, STORED_A, CRC_A, 1);
    CHECK(b300[10] == (300 & 255) && b300[11] == (300 >> 8));
    expect_block(b300, b300.size(), 312, 326, 6, CRC_A, 1);
}

static void reject() {
    const Bytes good = block(BC, 4, STORED_A, CRC_A, 1);
    const Bytes xy = subfield('X', 'Y', {7, 8});
    // a BC header whose two value bytes would lie beyond XLEN (the payload's first bytes stand where they would be)
    {
        Bytes b = block(cat({xy, Bytes{'B', 'C', 2, 0}}), SIZE_MAX, Bytes{0x30, 0x00, 1, 2, 3}, 0, 0);
        expect_error(b, 12 + 10, b.size(), "BGZF block without BC field"); // (the header alone: nothing behind XLEN to read)
        expect_error(b, b.size(), b.size(), "BGZF block without BC field");
        // ... and as the only subfield: XLEN 4
        Bytes c = block(Bytes{'B', 'C', 2, 0}, SIZE_MAX, Bytes{0x30, 0x00, 1, 2, 3}, 0, 0);
        expect_error(c, 18, c.size(), "BGZF block without BC field");
    }
    // BC with SLEN 3, and nothing else
    expect_error(block(subfield('B', 'C', {31, 0, 0}), SIZE_MAX, STORED_A, CRC_A, 1), 12 + 7, 33, "BGZF block without BC field");
    // XLEN 0
    expect_error(block({}, SIZE_MAX, STORED_A, CRC_A, 1), 18, 26, "BGZF block without BC field");
    // 17 bytes
    expect_error(good, 17, 17, "not a BGZF block");
    expect_error(good, 0, 0, "not a BGZF block");
    // the extra field cut short by the end of the data: 12 + XLEN - 1 bytes
    const Bytes b300 = block(cat({subfield('Z', 'Z', Bytes(290, 0x42)), BC}), 294 + 4, STORED_A, CRC_A, 1);
    expect_error(b300, 311, 311, "truncated BGZF header");
    expect_error(b300, 18, 311, "truncated BGZF header"); // (known from the first 18 bytes)
    const Bytes b13 = block(cat({subfield('X', 'Y', {7, 8, 9}), BC}), 7 + 4, STORED_A, CRC_A, 1);
    expect_error(b13, 24, 24, "truncated BGZF header");
    // BSIZE = 12 + XLEN + 7: no room for the trailer
    {
        Bytes b = good;
        b[16] = 12 + 6 + 7 - 1, b[17] = 0;
        expect_error(b, b.size(), b.size(), "truncated BGZF block");
        b[16] = 0; // BSIZE 1
        expect_error(b, b.size(), b.size(), "truncated BGZF block");
    }
    // BSIZE one more than the bytes left
    expect_error(good, good.size() - 1, good.size() - 1, "truncated BGZF block");
    expect_error(good, 18, good.size() - 1, "truncated BGZF block");
    // each of the magic and flag bytes wrong in turn
    for (int i = 0; i < 4; ++i) {
        Bytes b = good;
        b[i] = i == 3 ? (uint8_t)(b[i] & ~4) : (uint8_t)(b[i] + 1);
        expect_error(b, b.size(), b.size(), "not a BGZF block");
    }
    { // (FEXTRA among other flags is fine; other flags without it are not)
        Bytes b = good;
        b[3] = 0xFB;
        expect_error(b, b.size(), b.size(), "not a BGZF block");
    }
}

static void need() {
    const Bytes good = block(BC, 4, STORED_A, CRC_A, 1);
    // a header fed in two parts: 18 bytes first, then 12 + XLEN
    expect_need(good, 10, good.size(), 18);
    expect_need(good, 0, good.size(), 18);
    expect_need(good, 17, good.size(), 18);
    expect_block(good, good.size(), 18, 32, 6, CRC_A, 1); // (XLEN 6: the 18 bytes are the header)
    const Bytes b300 = block(cat({subfield('Z', 'Z', Bytes(290, 0x42)), BC}), 294 + 4, STORED_A, CRC_A, 1);
    expect_need(b300, 5, b300.size(), 18);
    expect_need(b300, 18, b300.size(), 312);
    expect_need(b300, 311, b300.size(), 312);
    const auto p = exactly(b300, 312);
    const BgzfHeader h = bgzf_header(p.get(), 312, b300.size());
    CHECK(h.need == 0 && h.hdr_len == 312 && h.bsize == 326 && h.clen == 6);
    // bad magic is seen before more bytes are asked for
    Bytes bad = b300;
    bad[1] = 0;
    expect_error(bad, 18, bad.size(), "not a BGZF block");
}

int main(int argc, char **argv) {
    const std::string s = argc > 1 ? argv[1] : "";
    try {
        if (s == "accept") accept();
        else if (s == "reject") reject();
        else if (s == "need") need();
        else {
            fprintf(stderr, "usage: bgzf_test accept | reject | need\n");
            return 2;
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 1;
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
