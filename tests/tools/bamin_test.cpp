// The host twin of BAM input (nextpolish2_amd/csrc/np2_bamin_core.hpp: twin, the one-lane text of the rule that the kernels'
// lanes run) without a device or a file: hand-built streams, each in a heap buffer of exactly its bytes, so that a read beyond
// them is the address sanitizer's to catch.  Built with the address and undefined-behaviour sanitizers (tests/test_bamin_cpu.py).
//
//     bamin_test refusals | prefixes
//
// Prints "ok" and exits 0, or names the failed checks and exits 1.
#include "../../nextpolish2_amd/csrc/np2_bamin_core.hpp"

#include <cstdio>
#include <memory>

using namespace np2bamin;
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
static void cat(Bytes &b, const Bytes &x) { b.insert(b.end(), x.begin(), x.end()); }
static Bytes str(const char *s, size_t n) { return Bytes(s, s + n); }

static Bytes header() { // two references and a text with one carried line
    const std::string text = "@HD\tVN:1.6\n@SQ\tSN:c1\tLN:1000\n@PG\tID:x\n";
    Bytes h = str("BAM\1", 4);
    put32(h, (uint32_t)text.size());
    cat(h, str(text.data(), text.size()));
    put32(h, 2);
    put32(h, 3), cat(h, str("c1\0", 3)), put32(h, 1000);
    put32(h, 3), cat(h, str("c2\0", 3)), put32(h, 500);
    return h;
}
struct R {
    int32_t tid = 0, pos = 7, ntid = -1, npos = -1, tlen = 0;
    uint32_t flag = 0, l_seq = 4;
    Bytes name = str("q\0", 2), seq = {0x12, 0x48}, qual = {1, 2, 3, 4}, aux;
    std::vector<uint32_t> cigar = {4u << 4};
    int64_t block_size = -1, l_name = -1, n_cigar = -1;
    Bytes bytes() const {
        Bytes b;
        put32(b, (uint32_t)tid), put32(b, (uint32_t)pos);
        b.push_back((uint8_t)(l_name < 0 ? name.size() : (size_t)l_name)), b.push_back(60), put16(b, 0);
        put16(b, (uint32_t)(n_cigar < 0 ? cigar.size() : (size_t)n_cigar)), put16(b, flag), put32(b, l_seq);
        put32(b, (uint32_t)ntid), put32(b, (uint32_t)npos), put32(b, (uint32_t)tlen);
        cat(b, name);
        for (uint32_t w : cigar) put32(b, w);
        cat(b, seq), cat(b, qual), cat(b, aux);
        Bytes out;
        put32(out, block_size < 0 ? (uint32_t)b.size() : (uint32_t)block_size);
        cat(out, b);
        return out;
    }
};

// the twin on a heap copy of exactly s's bytes
static int run(const Bytes &s, uint32_t flags, Twin *t, std::string *bad) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[s.size() ? s.size() : 1]);
    if (!s.empty()) memcpy(exact.get(), s.data(), s.size());
    return twin(exact.get(), s.size(), flags, 1u, t, bad);
}

static void expect(const char *what, const R &r, uint32_t where) {
    for (int where_in_stream = 0; where_in_stream < 2; ++where_in_stream) { // as the last record, and with one behind it
        Bytes s = header();
        cat(s, R().bytes()), cat(s, r.bytes());
        if (where_in_stream) cat(s, R().bytes());
        Twin t;
        std::string bad;
        const int rc = run(s, KEEP_ALL, &t, &bad);
        const bool ok = rc == 0 && t.status.size() >= 2 && t.where[1] == where && t.speaks == (where ? 1 : -1) &&
                        t.status[1] == (where ? where_status(where) : 0);
        if (!ok) fprintf(stderr, "%s: rc %d, %zu records, where %u, speaks %lld\n", what, rc, t.status.size(), t.status.size() >= 2 ? t.where[1] : 99u, (long long)t.speaks);
        CHECK(ok);
        if (where != W_SHORT && where_in_stream) CHECK(t.status.size() == 3 && t.status[2] == 0 && t.recs.size() == (where ? 2u : 3u));
    }
}

static void refusals() {
    R r;
    expect("good", r, W_OK);
    r = R(), r.block_size = 31, expect("short", r, W_SHORT);
    r = R(), r.l_name = 255, expect("name overruns", r, W_OVERRUN);
    r = R(), r.n_cigar = 65535, expect("cigar overruns", r, W_OVERRUN);
    r = R(), r.l_seq = 0xFFFFFFFFu, expect("seq overruns", r, W_OVERRUN);
    r = R(), r.tid = 2, expect("refID", r, W_REFID);
    r = R(), r.tid = -2, expect("refID below", r, W_REFID);
    r = R(), r.pos = -2, expect("pos", r, W_POS);
    r = R(), r.cigar = {4u << 4 | 9u}, expect("cigar op", r, W_CIGAR);
    r = R(), r.cigar = {4u << 4 | 4u, 9u << 4 | 3u}, expect("CG", r, W_CG);
    r = R(), r.name = str("abc", 3), expect("name without NUL", r, W_NAME);
    r = R(), r.name = str("\0", 1), expect("empty name", r, W_NAME);
    r = R(), r.ntid = 2, expect("next_refID", r, W_NEXT_REFID);
    r = R(), r.npos = -2, expect("next_pos", r, W_NEXT_POS);
    r = R(), r.qual = {0, 94, 0, 0}, expect("quality", r, W_QUAL);
    r = R(), r.qual = {255, 255, 255, 0}, expect("quality partly 0xFF", r, W_QUAL);
    r = R(), r.qual = {255, 255, 255, 255}, expect("no quality", r, W_OK);
    r = R(), r.aux = str("NM", 2), expect("aux short", r, W_AUX);
    r = R(), r.aux = str("NMi\0\0\0", 6), expect("aux int cut", r, W_AUX);
    r = R(), r.aux = str("NMZabc", 6), expect("aux Z without NUL", r, W_AUX);
    r = R(), r.aux = str("XBBc\xff\xff\xff\xff\1", 9), expect("aux B count", r, W_AUX);
    r = R(), r.aux = str("XBBc\2\0\0\0\1", 9), expect("aux B cut", r, W_AUX);
    r = R(), r.aux = str("XBBs\1\0\0\0\1\2NMC\7XZZ\0", 18), expect("aux good", r, W_OK);
    // a header that stops anywhere
    const Bytes h = header();
    for (size_t n = 0; n < h.size(); ++n) {
        Twin t;
        std::string bad;
        CHECK(run(Bytes(h.begin(), h.begin() + n), KEEP_ALL, &t, &bad) == 1);
    }
    Twin t;
    std::string bad;
    CHECK(run(h, KEEP_ALL, &t, &bad) == 0 && t.refs.names.size() == 2 && t.refs.lens[1] == 500 && t.extra.size() == 1 && t.extra[0] == "@PG\tID:x");
}

static void prefixes() {
    R a, b, c;
    b.aux = str("NMC\7XZZabc\0", 11), b.tid = -1;
    c.name = str("longer name\0", 12), c.l_seq = 3, c.seq = {0x12, 0x4F}, c.qual = {9, 9, 9}, c.aux = str("XBBs\1\0\0\0\1\2", 10);
    const Bytes h = header(), ra = a.bytes(), rb = b.bytes(), rc = c.bytes();
    Bytes s = h;
    cat(s, ra), cat(s, rb), cat(s, rc);
    const size_t ends[4] = {h.size(), h.size() + ra.size(), h.size() + ra.size() + rb.size(), s.size()};
    for (uint32_t flags : {0u, KEEP_NAMES, KEEP_ALL})
        for (size_t n = h.size(); n <= s.size(); ++n) {
            Twin t;
            std::string bad;
            CHECK(run(Bytes(s.begin(), s.begin() + n), flags, &t, &bad) == 0);
            size_t whole = 0;
            while (whole < 3 && ends[whole + 1] <= n) ++whole;
            const size_t rest = n - ends[whole];
            CHECK(t.status.size() == whole + (rest ? 1u : 0u));
            if (rest && t.status.size() == whole + 1) CHECK(t.where[whole] == (rest < 4 ? W_GARBAGE : W_TRUNC) && t.speaks == (int64_t)whole);
            if (!rest) CHECK(t.speaks == -1);
            CHECK(t.recs.size() == (whole >= 3 ? 2u : whole >= 1 ? 1u : 0u)); // (the second record is unmapped)
            if (whole == 3) {
                CHECK(t.seq4.size() == 4 && t.seq4[3] == 0x40);
                if (flags & KEEP_ALL) CHECK(t.tails.size() % 4 == 0 && t.tail_ref.size() == 2 && (t.tail_ref[1] & 1u));
            }
        }
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "refusals") refusals();
    else if (what == "prefixes") prefixes();
    else return fprintf(stderr, "usage: bamin_test refusals | prefixes\n"), 2;
    if (!failures) printf("ok\n");
    return failures ? 1 : 0;
}
