// Host run of the depth report's per-record core (csrc/np2_depth_core.hpp): the CIGAR measure, the admission rule, the
// run rule and a serial difference-array model built on them, against hand-written cases; then the double predicate
// against the integer test 5 * aligned < 4 * read_len over pairs drawn up to 2^32 - 1.
//   depth_core_test            exit 0 and "ok <checks>" when every case holds; 1 and the failed case otherwise
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../nextpolish2_amd/csrc/np2_depth_core.hpp"

using np2depth::Measure;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        ++g_checks;                               \
        if (!(cond)) {                            \
            ++g_failed;                           \
            fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);         \
            fprintf(stderr, "\n");                \
        }                                         \
    } while (0)

static uint32_t op(char c, uint32_t len) {
    const char *ops = "MIDNSHP=X";
    uint32_t k = 0;
    while (ops[k] != c) ++k;
    return len << 4 | k;
}
static Measure measure(const std::vector<uint32_t> &cig) {
    Measure m;
    for (uint32_t w : cig) np2depth::add_op(m, w);
    return m;
}

struct Rec {
    int32_t pos;
    uint32_t flag, mapq;
    std::vector<uint32_t> cigar;
};
struct Rule {
    uint32_t exclude_flags = 0x4, min_mapq = 0;
    double min_fra = 0.8;
};
static bool is_counted(const Rec &r, const Rule &q = Rule()) {
    return np2depth::counted(r.flag, r.mapq, (uint32_t)r.cigar.size(), measure(r.cigar), q.exclude_flags, q.min_mapq, q.min_fra);
}
// depth[0, L) by +1 / -1 into L + 1 wrapping words and a running sum, as the kernels have it
static std::vector<uint32_t> depth_model(uint32_t L, const std::vector<Rec> &recs, const Rule &q = Rule()) {
    std::vector<uint32_t> diff(L + 1, 0);
    for (const Rec &r : recs) {
        uint32_t lo, hi;
        if (is_counted(r, q) && np2depth::cover(r.pos, measure(r.cigar).span, L, lo, hi)) diff[lo] += 1u, diff[hi] -= 1u;
    }
    uint32_t run = 0;
    for (uint32_t i = 0; i < L; ++i) diff[i] = run += diff[i];
    diff.resize(L);
    return diff;
}
struct Run {
    uint32_t s, e;
};
static std::vector<Run> runs_model(const std::vector<uint32_t> &depth, uint32_t min_depth, uint32_t min_len) {
    std::vector<Run> out;
    const uint32_t L = (uint32_t)depth.size();
    for (uint32_t i = 0; i < L;) {
        if (!np2depth::depth_ok(depth[i], min_depth)) {
            ++i;
            continue;
        }
        uint32_t e = i;
        while (e + 1 < L && np2depth::depth_ok(depth[e + 1], min_depth)) ++e;
        if (np2depth::run_kept(i, e, min_len)) out.push_back(Run{i, e});
        i = e + 1;
    }
    return out;
}

int main() {
    // every operation alone: (span, aligned, read_len) of 7 bases of it
    {
        const struct { char c; uint32_t span, aligned, read_len; } want[9] = {
            {'M', 7, 7, 7}, {'I', 0, 7, 7}, {'D', 7, 0, 0}, {'N', 7, 0, 0}, {'S', 0, 0, 7}, {'H', 0, 0, 7}, {'P', 0, 0, 0}, {'=', 7, 7, 7}, {'X', 7, 7, 7}};
        for (uint32_t k = 0; k < 9; ++k) {
            const uint32_t w = op(want[k].c, 7);
            CHECK((w & 15u) == k, "op code of %c", want[k].c);
            const Measure m = measure({w});
            CHECK(m.span == want[k].span && m.aligned == want[k].aligned && m.read_len == want[k].read_len, "measure of 7%c: %llu %llu %llu", want[k].c,
                  (unsigned long long)m.span, (unsigned long long)m.aligned, (unsigned long long)m.read_len);
        }
        for (uint32_t k = 9; k < 16; ++k) { // codes BAM does not define count in nothing
            const Measure m = measure({7u << 4 | k});
            CHECK(m.span == 0 && m.aligned == 0 && m.read_len == 0, "undefined op %u", k);
        }
        const Measure big = measure(std::vector<uint32_t>(65535, op('M', (1u << 28) - 1))); // the longest CIGAR a record holds
        CHECK(big.span == 65535ull * ((1u << 28) - 1), "sums are 64-bit");
    }
    // I counts in aligned but not in span; D and N the other way round; P in neither
    {
        const Measure m = measure({op('M', 10), op('I', 3), op('M', 10), op('D', 4), op('N', 5), op('P', 6), op('M', 1)});
        CHECK(m.span == 30 && m.aligned == 24 && m.read_len == 24, "mixed CIGAR: %llu %llu %llu", (unsigned long long)m.span, (unsigned long long)m.aligned,
              (unsigned long long)m.read_len);
    }
    // the admission rule at its boundaries
    CHECK(is_counted(Rec{0, 0, 0, {op('M', 80), op('S', 20)}}), "80M20S is counted (exactly 4/5)");
    CHECK(!is_counted(Rec{0, 0, 0, {op('M', 799), op('S', 201)}}), "799M201S is dropped");
    CHECK(is_counted(Rec{0, 0, 0, {op('M', 80), op('H', 20)}}), "80M20H is counted (hard clips count in the read length)");
    CHECK(!is_counted(Rec{0, 0, 0, {op('M', 80), op('H', 21)}}), "80M21H is dropped");
    CHECK(!is_counted(Rec{0, 0, 0, {}}), "an empty CIGAR is skipped");
    CHECK(!is_counted(Rec{0, 4, 0, {op('M', 10)}}), "flag & 4 is skipped");
    CHECK(is_counted(Rec{0, 0x900 | 0x400 | 0x200 | 0x10, 0, {op('M', 10)}}), "secondary, supplementary, duplicate, QC-fail are counted by default");
    {
        Rule q;
        q.exclude_flags = 0x904;
        CHECK(!is_counted(Rec{0, 0x100, 0, {op('M', 10)}}, q) && !is_counted(Rec{0, 0x800, 0, {op('M', 10)}}, q) && is_counted(Rec{0, 0x400, 0, {op('M', 10)}}, q),
              "exclude_flags 0x904");
        Rule m;
        m.min_mapq = 20;
        CHECK(!is_counted(Rec{0, 0, 19, {op('M', 10)}}, m) && is_counted(Rec{0, 0, 20, {op('M', 10)}}, m), "min_mapq 20");
        Rule z;
        z.min_fra = 0.0;
        CHECK(is_counted(Rec{0, 0, 0, {op('S', 10), op('D', 3)}}, z), "min_fra 0 keeps a record without aligned bases");
        CHECK(!is_counted(Rec{0, 0, 0, {op('D', 3)}}, z), "read_len 0 is skipped whatever the fraction");
        Rule o;
        o.min_fra = 1.0;
        CHECK(is_counted(Rec{0, 0, 0, {op('M', 10)}}, o) && !is_counted(Rec{0, 0, 0, {op('M', 999), op('S', 1)}}, o), "min_fra 1");
    }
    CHECK(np2depth::fra_ok(0.0) && np2depth::fra_ok(1.0) && np2depth::fra_ok(0.8), "fractions in [0, 1]");
    CHECK(!np2depth::fra_ok(-0.001) && !np2depth::fra_ok(1.001) && !np2depth::fra_ok(std::nan("")) && !np2depth::fra_ok(INFINITY), "fractions outside");
    // cover: clamped to the contig, one base for a span of 0, nothing for a start outside
    {
        uint32_t lo = 99, hi = 99;
        CHECK(np2depth::cover(5, 0, 20, lo, hi) && lo == 5 && hi == 6, "zero span covers one base");
        CHECK(np2depth::cover(15, 10, 20, lo, hi) && lo == 15 && hi == 20, "an overhang is clamped");
        CHECK(np2depth::cover(0, 20, 20, lo, hi) && lo == 0 && hi == 20, "the whole contig");
        CHECK(!np2depth::cover(-1, 10, 20, lo, hi) && !np2depth::cover(20, 1, 20, lo, hi) && !np2depth::cover(0, 1, 0, lo, hi), "starts outside [0, L)");
        CHECK(np2depth::cover(0x7FFFFFFF, 0xFFFFFFFFFull, 0xFFFF0000u, lo, hi) && lo == 0x7FFFFFFFu && hi == 0xFFFF0000u, "no 32-bit wrap at the end");
    }
    // the serial model on a contig of 20 positions
    {
        const std::vector<Rec> recs = {
            {0, 0, 0, {op('M', 5)}},                         // [0, 5)
            {3, 0, 0, {op('M', 2), op('D', 3), op('M', 2)}},  // [3, 10)
            {5, 0, 0, {op('I', 10)}},                         // zero span: position 5
            {15, 0, 0, {op('M', 10)}},                        // [15, 25) clamped to 20
            {19, 0, 0, {op('=', 1)}},                         // [19, 20)
            {8, 4, 0, {op('M', 10)}},                         // unmapped flag: skipped
            {8, 0, 0, {}},                                    // no CIGAR: skipped
            {8, 0, 0, {op('M', 10), op('S', 10)}},            // half aligned: dropped
            {-1, 0, 0, {op('M', 10)}},                        // outside
            {20, 0, 0, {op('M', 10)}},                        // outside
        };
        const std::vector<uint32_t> want = {1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2};
        const std::vector<uint32_t> got = depth_model(20, recs);
        CHECK(got == want, "depth of the hand-written contig");
        auto same = [](const std::vector<Run> &a, const std::vector<Run> &b) {
            if (a.size() != b.size()) return false;
            for (size_t i = 0; i < a.size(); ++i)
                if (a[i].s != b[i].s || a[i].e != b[i].e) return false;
            return true;
        };
        CHECK(same(runs_model(got, 1, 1), {{0, 9}, {15, 19}}), "runs at depth 1");
        CHECK(same(runs_model(got, 1, 5), {{0, 9}, {15, 19}}), "a run of exactly min_len is kept");
        CHECK(same(runs_model(got, 1, 6), {{0, 9}}), "a run of min_len - 1 is dropped");
        CHECK(same(runs_model(got, 2, 1), {{3, 5}, {19, 19}}), "runs at depth 2");
        CHECK(same(runs_model(got, 0, 1), {{0, 19}}), "min_depth 0: the whole contig");
        CHECK(same(runs_model(depth_model(20, {}), 0, 1), {{0, 19}}), "min_depth 0 without a record");
        CHECK(runs_model(got, 3, 1).empty(), "a threshold above the maximum");
        CHECK(runs_model(depth_model(0, recs), 0, 0).empty(), "L = 0 gives nothing");
        CHECK(np2depth::run_kept(0, 0xFFFFFFFEu, 0xFFFFFFFFu) && !np2depth::run_kept(1, 0xFFFFFFFEu, 0xFFFFFFFFu), "run lengths do not wrap");
    }
    // the double predicate equals 5a < 4b: around the boundary and at random, operands up to 2^32 - 1
    {
        uint64_t x = 0x9E3779B97F4A7C15ull;
        auto next = [&]() {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            return x;
        };
        uint32_t bad = 0, n = 0, near[3] = {0, 0, 0};
        auto one = [&](uint64_t a, uint64_t b) {
            if (b == 0 || a > 0xFFFFFFFFull || b > 0xFFFFFFFFull) return;
            ++n;
            if (np2depth::fra_below(a, b, 0.8) != (5 * a < 4 * b)) ++bad;
            const int64_t d = (int64_t)(5 * a) - (int64_t)(4 * b);
            if (d >= -1 && d <= 1) ++near[d + 1];
        };
        for (uint32_t i = 0; i < 2000000; ++i) {
            one(next() >> 32, next() >> 32);                       // anywhere
            const uint64_t b = (next() >> 32) | (i & 1 ? 0xF0000000ull : 0); // (half of them near the top of the range)
            const uint64_t a = 4 * b / 5;
            for (int64_t da = -1; da <= 1; ++da)                  // 5a - 4b in -9 .. 5 around the boundary
                one(a + (uint64_t)da, b);
        }
        // exact solutions of 5a - 4b = d: b = 5t - d, a = 4t - d
        for (uint32_t i = 0; i < 1000000; ++i) {
            const uint64_t t = 2 + next() % 858993458ull;
            for (int64_t d = -1; d <= 1; ++d) one(4 * t - (uint64_t)d, 5 * t - (uint64_t)d);
        }
        one(0xFFFFFFFFull, 0xFFFFFFFFull), one(0, 0xFFFFFFFFull), one(1, 1), one(0, 1), one(3435973836ull, 4294967295ull), one(3435973835ull, 4294967294ull);
        CHECK(bad == 0, "%u of %u pairs: the double predicate differs from 5a < 4b", bad, n);
        CHECK(near[0] > 100000 && near[1] > 100000 && near[2] > 100000, "pairs with 5a - 4b = -1, 0, 1: %u %u %u", near[0], near[1], near[2]);
    }
    if (g_failed) {
        fprintf(stderr, "%d of %d checks failed\n", g_failed, g_checks);
        return 1;
    }
    printf("ok %d\n", g_checks);
    return 0;
}
