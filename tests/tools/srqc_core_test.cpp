// The short-read quality rule's core (csrc/np2_srqc_core.hpp) as a stand-alone host program: judge_serial against a
// brute-force restatement of the rule (every window summed from scratch) on the boundary cases, and known answers.
// Built with -fsanitize=address,undefined by tests/test_srqc_cpu.py; prints "ok <cases>".
#include "../../nextpolish2_amd/csrc/np2_srqc_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace np2srqc;

static int n_cases = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                              \
        }                                                              \
    } while (0)

struct Res {
    uint32_t a, b, cls;
    bool operator==(const Res &o) const { return a == o.a && b == o.b && cls == o.cls; }
};

// the rule, step by step, with nothing shared with the core but the option struct
static Res brute(const std::string &s, const std::string &q, const Opts &o) {
    const long n = (long)s.size(), W = o.cut_window, need = (long)o.cut_mean_q * W;
    auto p = [&](long i) { return std::max(0L, (long)(unsigned char)q[(size_t)i] - 33); };
    auto isn = [&](long i) { return s[(size_t)i] == 'N' || s[(size_t)i] == 'n'; };
    auto wsum = [&](long i) {
        long t = 0;
        for (long j = i; j < i + W; ++j) t += p(j);
        return t;
    };
    long a = std::min<long>(o.trim_front, n), b = std::max<long>(a, n - (long)std::min<uint64_t>(o.trim_tail, (uint64_t)n));
    if ((o.flags & CUT_FRONT) && b > a) {
        long hit = -1;
        for (long i = a; i + W <= b; ++i)
            if (wsum(i) >= need) {
                hit = i;
                break;
            }
        if (hit < 0) a = b;
        else {
            a = hit;
            while (a < b && isn(a)) ++a;
        }
    }
    if ((o.flags & CUT_TAIL) && b > a) {
        long hit = -1;
        for (long j = b; j - W >= a; --j)
            if (wsum(j - W) >= need) {
                hit = j;
                break;
            }
        if (hit < 0) b = a;
        else {
            b = hit;
            while (b > a && isn(b - 1)) --b;
        }
    }
    long nn = 0, low = 0;
    for (long i = a; i < b; ++i) nn += isn(i), low += p(i) < (long)o.qualified_q;
    const long len = b - a;
    uint32_t cls = 0;
    if (len < (long)o.min_len || len == 0) cls = 1;
    else if (nn > (long)o.n_base_limit) cls = 2;
    else if (100 * low > (long)o.unqualified_percent * len) cls = 3;
    return Res{(uint32_t)a, (uint32_t)b, cls};
}

static Res core(const std::string &s, const std::string &q, const Opts &o) {
    // exact-size heap copies: a read past either end is the sanitizer's to report
    std::vector<uint8_t> sv(s.begin(), s.end()), qv(q.begin(), q.end());
    Res r;
    r.cls = judge_serial(sv.data(), qv.data(), (uint32_t)s.size(), o, r.a, r.b);
    return r;
}

static Res both(const std::string &s, const std::string &q, const Opts &o) {
    CHECK(s.size() == q.size());
    CHECK(invalid(o) == nullptr);
    const Res r = core(s, q, o), e = brute(s, q, o);
    if (!(r == e)) std::printf("core (%u, %u, %u) brute (%u, %u, %u) n = %zu\n", r.a, r.b, r.cls, e.a, e.b, e.cls, s.size());
    CHECK(r == e);
    ++n_cases;
    return r;
}

static std::string bases(size_t n) {
    std::string s(n, 'A');
    for (size_t i = 0; i < n; ++i) s[i] = "ACGT"[(i * 7 + i / 3) & 3];
    return s;
}
static const Opts NEUTRAL = {0, 0, 4, 20, 0xFFFFFFFFu, 0, 100, 0, 0};

int main() {
    const char G = 'I', B = '#'; // phred 40, 2
    // ---- validation
    {
        Opts o = recipe();
        CHECK(invalid(o) == nullptr);
        o.cut_window = 0;
        CHECK(invalid(o) != nullptr);
        o.cut_window = 1001;
        CHECK(invalid(o) != nullptr);
        o.cut_window = 1000;
        CHECK(invalid(o) == nullptr);
        o = recipe(), o.cut_mean_q = 94;
        CHECK(invalid(o) != nullptr);
        o = recipe(), o.qualified_q = 94;
        CHECK(invalid(o) != nullptr);
        o = recipe(), o.unqualified_percent = 101;
        CHECK(invalid(o) != nullptr);
        o = recipe(), o.flags = 4;
        CHECK(invalid(o) != nullptr);
        o = recipe(), o.trim_front = o.trim_tail = o.n_base_limit = o.min_len = 0xFFFFFFFFu, o.cut_mean_q = o.qualified_q = 93, o.unqualified_percent = 100;
        CHECK(invalid(o) == nullptr);
        CHECK(phred(0) == 0 && phred(32) == 0 && phred(33) == 0 && phred(34) == 1 && phred(126) == 93 && phred(255) == 222);
        CHECK(is_n('N') && is_n('n') && !is_n('A') && !is_n('\n'));
    }
    // ---- every option alone, on reads with bad ends and an N
    {
        std::string s = bases(40), q = std::string(7, B) + std::string(26, G) + std::string(7, B);
        s[7] = 'N', s[32] = 'n', s[20] = 'N';
        Opts o = NEUTRAL;
        CHECK((both(s, q, o) == Res{0, 40, 0}));
        o = NEUTRAL, o.trim_front = 5;
        CHECK((both(s, q, o) == Res{5, 40, 0}));
        o = NEUTRAL, o.trim_tail = 5;
        CHECK((both(s, q, o) == Res{0, 35, 0}));
        o = NEUTRAL, o.flags = CUT_FRONT; // windows from 5: 2 + 2 + 40 + 40 = 84 >= 80, at 4: 46
        CHECK((both(s, q, o) == Res{5, 40, 0}));
        o = NEUTRAL, o.flags = CUT_TAIL;
        CHECK((both(s, q, o) == Res{0, 35, 0}));
        o = NEUTRAL, o.n_base_limit = 2;
        CHECK((both(s, q, o) == Res{0, 40, 2}));
        o.n_base_limit = 3;
        CHECK((both(s, q, o) == Res{0, 40, 0}));
        o = NEUTRAL, o.qualified_q = 20, o.unqualified_percent = 34; // lowq = 14 of 40: 1400 > 1360
        CHECK((both(s, q, o) == Res{0, 40, 3}));
        o.unqualified_percent = 35; // 1400 > 1400 is false
        CHECK((both(s, q, o) == Res{0, 40, 0}));
        o = NEUTRAL, o.min_len = 40;
        CHECK((both(s, q, o) == Res{0, 40, 0}));
        o.min_len = 41;
        CHECK((both(s, q, o) == Res{0, 40, 1}));
        // an N directly after the front cut and directly before the tail cut
        std::string s2 = bases(40);
        s2[5] = s2[6] = 'N', s2[34] = 'n', s2[33] = 'N';
        o = NEUTRAL, o.flags = CUT_FRONT | CUT_TAIL;
        CHECK((both(s2, q, o) == Res{7, 33, 0}));
        CHECK((both(s2, q, recipe()) == Res{7, 33, 0}));
        CHECK((both(std::string(40, 'N'), std::string(40, G), o) == Res{40, 40, 1}));
    }
    // ---- W = 1 and W = 1000, M = 0, lengths 0, 1, W - 1, W, W + 1
    for (uint32_t W : {1u, 4u, 64u, 1000u}) {
        for (uint32_t M : {0u, 20u, 93u}) {
            Opts o = NEUTRAL;
            o.cut_window = W, o.cut_mean_q = M, o.flags = CUT_FRONT | CUT_TAIL;
            for (size_t n : {(size_t)0, (size_t)1, (size_t)W - 1, (size_t)W, (size_t)W + 1, (size_t)2 * W + 3}) {
                const Res g = both(bases(n), std::string(n, G), o), b = both(bases(n), std::string(n, B), o);
                if (M == 0 && n >= W) CHECK((g == Res{0, (uint32_t)n, 0u}) && (b == g)); // nothing is cut
                if (M == 20 && n >= W) CHECK((g == Res{0, (uint32_t)n, 0u}));
                if (M == 20 && n) CHECK(b.a == b.b && b.cls == 1);
                if (n && n < W) CHECK(g.a == g.b && g.cls == 1); // no window fits, whatever M
                std::string q(n, G);
                for (size_t i = 0; i < n; i += 3) q[i] = B;
                both(bases(n), q, o);
                if (n > 2) q[0] = q[n - 1] = '~', both(bases(n), q, o);
            }
        }
    }
    // ---- trim_front + trim_tail = n - 1, n, n + 1, and beyond
    for (uint32_t n : {0u, 1u, 2u, 11u, 12u}) {
        for (uint32_t f = 0; f <= n + 2; ++f)
            for (uint32_t t : {0u, n > f ? n - f - 1 : 0u, n > f ? n - f : 0u, n - (f < n ? f : n) + 1, 0xFFFFFFFFu}) {
                Opts o = NEUTRAL;
                o.trim_front = f, o.trim_tail = t;
                const Res r = both(bases(n), std::string(n, G), o);
                CHECK(r.a <= r.b && r.b <= n);
                o = recipe(), o.trim_front = f, o.trim_tail = t, o.min_len = 1;
                both(bases(n), std::string(n, G), o);
            }
    }
    // ---- a single bad base at each position of a 12-base read
    for (size_t pos = 0; pos < 12; ++pos) {
        std::string q(12, G);
        q[pos] = B;
        Opts o = NEUTRAL;
        o.flags = CUT_FRONT | CUT_TAIL, o.cut_mean_q = 40; // every window must be all good
        const Res r = both(bases(12), q, o);
        if (pos < 4) CHECK((r == Res{(uint32_t)pos + 1, 12, 0}));
        else if (pos >= 8) CHECK((r == Res{0, (uint32_t)pos, 0}));
        else CHECK((r == Res{0, 12, 0})); // the ends are clean: a bad middle is not the cuts' business
        o.cut_mean_q = 31; // (3 * 40 + 2) / 4 = 30.5: a window with the bad base fails
        both(bases(12), q, o);
        o.cut_mean_q = 30; // ... and passes
        CHECK((both(bases(12), q, o) == Res{0, 12, 0}));
        both(bases(12), q, recipe());
    }
    // ---- nN at the limit and one above; 100 * lowq against U * len; len against min_len
    {
        for (uint32_t lim : {0u, 1u, 5u})
            for (uint32_t nn = 0; nn <= 7; ++nn) {
                std::string s = bases(50);
                for (uint32_t i = 0; i < nn; ++i) s[10 + 3 * i] = i & 1 ? 'n' : 'N';
                Opts o = recipe();
                o.n_base_limit = lim;
                CHECK(both(s, std::string(50, G), o).cls == (nn > lim ? 2u : 0u));
            }
        for (uint32_t low = 0; low <= 30; ++low) { // the kept span is [5, 35) of 40: 30 bases, U = 40: 12 is the last to pass
            std::string q(40, G);
            for (uint32_t i = 0; i < low; ++i) q[5 + i] = '4'; // phred 19: below Q = 20, yet no window fails at M = 19
            Opts o = recipe();
            o.cut_mean_q = 19;
            const Res r = both(bases(40), q, o);
            CHECK((r == Res{5, 35, low > 12 ? 3u : 0u}));
        }
        for (uint32_t n : {23u, 24u, 25u, 26u}) CHECK(both(bases(n), std::string(n, G), recipe()).cls == (n - 10 < 15 ? 1u : 0u));
    }
    // ---- pseudo-random reads, every flag combination
    {
        uint64_t x = 88172645463325252ull;
        auto rnd = [&] {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            return (uint32_t)(x >> 24);
        };
        for (int it = 0; it < 3000; ++it) {
            const size_t n = rnd() % (it % 10 == 0 ? 1200 : 80);
            std::string s = bases(n), q(n, G);
            const uint32_t mode = rnd() % 4;
            for (size_t i = 0; i < n; ++i) {
                if (rnd() % 20 == 0) s[i] = rnd() & 1 ? 'N' : 'n';
                q[i] = (char)(33 + (mode == 0 ? 30 + rnd() % 11 : mode == 1 ? 18 + rnd() % 5 : mode == 2 ? rnd() % 42 : (i < 9 || i + 9 > n ? 3 : 38)));
            }
            Opts o = recipe();
            o.flags = rnd() % 4, o.cut_window = it % 7 == 0 ? 1 + rnd() % 1000 : 1 + rnd() % 8, o.cut_mean_q = rnd() % 41;
            o.trim_front = rnd() % 8, o.trim_tail = rnd() % 8, o.n_base_limit = rnd() % 4, o.min_len = rnd() % 20;
            o.qualified_q = rnd() % 41, o.unqualified_percent = rnd() % 101;
            both(s, q, o);
        }
    }
    std::printf("ok %d\n", n_cases);
    return 0;
}
