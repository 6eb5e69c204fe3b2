// The host plumbing the drivers share (nextpolish2_amd/csrc/np2_pieces.hpp) without a device: the halo writer against the
// stream it was fed, the piece queue and its reader threads (order, a reader's error, a consumer that gives up), the string
// packer against a direct model, and the messages of the string-set check.  Built with the thread sanitizer and with the
// address and undefined-behaviour sanitizers (tests/test_pieces_cpu.py).
//
//     pieces_test halo | flush | order | error_arg | error_alloc | giveup | strings | check
//
// Prints "ok" and exits 0, or names the failed checks and exits 1.
#include "../../nextpolish2_amd/csrc/np2_pieces.hpp"

#include <atomic>
#include <cstdio>
#include <memory>
#include <new>
#include <random>
#include <string>

using namespace np2h;

static std::atomic<int> failures{0};
#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

struct Piece {
    uint8_t *buf = nullptr;
    size_t n = 0;
    int producer = 0, seq = 0;
};

// `count` pieces of `cap` bytes (and their halo) on a queue's idle side
struct Pool {
    std::vector<std::vector<uint8_t>> mem;
    std::vector<Piece> pieces;
    Pool(PieceQueue<Piece> &q, size_t count, size_t cap) : mem(count, std::vector<uint8_t>(HALO + cap + 64)), pieces(count) {
        for (size_t i = 0; i < count; ++i) pieces[i].buf = mem[i].data(), q.idle.push_back(&pieces[i]);
    }
};

// ---- HaloWriter: the pieces' data concatenated is the stream, every halo is the 32 bytes in front of its piece ----------
static void halo_case(size_t cap, size_t n_in, uint32_t seed) {
    std::mt19937 rng(seed);
    std::vector<uint8_t> in(n_in);
    for (auto &b : in) b = rng() % 9 == 0 ? '\n' : "ACGT"[rng() % 4];
    PieceQueue<Piece> q;
    Pool pool(q, 2, cap);
    std::vector<uint8_t> got, halos; // data of all pieces; halo of all pieces
    std::vector<size_t> sizes;
    {
        auto readers = run_readers(1, q, [&](size_t) {
            HaloWriter<Piece> w(q, cap);
            std::mt19937 r2(seed + 1);
            for (size_t at = 0; at < in.size();) {
                const size_t take = std::min<size_t>(1 + r2() % 97, in.size() - at);
                w.put(in.data() + at, take);
                at += take;
            }
            w.flush();
            w.flush(); // (nothing is open: nothing happens)
        });
        while (Piece *p = q.take_full()) {
            halos.insert(halos.end(), p->buf, p->buf + HALO);
            got.insert(got.end(), p->buf + HALO, p->buf + HALO + p->n);
            sizes.push_back(p->n);
            q.give_idle(p);
        }
    }
    CHECK(q.err_code == NP2_OK && q.producers == 0);
    CHECK(got == in);
    CHECK(sizes.size() == (n_in + cap - 1) / cap);
    std::vector<uint8_t> padded(HALO, '\n'); // the stream with separators in front
    padded.insert(padded.end(), in.begin(), in.end());
    size_t at = 0;
    for (size_t i = 0; i < sizes.size(); ++i) {
        CHECK(sizes[i] == (i + 1 < sizes.size() ? cap : n_in - at) && sizes[i] > 0);
        CHECK(memcmp(halos.data() + i * HALO, padded.data() + at, HALO) == 0); // padded[at .. at + HALO) lies in front of in[at]
        at += sizes[i];
    }
}
static void test_halo() {
    for (size_t cap : {64, 65, 95, 96, 97, 4096, 8192})
        for (size_t n_in : {4096, 1, 31, 33, 0}) halo_case(cap, n_in, (uint32_t)(cap * 31 + n_in));
}

static void test_flush() {
    PieceQueue<Piece> q;
    Pool pool(q, 1, 64);
    HaloWriter<Piece> w(q, 64);
    w.flush(); // no piece is open
    CHECK(q.idle.size() == 1 && q.full.empty());
    CHECK(w.fresh() && w.cur == &pool.pieces[0] && w.cur->n == 0);
    w.flush(); // an open piece without a byte goes back, nothing is emitted
    CHECK(w.cur == nullptr && q.idle.size() == 1 && q.full.empty());
    const uint8_t b = 'A';
    w.put(&b, 1);
    w.flush();
    CHECK(q.idle.empty() && q.full.size() == 1 && q.full.front()->n == 1 && w.tail[HALO - 1] == 'A' && w.tail[HALO - 2] == '\n');
    // `even_empty`: a piece without a byte is emitted all the same (the binner's end of a file)
    q.give_idle(q.take_full());
    CHECK(w.fresh());
    w.flush(true);
    CHECK(q.full.size() == 1 && q.full.front()->n == 0 && w.tail[HALO - 1] == 'A');
    // a run that was given up: the writer is dead and swallows what it is given
    q.give_up();
    w.put(&b, 1);
    CHECK(w.dead && w.cur == nullptr);
}

// ---- PieceQueue + run_readers --------------------------------------------------------------------------------------------
static void test_order() {
    const int N_PROD = 4, N_EACH = 200;
    PieceQueue<Piece> q;
    Pool pool(q, 8, 64);
    int next[N_PROD] = {0, 0, 0, 0}, seen = 0;
    {
        auto readers = run_readers(N_PROD, q, [&](size_t ti) {
            for (int s = 0; s < N_EACH; ++s) {
                Piece *p = q.take_idle();
                if (!p) return;
                p->producer = (int)ti, p->seq = s;
                q.give_full(p);
            }
        });
        while (Piece *p = q.take_full()) {
            CHECK(p->producer >= 0 && p->producer < N_PROD && p->seq == next[p->producer]);
            ++next[p->producer], ++seen;
            q.give_idle(p);
        }
        CHECK(seen == N_PROD * N_EACH); // (nullptr came only after every reader had finished and nothing was left)
        CHECK(q.producers == 0);
    }
    for (int i = 0; i < N_PROD; ++i) CHECK(next[i] == N_EACH);
    CHECK(q.err_code == NP2_OK && q.err.empty() && q.idle.size() == 8);
    // a queue each: the consumer takes the readers' pieces in an order of its own
    std::vector<PieceQueue<Piece>> qs(3);
    std::vector<std::unique_ptr<Pool>> pools;
    for (auto &x : qs) pools.emplace_back(new Pool(x, 2, 64));
    {
        auto readers = run_readers(3, qs, [&](size_t ti) {
            for (int s = 0; s < 50; ++s) {
                Piece *p = qs[ti].take_idle();
                if (!p) return;
                p->producer = (int)ti, p->seq = s;
                qs[ti].give_full(p);
            }
        });
        for (int ti = 2; ti >= 0; --ti) {
            int s = 0;
            while (Piece *p = qs[ti].take_full()) {
                CHECK(p->producer == ti && p->seq == s);
                ++s;
                qs[ti].give_idle(p);
            }
            CHECK(s == 50 && qs[ti].err_code == NP2_OK);
        }
    }
}

// reader 1 throws after 10 pieces; the others would go on for ever
template <class Throw> static void error_case(Throw thrower, int want_code, const std::string &want_msg) {
    PieceQueue<Piece> q;
    Pool pool(q, 8, 64);
    std::atomic<int> finished{0};
    {
        auto readers = run_readers(4, q, [&](size_t ti) {
            struct Done {
                std::atomic<int> &n;
                ~Done() { ++n; }
            } done{finished};
            for (int s = 0;; ++s) {
                if (ti == 1 && s == 10) thrower();
                Piece *p = q.take_idle();
                if (!p) return; // (the others stop here)
                q.give_full(p);
            }
        });
        while (Piece *p = q.take_full()) q.give_idle(p);
        CHECK(q.producers == 0 && finished == 4); // (nullptr: every reader is through)
        CHECK(q.err_code == want_code);
        CHECK(q.err == want_msg);
    }
    CHECK(finished == 4);
}
static void test_error_arg() {
    error_case([] { throw Np2Error(NP2_E_ARG, "reads.fq.gz: cannot read the sequence file"); }, NP2_E_ARG, "reads.fq.gz: cannot read the sequence file");
}
static void test_error_alloc() {
    error_case([] { throw std::bad_alloc(); }, NP2_E_NOMEM, std::string("unexpected exception: ") + std::bad_alloc().what());
}

// the consumer leaves while every reader waits for an idle piece
static void test_giveup() {
    PieceQueue<Piece> q;
    Pool pool(q, 8, 64);
    std::atomic<int> finished{0};
    {
        auto readers = run_readers(4, q, [&](size_t) {
            while (Piece *p = q.take_idle()) q.give_full(p);
            ++finished;
        });
        for (;;) { // until all pieces are full: the readers wait from then on
            std::lock_guard<std::mutex> l(q.mu);
            if (q.full.size() == 8) break;
        }
        CHECK(finished == 0);
    } // (~Readers: give_up, join)
    CHECK(finished == 4 && q.producers == 0 && q.err_code == NP2_OK);
}

// ---- StringPieces against a direct model ------------------------------------------------------------------------------------
static void strings_case(const std::vector<uint64_t> &lens, uint32_t cap, uint32_t seed) {
    const uint32_t TILE = 64, HAL = 32, FIRST = 1u << 31, TILE_BITS = TILE / 8;
    const uint8_t PAD = '\n';
    std::mt19937 rng(seed);
    std::vector<uint64_t> off(1, 0);
    for (uint64_t l : lens) off.push_back(off.back() + l);
    std::vector<uint8_t> strs(off.back() + 1);
    for (auto &b : strs) b = (uint8_t)('A' + rng() % 26);
    // the model: every sequence's tiles in order, and where its bitmap lies
    struct Tile {
        uint64_t seq, t;
    };
    std::vector<Tile> tiles;
    std::vector<uint64_t> bit_base(lens.size() + 1, 0);
    for (size_t s = 0; s < lens.size(); ++s) {
        for (uint64_t t = 0; t * TILE < lens[s]; ++t) tiles.push_back({s, t});
        bit_base[s + 1] = bit_base[s] + (lens[s] + 7) / 8;
    }
    std::vector<int> bit_cover(bit_base.back(), 0);
    StringPieces sp(strs.data(), off.data(), lens.size(), cap, TILE, HAL, PAD, FIRST, TILE_BITS);
    size_t at = 0, n_pieces = 0; // tiles handed out so far
    while (sp.next()) {
        ++n_pieces;
        CHECK(sp.nt == std::min<size_t>(cap, tiles.size() - at) && sp.nt > 0);
        if (at + sp.nt > tiles.size()) return;
        // the halo: the 32 bytes in front of a sequence that goes on, else padding
        const Tile &f = tiles[at];
        std::vector<uint8_t> halo(HAL, PAD);
        if (f.t) memcpy(halo.data(), strs.data() + off[f.seq] + f.t * TILE - HAL, HAL);
        CHECK(memcmp(sp.hs.data(), halo.data(), HAL) == 0);
        size_t n_spans = 0;
        for (uint32_t x = 0; x < sp.nt; ++x) {
            const Tile &m = tiles[at + x];
            const bool new_span = x == 0 || tiles[at + x - 1].seq != m.seq;
            n_spans += new_span;
            const uint64_t from = m.t * TILE, n = std::min<uint64_t>(TILE, lens[m.seq] - from);
            std::vector<uint8_t> want(TILE, PAD);
            memcpy(want.data(), strs.data() + off[m.seq] + from, n);
            CHECK(memcmp(sp.hs.data() + HAL + (size_t)x * TILE, want.data(), TILE) == 0);
            CHECK(((sp.hd[x] & FIRST) != 0) == (m.t == 0));
            const uint32_t si = sp.hd[x] & ~FIRST;
            CHECK(si == n_spans - 1 && si < sp.spans.size());
            if (si >= sp.spans.size()) return;
            const StringPieces::Span &s = sp.spans[si];
            CHECK(s.seq == m.seq && s.tile0 <= x);
            if (new_span) { // its tiles in this piece: x .. x + k - 1
                uint32_t k = 1;
                while (x + k < sp.nt && tiles[at + x + k].seq == m.seq) ++k;
                CHECK(s.tile0 == x);
                CHECK(s.bit_at == bit_base[m.seq] + from / 8);
                CHECK(s.bit_bytes == std::min<uint64_t>((lens[m.seq] + 7) / 8 - from / 8, (uint64_t)k * TILE_BITS));
                for (uint64_t b = s.bit_at; b < s.bit_at + s.bit_bytes && b < bit_cover.size(); ++b) ++bit_cover[b];
            }
        }
        CHECK(sp.spans.size() == n_spans);
        at += sp.nt;
    }
    CHECK(at == tiles.size() && n_pieces == (tiles.size() + cap - 1) / cap);
    CHECK(!sp.next() && sp.nt == 0);
    for (int c : bit_cover) CHECK(c == 1); // the spans tile the bitmap: no gap, no overlap
}
static void test_strings() {
    const uint64_t T = 64;
    const std::vector<uint64_t> base = {0, 1, 31, 32, 33, T - 1, T, T + 1, 3 * T + 5};
    std::vector<std::vector<uint64_t>> orders = {base, std::vector<uint64_t>(base.rbegin(), base.rend()), {3 * T + 5}, {0, 0, 0}, {}, {0, 3 * T + 5, 0, 0, T, 0},
                                                 {3 * T + 5, 3 * T + 5, 1, 2 * T}};
    std::mt19937 rng(7);
    for (int i = 0; i < 4; ++i) {
        std::vector<uint64_t> o = base;
        std::shuffle(o.begin(), o.end(), rng);
        orders.push_back(o);
    }
    uint32_t seed = 1;
    for (const auto &o : orders)
        for (uint32_t cap : {1u, 2u, 3u, 1000u}) strings_case(o, cap, seed++);
}

// ---- check_string_set ---------------------------------------------------------------------------------------------------------
static std::string refused(const uint8_t *strs, const uint64_t *off, uint64_t n) {
    try {
        check_string_set("np2_x_strings", strs, off, n);
    } catch (const Np2Error &e) {
        CHECK(e.code == NP2_E_ARG);
        return e.what();
    }
    return "";
}
static void test_check() {
    const uint8_t s[4] = {'A', 'C', 'G', 'T'};
    const uint64_t up[3] = {0, 2, 4}, down[3] = {0, 3, 2}, flat[3] = {5, 5, 5};
    CHECK(refused(s, up, 2) == "" && refused(nullptr, nullptr, 0) == "" && refused(nullptr, flat, 2) == "");
    CHECK(refused(s, nullptr, 2) == "np2_x_strings: off is NULL with n > 0");
    CHECK(refused(s, down, 2) == "np2_x_strings: off is descending at sequence 1");
    CHECK(refused(nullptr, up, 2) == "np2_x_strings: strs is NULL with a non-zero length");
}

int main(int argc, char **argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "halo") test_halo();
    else if (what == "flush") test_flush();
    else if (what == "order") test_order();
    else if (what == "error_arg") test_error_arg();
    else if (what == "error_alloc") test_error_alloc();
    else if (what == "giveup") test_giveup();
    else if (what == "strings") test_strings();
    else if (what == "check") test_check();
    else {
        fprintf(stderr, "usage: pieces_test halo | flush | order | error_arg | error_alloc | giveup | strings | check\n");
        return 2;
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
