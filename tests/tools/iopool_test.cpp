// The input side's host pool and buffers (nextpolish2_amd/csrc/np2_iopool.hpp) without a device: every item of a parallel
// loop runs exactly once whatever the sizes, the caller's `during` runs once while the helpers work and its exception comes
// back once the loop has drained, two callers share the pool, RawBuf against a std::vector, and which blocks HostBlockPool
// keeps.  Built with the thread sanitizer and with the address and undefined-behaviour sanitizers, run with
// NP2_IO_THREADS=4 (tests/test_iopool_cpu.py).
//
//     iopool_test sizes | one_thread | during | during_throws | two_callers | rawbuf | blocks
//
// Prints "ok" and exits 0, or names the failed checks and exits 1.
#include "../../nextpolish2_amd/csrc/np2_iopool.hpp"

#include <cstdio>
#include <memory>
#include <random>
#include <sched.h>
#include <stdexcept>
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

// how often each item of a loop ran
struct Counts {
    std::unique_ptr<std::atomic<int>[]> c;
    size_t n;
    explicit Counts(size_t n_) : c(new std::atomic<int>[n_ + 1]), n(n_) {
        for (size_t i = 0; i <= n; ++i) c[i].store(0);
    }
    bool all_once() const {
        for (size_t i = 0; i < n; ++i)
            if (c[i].load() != 1) return false;
        return c[n].load() == 0; // (and nothing beyond the last)
    }
};

static void sizes() {
    CHECK(IoPool::get().size() == 4); // NP2_IO_THREADS workers, the caller among them
    for (size_t n : {(size_t)0, (size_t)1, (size_t)3, (size_t)1000})
        for (unsigned max_threads : {64u, 2u}) {
            Counts k(n);
            std::atomic<uint64_t> sum{0};
            IoPool::get().parallel_for(n, max_threads, [&](size_t i) {
                CHECK(i < n);
                ++k.c[std::min(i, n)];
                sum += i;
            });
            CHECK(k.all_once());
            CHECK(sum.load() == (uint64_t)n * (n ? n - 1 : 0) / 2);
        }
}

static void one_thread() { // max_threads 1 (and a loop of one item): the caller does it all, in order
    const std::thread::id me = std::this_thread::get_id();
    std::vector<size_t> order; // (written without a lock: one thread)
    IoPool::get().parallel_for(500, 1, [&](size_t i) {
        CHECK(std::this_thread::get_id() == me);
        order.push_back(i);
    });
    CHECK(order.size() == 500);
    for (size_t i = 0; i < order.size(); ++i) CHECK(order[i] == i);
    int ran = 0;
    IoPool::get().parallel_for(1, 64, [&](size_t) {
        CHECK(std::this_thread::get_id() == me);
        ++ran;
    });
    CHECK(ran == 1);
    // the same for the loop with a `during`: nobody to wait for, so the items run first, then `during`
    std::vector<int> log;
    IoPool::get().parallel_for_during(3, 1, [&](size_t i) { log.push_back((int)i); }, [&] { log.push_back(-1); });
    CHECK((log == std::vector<int>{0, 1, 2, -1}));
    log.clear();
    IoPool::get().parallel_for_during(0, 64, [&](size_t i) { log.push_back((int)i); }, [&] { log.push_back(-1); });
    CHECK((log == std::vector<int>{-1}));
}

// `during` trails the items as they complete, in index order (what the BAM reader's record walk does behind the inflate)
static void during() {
    const size_t n = 400;
    const std::thread::id me = std::this_thread::get_id();
    Counts k(n);
    std::unique_ptr<std::atomic<uint8_t>[]> done(new std::atomic<uint8_t>[n]);
    std::vector<uint32_t> value(n, 0);
    for (size_t i = 0; i < n; ++i) done[i].store(0);
    int during_runs = 0;
    size_t seen = 0;
    std::atomic<int> by_helpers{0};
    IoPool::get().parallel_for_during(n, 64, [&](size_t i) {
        if (std::this_thread::get_id() != me) ++by_helpers;
        ++k.c[i];
        value[i] = (uint32_t)(i * 2654435761u);
        done[i].store(1, std::memory_order_release);
    }, [&] {
        CHECK(std::this_thread::get_id() == me);
        ++during_runs;
        for (size_t i = 0; i < n; ++i) { // (every item is done by a helper: the caller joins only after this)
            while (!done[i].load(std::memory_order_acquire)) sched_yield();
            CHECK(value[i] == (uint32_t)(i * 2654435761u));
            ++seen;
        }
    });
    CHECK(during_runs == 1 && seen == n);
    CHECK(by_helpers.load() == (int)n);
    CHECK(k.all_once());
}

// an exception of `during` comes back to the caller after the loop has drained: every item still ran, exactly once, and
// the pool goes on working
static void during_throws() {
    const size_t n = 300;
    Counts k(n);
    std::unique_ptr<std::atomic<uint8_t>[]> done(new std::atomic<uint8_t>[n]);
    for (size_t i = 0; i < n; ++i) done[i].store(0);
    bool caught = false;
    try {
        IoPool::get().parallel_for_during(n, 64, [&](size_t i) {
            ++k.c[i];
            done[i].store(1, std::memory_order_release);
        }, [&] {
            for (size_t i = 0; i < 5; ++i)
                while (!done[i].load(std::memory_order_acquire)) sched_yield();
            throw std::runtime_error("the walk tripped");
        });
    } catch (const std::runtime_error &e) {
        caught = std::string(e.what()) == "the walk tripped";
        CHECK(k.all_once()); // (already here: nothing of the loop is still running)
    }
    CHECK(caught);
    Counts k2(100);
    IoPool::get().parallel_for(100, 64, [&](size_t i) { ++k2.c[i]; });
    CHECK(k2.all_once());
}

static void two_callers() { // two threads, each with loops of its own at the same time
    std::vector<std::thread> th;
    for (int t = 0; t < 2; ++t)
        th.emplace_back([t] {
            for (int rep = 0; rep < 20; ++rep) {
                const size_t n = 200 + 37 * (size_t)t + (size_t)rep;
                Counts k(n);
                std::atomic<uint64_t> sum{0};
                IoPool::get().parallel_for(n, 64, [&](size_t i) {
                    ++k.c[i];
                    sum += i + (size_t)t;
                });
                CHECK(k.all_once());
                CHECK(sum.load() == (uint64_t)n * (n - 1) / 2 + (uint64_t)n * (uint64_t)t);
            }
        });
    for (auto &x : th) x.join();
}

static void rawbuf() {
    std::mt19937 rng(20240);
    RawBuf b;
    std::vector<uint8_t> model;
    CHECK(b.size() == 0 && b.data() == nullptr);
    for (int step = 0; step < 400; ++step) {
        const unsigned what = rng() % 8;
        if (what < 5) { // grow or shrink; new bytes are not initialised: written here, in both
            size_t m = rng() % 3 == 0 ? rng() % (model.size() + 1) : model.size() + rng() % 70000;
            if (step == 200) m = model.size() + ((size_t)5 << 20); // (past the block pool's threshold, once)
            const size_t old = model.size();
            b.resize(m);
            model.resize(m);
            for (size_t i = old; i < m; ++i) b.data()[i] = model[i] = (uint8_t)rng();
        } else if (what < 7) {
            const size_t k = rng() % 5 == 0 ? model.size() + rng() % 3 : rng() % (model.size() + 1);
            b.drop_front(k);
            model.erase(model.begin(), model.begin() + (long)std::min(k, model.size()));
        } else {
            b.clear();
            model.clear();
        }
        CHECK(b.size() == model.size());
        CHECK(b.cap >= b.n);
        CHECK(model.empty() || memcmp(b.data(), model.data(), model.size()) == 0);
    }
}

static void blocks() {
    HostBlockPool &hp = HostBlockPool::get();
    const size_t T = (size_t)4 << 20; // blocks from this size on are kept
    size_t cap = 0;
    uint8_t *small = hp.take(T - 1, cap);
    CHECK(small && cap == T - 1);
    hp.give(small, cap); // freed, not kept
    CHECK(hp.idle.empty());
    hp.give(nullptr, T); // nothing
    CHECK(hp.idle.empty());
    uint8_t *a = hp.take(T, cap);
    CHECK(a && cap == T);
    uint8_t *b = hp.take(T + 4096, cap);
    CHECK(b && cap == T + 4096);
    hp.give(b, T + 4096);
    hp.give(a, T);
    CHECK(hp.idle.size() == 2);
    // the smallest block that is large enough, with ITS capacity
    CHECK(hp.take(T - 100, cap) == a && cap == T);
    CHECK(hp.idle.size() == 1);
    hp.give(a, T);
    CHECK(hp.take(T + 1, cap) == b && cap == T + 4096);
    hp.give(b, T + 4096);
    // none large enough: a fresh one of the size asked for
    uint8_t *c = hp.take(T + 4097, cap);
    CHECK(c && c != a && c != b && cap == T + 4097);
    CHECK(hp.idle.size() == 2);
    hp.give(c, cap);
    CHECK(hp.idle.size() == 3);
    // at most 8 idle blocks
    std::vector<uint8_t *> more;
    for (int i = 0; i < 6; ++i) more.push_back(hp.take(T + 8192, cap));
    for (uint8_t *p : more) hp.give(p, T + 8192);
    CHECK(hp.idle.size() == 8);
}

int main(int argc, char **argv) {
    const std::string s = argc > 1 ? argv[1] : "";
    if (s == "sizes") sizes();
    else if (s == "one_thread") one_thread();
    else if (s == "during") during();
    else if (s == "during_throws") during_throws();
    else if (s == "two_callers") two_callers();
    else if (s == "rawbuf") rawbuf();
    else if (s == "blocks") blocks();
    else {
        fprintf(stderr, "usage: iopool_test sizes | one_thread | during | during_throws | two_callers | rawbuf | blocks\n");
        return 2;
    }
    if (failures.load()) return 1;
    printf("ok\n");
    return 0;
}
