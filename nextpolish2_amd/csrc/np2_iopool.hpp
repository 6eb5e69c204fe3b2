// The persistent thread pool behind every parallel loop of the input side (np2_bamfile.cpp, np2_frontend.cpp, np2_fetch_gpu.cpp), the cache of large host blocks and the byte buffer on it.
// Host-only: no HIP here, so that a plain C++ compiler builds it (tests/tools/iopool_test.cpp, under the thread and address sanitizers).
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <utility>
#include <vector>

namespace np2h {

// Small persistent pool for the input side: BGZF blocks are independent deflate streams and BAM records independent
// byte ranges, so inflate and record copy are plain parallel loops.  Work items are handed out by an atomic counter;
// the calling thread works too.  One pool per process, sized to the host (at most 64 workers).  Several loops may be
// in flight at once (the command line keeps a few contigs' front ends going side by side): a worker takes items from
// whichever open loop still has some, so a single caller gets the whole pool and concurrent callers share it.
class IoPool {
  public:
    static IoPool &get() {
        static IoPool *p = new IoPool(); // leaked on purpose: workers outlive static destruction
        return *p;
    }
    unsigned size() const { return (unsigned)workers_.size() + 1; }
    // run fn(i) for i in [0, n), at most `max_threads` threads including the caller
    template <class F> void parallel_for(size_t n, unsigned max_threads, F fn) {
        if (n == 0) return;
        const unsigned want = (unsigned)std::min<size_t>(std::min<size_t>(max_threads, size()), n);
        if (want <= 1) {
            for (size_t i = 0; i < n; ++i) fn(i);
            return;
        }
        Job job;
        job.n = n;
        job.slots = want - 1; // helpers wanted besides the caller
        std::function<void(size_t)> body = fn;
        job.fn = &body;
        {
            std::lock_guard<std::mutex> l(mu_);
            jobs_.push_back(&job);
        }
        cv_.notify_all();
        run(job);
        std::unique_lock<std::mutex> l(mu_);
        jobs_.erase(std::find(jobs_.begin(), jobs_.end(), &job)); // no new helper can pick it up from here on
        done_cv_.wait(l, [&] { return job.helpers == 0; });
    }

    // the same loop with the CALLER doing `during()` first — work that consumes the items' results as they appear (it
    // must only wait for items in index order: they are handed out in that order) — and joining the loop afterwards
    template <class F, class G> void parallel_for_during(size_t n, unsigned max_threads, F fn, G during) {
        const unsigned want = (unsigned)std::min<size_t>(std::min<size_t>(max_threads, size()), n);
        if (want <= 1) { // nobody to wait for: items first
            for (size_t i = 0; i < n; ++i) fn(i);
            during();
            return;
        }
        Job job;
        job.n = n;
        job.slots = want - 1;
        std::function<void(size_t)> body = fn;
        job.fn = &body;
        {
            std::lock_guard<std::mutex> l(mu_);
            jobs_.push_back(&job);
        }
        cv_.notify_all();
        std::exception_ptr ep;
        try {
            during();
        } catch (...) {
            ep = std::current_exception();
        }
        run(job);
        {
            std::unique_lock<std::mutex> l(mu_);
            jobs_.erase(std::find(jobs_.begin(), jobs_.end(), &job));
            done_cv_.wait(l, [&] { return job.helpers == 0; });
        }
        if (ep) std::rethrow_exception(ep);
    }

  private:
    struct Job {
        size_t n = 0;
        std::atomic<size_t> next{0};
        unsigned slots = 0;   // helpers that may still join (guarded by mu_)
        unsigned helpers = 0; // helpers currently inside (guarded by mu_)
        std::function<void(size_t)> *fn = nullptr;
    };
    static void run(Job &j) {
        for (;;) {
            const size_t i = j.next.fetch_add(1, std::memory_order_relaxed);
            if (i >= j.n) break;
            (*j.fn)(i);
        }
    }
    IoPool() {
        // sized by the hardware, not by the quota: the pool works in bursts of a few milliseconds (one contig's inflate),
        // which a CFS quota does not throttle — measured on a box with 256 hardware threads and a quota of 16 CPUs: an
        // E. coli-sized contig's records arrive in 8 ms with 64 workers and in 18 ms with 16
        unsigned hw = std::thread::hardware_concurrency();
        unsigned n = std::min<unsigned>(64, std::max<unsigned>(2, hw / 2));
        if (const char *e = getenv("NP2_IO_THREADS")) n = (unsigned)std::max(1, atoi(e));
        for (unsigned i = 1; i < n; ++i) workers_.emplace_back([this] { loop(); });
        for (auto &t : workers_) t.detach();
    }
    Job *pick() { // mu_ held: an open loop with items left and a free helper slot
        for (Job *j : jobs_)
            if (j->slots && j->next.load(std::memory_order_relaxed) < j->n) return j;
        return nullptr;
    }
    void loop() {
        std::unique_lock<std::mutex> l(mu_);
        for (;;) {
            Job *j = nullptr;
            cv_.wait(l, [&] { return (j = pick()) != nullptr; });
            --j->slots;
            ++j->helpers;
            l.unlock();
            run(*j);
            l.lock();
            if (--j->helpers == 0) done_cv_.notify_all();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    std::vector<Job *> jobs_;
};

// growable byte buffer without value-initialisation (a std::vector would zero 100+ MiB per refill just to have inflate
// overwrite it); kept by the BAM handle, so its pages are faulted in once
// Large host blocks kept across BAM handles (the command line opens one handle per front-end thread and run): a block
// of this size goes back to the kernel when freed, and the next handle's inflate threads then fault 200 MB of fresh
// pages in again (11-14 ms of an E. coli-sized contig's first front end).  At most 8 idle blocks / 1 GiB are kept.
struct HostBlockPool {
    std::mutex mu;
    std::vector<std::pair<size_t, uint8_t *>> idle;
    static HostBlockPool &get() {
        static HostBlockPool *p = new HostBlockPool(); // leaked on purpose
        return *p;
    }
    uint8_t *take(size_t want, size_t &cap) {
        {
            std::lock_guard<std::mutex> l(mu);
            size_t best = idle.size();
            for (size_t i = 0; i < idle.size(); ++i)
                if (idle[i].first >= want && (best == idle.size() || idle[i].first < idle[best].first)) best = i;
            if (best != idle.size()) {
                uint8_t *p = idle[best].second;
                cap = idle[best].first;
                idle.erase(idle.begin() + (long)best);
                return p;
            }
        }
        cap = want;
        return (uint8_t *)malloc(want);
    }
    void give(uint8_t *p, size_t cap) {
        if (!p) return;
        if (cap >= ((size_t)4 << 20)) {
            std::lock_guard<std::mutex> l(mu);
            size_t held = cap;
            for (auto &b : idle) held += b.first;
            if (idle.size() < 8 && held <= ((size_t)1 << 30)) {
                idle.emplace_back(cap, p);
                return;
            }
        }
        free(p);
    }
};
struct RawBuf {
    uint8_t *p = nullptr;
    size_t n = 0, cap = 0;
    RawBuf() = default;
    RawBuf(const RawBuf &) = delete;
    RawBuf &operator=(const RawBuf &) = delete;
    ~RawBuf() { HostBlockPool::get().give(p, cap); }
    size_t size() const { return n; }
    uint8_t *data() { return p; }
    const uint8_t *data() const { return p; }
    void clear() { n = 0; }
    void resize(size_t m) {
        if (m > cap) {
            const size_t want = std::max(m, cap + cap / 2 + (1u << 20));
            size_t got = 0;
            uint8_t *q = HostBlockPool::get().take(want, got);
            if (!q) throw std::bad_alloc();
            if (n) memcpy(q, p, n);
            HostBlockPool::get().give(p, cap);
            p = q;
            cap = got;
        }
        n = m;
    }
    void drop_front(size_t k) { // discard the first k bytes
        if (k >= n) {
            n = 0;
            return;
        }
        memmove(p, p + k, n - k);
        n -= k;
    }
};

} // namespace np2h
