// What the host drivers (np2_*_host.cpp) share on the HIP side: events and the kernel timer built on them, the grid of
// a kernel whose blocks stride over their work, the tests' environment hooks, the look at the device's free memory, the
// pinned buffers of a run, the output file of the native writers and the range check of a table index.  (The plumbing
// that needs no HIP is np2_pieces.hpp.)
#pragma once
#include "np2_ctx.hpp"
#include "np2_deflate.hpp"

#include <climits>

namespace np2h {

struct DevEvent {
    hipEvent_t e = nullptr;
    DevEvent() = default;
    DevEvent(const DevEvent &) = delete;
    DevEvent &operator=(const DevEvent &) = delete;
    ~DevEvent() {
        if (e) (void)hipEventDestroy(e);
    }
    void make() { HIPCHK(hipEventCreate(&e)); }
};
inline float elapsed(const DevEvent &a, const DevEvent &b) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, a.e, b.e));
    return ms;
}

// NP2_*_TEST_*: a test's (or a probe's) value for a size the drivers fix, clamped to [lo, hi]; read once per call
inline long long test_hook(const char *env, long long lo, long long hi, long long dflt) {
    const char *e = getenv(env);
    return e ? std::min(hi, std::max(lo, atoll(e))) : dflt;
}

// the grid of a kernel whose blocks stride over their work: what the device holds at once, `per_cu` blocks a CU;
// test_env: a test's grid
inline uint32_t grid_blocks(int device, uint32_t per_cu, const char *test_env = nullptr) {
    if (test_env && getenv(test_env)) return (uint32_t)test_hook(test_env, 1, 1 << 16, 1);
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    return (uint32_t)std::max(1, cus) * per_cu;
}

// room for `bytes` and a margin on the device, or NP2_E_NOMEM with make_message(free bytes)
template <class Msg> void need_device_bytes(size_t bytes, size_t margin, Msg make_message) {
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    if (bytes + margin > fr) {
        dev_cache().trim(0); // (this process's idle blocks may be what is missing)
        HIPCHK(hipMemGetInfo(&fr, &tot));
    }
    if (bytes + margin > fr) throw Np2Error(NP2_E_NOMEM, make_message(fr));
}

// the pinned buffers of a run's pieces (process-wide pool), given back when the run ends: declare it before the threads
struct PinnedBlocks {
    std::vector<void *> held;
    ~PinnedBlocks() {
        for (void *p : held) pinned_pool().put(p);
    }
    uint8_t *get(size_t bytes) {
        held.reserve(held.size() + 1);
        void *p = pinned_pool().get(bytes);
        if (!p) throw Np2Error(NP2_E_NOMEM, "hipHostMalloc failed");
        held.push_back(p);
        return (uint8_t *)p;
    }
};

// An output a caller may not have asked for: open(nullptr, ...) leaves it closed, put() then writes nothing.  A path ending
// in .gz or .bgz is written as BGZF through the device (BgzfWriter, np2_deflate.hpp), every other path as the plain bytes.
// An OutFile that goes without close() — its driver failed — leaves a compressed file without the EOF block.
struct OutFile {
    std::string path;
    FILE *f = nullptr;
    std::unique_ptr<BgzfWriter> z;
    ~OutFile() {
        if (f) fclose(f);
    }
    bool is_open() const { return f != nullptr || z != nullptr; }
    void open(const char *p, int device) {
        if (!p) return;
        path = p;
        if (bgzf_path(p)) {
            z.reset(new BgzfWriter(device, p));
            return;
        }
        f = fopen(p, "wb");
        if (!f) throw Np2Error(NP2_E_ARG, "cannot open " + path + " for writing");
        setvbuf(f, nullptr, _IOFBF, 1 << 20);
    }
    void put(const void *p, size_t n) {
        if (z) z->write(p, n);
        else if (f && n && fwrite(p, 1, n, f) != n) throw Np2Error(NP2_E_ARG, "cannot write " + path);
    }
    void close() {
        if (z) {
            std::unique_ptr<BgzfWriter> w(std::move(z));
            w->close();
        }
        FILE *g = f;
        f = nullptr;
        if (g && fclose(g) != 0) throw Np2Error(NP2_E_ARG, "cannot write " + path);
    }
};

// table `idx` (the entry point's argument `arg_name`) is one of the context's
inline void check_table(np2_ctx *cx, int idx, const std::string &who, const char *arg_name) {
    if (idx < 0 || (size_t)idx >= cx->yaks.size())
        throw Np2Error(NP2_E_ARG, who + ": " + arg_name + " " + std::to_string(idx) + " out of range (the context has " +
                                      std::to_string(cx->yaks.size()) + " tables)");
}

} // namespace np2h

struct KernelTimer { // HIP events around the scan kernel alone, summed over the pieces
    np2h::DevEvent a, b;
    float ms = 0.f;
    explicit KernelTimer(bool on) {
        if (on) a.make(), b.make();
    }
    void start(hipStream_t s) {
        if (a.e) HIPCHK(hipEventRecord(a.e, s));
    }
    void stop(hipStream_t s) {
        if (b.e) HIPCHK(hipEventRecord(b.e, s));
    }
    void collect() { // (after the stream was drained)
        if (a.e) ms += np2h::elapsed(a, b);
    }
};
