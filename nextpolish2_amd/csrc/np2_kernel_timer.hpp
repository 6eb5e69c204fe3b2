// HIP-event timer of the scan drivers (np2_qv_host.cpp, np2_trio_host.cpp): the kernels of a call alone, summed over its
// staging pieces.
#pragma once
#include "np2_ctx.hpp"

struct KernelTimer { // HIP events around the scan kernel alone, summed over the pieces
    hipEvent_t a = nullptr, b = nullptr;
    float ms = 0.f;
    explicit KernelTimer(bool on) {
        if (!on) return;
        HIPCHK(hipEventCreate(&a));
        HIPCHK(hipEventCreate(&b));
    }
    ~KernelTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    void start(hipStream_t s) {
        if (a) HIPCHK(hipEventRecord(a, s));
    }
    void stop(hipStream_t s) {
        if (b) HIPCHK(hipEventRecord(b, s));
    }
    void collect() { // (after the stream was drained)
        if (!a) return;
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, a, b));
        ms += t;
    }
};
