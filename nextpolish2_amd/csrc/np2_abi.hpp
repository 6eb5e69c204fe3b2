#pragma once
// The edge of the C ABI (include/np2.h, include/np2_io.h): no exception may leave an extern "C" function, where it would
// end the process in std::terminate.  Every entry point runs its body through abi_guard, which turns an exception into an
// NP2_E_* status and hands the message to the entry point's sink (the context, the I/O thread's slot, the batch driver or
// stderr).  Host-only: no HIP here, so that a plain C++ compiler builds it (tests/tools/abi_guard_test.cpp).
#include "../../include/np2.h"

#include <exception>
#include <stdexcept>
#include <string>

namespace np2h {

struct Np2Error : std::runtime_error {
    int code;
    Np2Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

// Status and message of the exception being handled (call from inside a handler).  `code` is set before the message is
// built, so that it holds even when building the message runs out of memory.
inline void current_error(int &code, std::string &msg) {
    try {
        throw;
    } catch (const Np2Error &e) {
        code = e.code;
        msg = e.what();
    } catch (const std::exception &e) {
        code = NP2_E_NOMEM;
        msg = std::string("unexpected exception: ") + e.what();
    } catch (...) {
        code = NP2_E_NOMEM;
        msg = "unexpected exception";
    }
}

// body() -> status; an exception that escapes it -> on_error(code, message), then the code.  What on_error does (sync a
// stream, flush timers: both may throw) runs inside the guard's own try.
template <class Body, class OnError>
int abi_guard(Body &&body, OnError &&on_error) noexcept {
    try {
        return body();
    } catch (...) {
        int code = NP2_E_NOMEM;
        try {
            std::string msg;
            current_error(code, msg);
            on_error(code, msg);
        } catch (...) { // (the status still gets through)
        }
        return code;
    }
}
// ... for the entry points with no message channel: the status alone
template <class Body>
int abi_guard(Body &&body) noexcept {
    return abi_guard(body, [](int, const std::string &) {});
}

} // namespace np2h
