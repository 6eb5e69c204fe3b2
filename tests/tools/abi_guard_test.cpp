// The C ABI's exception-to-status boundary (nextpolish2_amd/csrc/np2_abi.hpp) on the host: what each kind of exception
// becomes, and when the sink is called.  Prints "ok" and exits 0, or names the first failed check and exits 1.
#include "../../nextpolish2_amd/csrc/np2_abi.hpp"

#include <cstdio>
#include <new>
#include <string>
#include <system_error>

using np2h::abi_guard;
using np2h::Np2Error;

static int failures = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                                \
        }                                                              \
    } while (0)

struct Sink {
    int calls = 0, code = 0;
    std::string msg;
};

template <class Body>
static int run(Body body, Sink &s) {
    return abi_guard(body, [&s](int code, const std::string &msg) {
        ++s.calls;
        s.code = code;
        s.msg = msg;
    });
}

int main() {
    { // a returned code passes through, and the sink is not called
        Sink s;
        CHECK(run([] { return NP2_OK; }, s) == NP2_OK);
        CHECK(run([] { return NP2_E_ARG; }, s) == NP2_E_ARG);
        CHECK(run([] { return 1; }, s) == 1);
        CHECK(s.calls == 0);
    }
    { // Np2Error: its own code and message
        Sink s;
        CHECK(run([]() -> int { throw Np2Error(NP2_E_REFPANIC, "reference would panic: x"); }, s) == NP2_E_REFPANIC);
        CHECK(s.calls == 1 && s.code == NP2_E_REFPANIC && s.msg == "reference would panic: x");
        CHECK(run([]() -> int { throw Np2Error(NP2_E_DEVICE, "hipMalloc: out of memory"); }, s) == NP2_E_DEVICE);
        CHECK(s.calls == 2 && s.code == NP2_E_DEVICE && s.msg == "hipMalloc: out of memory");
    }
    { // any other std::exception: NOMEM, "unexpected exception: " + what()
        Sink s;
        CHECK(run([]() -> int { throw std::bad_alloc(); }, s) == NP2_E_NOMEM);
        CHECK(s.calls == 1 && s.code == NP2_E_NOMEM && s.msg == std::string("unexpected exception: ") + std::bad_alloc().what());
        const std::system_error se(std::make_error_code(std::errc::resource_unavailable_try_again), "thread");
        CHECK(run([&]() -> int { throw se; }, s) == NP2_E_NOMEM);
        CHECK(s.calls == 2 && s.msg == std::string("unexpected exception: ") + se.what());
        CHECK(run([]() -> int { throw std::runtime_error("boom"); }, s) == NP2_E_NOMEM);
        CHECK(s.calls == 3 && s.msg == "unexpected exception: boom");
    }
    { // anything else: NOMEM, "unexpected exception"
        Sink s;
        CHECK(run([]() -> int { throw 42; }, s) == NP2_E_NOMEM);
        CHECK(s.calls == 1 && s.code == NP2_E_NOMEM && s.msg == "unexpected exception");
    }
    { // a sink that throws does not take the status with it
        CHECK(abi_guard([]() -> int { throw Np2Error(NP2_E_ARG, "bad"); }, [](int, const std::string &) { throw std::bad_alloc(); }) ==
              NP2_E_ARG);
    }
    { // without a sink: the status alone
        CHECK(abi_guard([]() -> int { throw Np2Error(NP2_E_UNSUPPORTED, "no"); }) == NP2_E_UNSUPPORTED);
        CHECK(abi_guard([]() -> int { throw std::bad_alloc(); }) == NP2_E_NOMEM);
        CHECK(abi_guard([] { return NP2_OK; }) == NP2_OK);
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
