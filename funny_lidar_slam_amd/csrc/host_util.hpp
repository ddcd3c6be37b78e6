// host_util.hpp -- host-side plumbing: HIP error handling, the exception-to-status ladder, the host-mapped-word spin wait, the
// bools-to-template-arguments dispatch, device buffers, pinned staging.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>
#include <stdexcept>
#include "../../include/fls_reg.h"
#include "../../include/fls_knn_order.h"

namespace fls {

struct HipError : std::runtime_error {
    hipError_t code;
    HipError(hipError_t c, const char* what) : std::runtime_error(what), code(c) {}
};

#define FLS_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            char _buf[256];                                                                    \
            snprintf(_buf, sizeof(_buf), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            throw ::fls::HipError(_e, _buf);                                                   \
        }                                                                                      \
    } while (0)

// No exception crosses the C ABI or leaves a host thread: f()'s status, or the status its exception stands for.  `context` (with
// `index`) names the thread in the message: "[fls_reg] batch lane 3: ...".
template <typename F>
fls_status guarded(F&& f, const char* context = nullptr, size_t index = 0) {
    try {
        return f();
    } catch (const HipError& e) {
        if (context) std::fprintf(stderr, "[fls_reg] %s %zu: %s\n", context, index, e.what());
        else std::fprintf(stderr, "[fls_reg] %s\n", e.what());
        return FLS_ERR_DEVICE;
    } catch (const std::bad_alloc&) {
        return FLS_ERR_NOMEM;
    } catch (...) {
        return FLS_ERR_INVALID;
    }
}

// FLS_HOST_TIMING=1: host-side timing lines on stderr
inline bool host_timing_enabled() {
    const char* e = std::getenv("FLS_HOST_TIMING");
    return e && std::atoi(e) != 0;
}

// Wait for a result the device publishes in host-mapped memory, without a blocking synchronisation: spin on ready() (the poll of that word).
// Every 0x4000 polls the stream state is consulted, so that a faulted kernel cannot hang the host: an error throws, a drained stream ends the
// wait.  true: ready() held; false: the stream drained first (whatever the device was going to write is there: the caller re-reads).
template <class F>
bool spin_until(hipStream_t stream, F&& ready) {
    for (unsigned long long spin = 1;; ++spin) {
        if (ready()) return true;
        if ((spin & 0x3fffu) == 0) {
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipSuccess) return false;
            if (q != hipErrorNotReady) FLS_HIP(q);
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
}

// Run-time bools into template arguments: with_bools(f, a, b, ...) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...), so a generic
// lambda can name kernel<A.value, B.value, ...> -- one instantiation per combination, selected by a ladder of ifs written here once.
template <class F>
void with_bools(F&& f) { f(); }
template <class F, class... Rest>
void with_bools(F&& f, const bool b, const Rest... rest) {
    if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// growable device buffer; contents are NOT preserved on growth unless keep=true
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    void reserve(size_t n, bool keep = false, hipStream_t s = nullptr, bool zero_new = false) {
        if (n <= cap) return;
        size_t nc = cap ? cap : 1;
        while (nc < n) nc = nc + nc / 2 + 64;
        T* q = nullptr;
        FLS_HIP(hipMalloc(&q, nc * sizeof(T)));
        if (zero_new) FLS_HIP(hipMemsetAsync(q, 0, nc * sizeof(T), s));
        if (keep && p && cap) FLS_HIP(hipMemcpyAsync(q, p, cap * sizeof(T), hipMemcpyDeviceToDevice, s));
        // growth is rare (buffers only grow): wait for the WHOLE device before the old allocation goes away -- kernels still
        // queued on any of the handle's streams (e.g. exit-at-once launches behind a converged Match) may hold the pointer
        if (p) { FLS_HIP(hipDeviceSynchronize()); FLS_HIP(hipFree(p)); }
        p = q;
        cap = nc;
    }
};

template <typename T>
struct PinnedBuf {
    T* p = nullptr;
    size_t cap = 0;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    void reserve(size_t n) {
        if (n <= cap) return;
        if (p) FLS_HIP(hipHostFree(p));
        p = nullptr;
        size_t nc = n + n / 4 + 64;
        FLS_HIP(hipHostMalloc(&p, nc * sizeof(T), hipHostMallocDefault));
        cap = nc;
    }
};

}  // namespace fls
