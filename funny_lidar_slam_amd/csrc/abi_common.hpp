// abi_common.hpp -- what the C ABI layers (abi_*.hpp, all of them parts of the one translation unit fls_reg.hip) share: the back-end and
// the public headers, and the call plumbing written once: the gfx950 device check, "on this handle's device", create and destroy of a handle,
// the argument check of the batch forms, the producer -> consumer stream hand-off.
#pragma once
#include <chrono>
#include "matcher_p2plane_ivox.hpp"
#include "matchers_kd.hpp"
#include "matcher_ndt.hpp"
#include "features_host.hpp"
#include "preprocess_host.hpp"
#include "loop_closure.hpp"
#include "replicas.hpp"
#include "keyframes.hpp"
#include "localmap.hpp"
#include "kernels_debug_linalg.hpp"
#include "kernels_debug_fit.hpp"
#include "../../include/fls_keyframes.h"
#include "../../include/fls_localmap.h"
#include "../../include/fls_batch.h"
#include "../../include/fls_batch_ivox.h"
#include "../../include/fls_debug_linalg.h"
#include "../../include/fls_debug_fit.h"
#include "../../include/fls_debug_ndt.h"
#include "../../include/fls_debug_loop.h"
#include "../../include/fls_debug_knn.h"
#include "../../include/fls_debug_ivox_knn.h"
#include "../../include/fls_map_kd.h"
#include <new>
#include <type_traits>

namespace fls {

// FLS_OK: device_id names a gfx950 device.  FLS_ERR_DEVICE: the device count fails, the id is out of range or the device is another
// architecture (there is no CPU fallback).  Silent unless `say` (fls_create names the device it refuses); does not throw.
inline fls_status gfx950_device(int device_id, bool say = false) {
    int n = 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n || hipGetDeviceProperties(&prop, device_id) != hipSuccess) return FLS_ERR_DEVICE;
    const char* arch = prop.gcnArchName;
    if (std::strncmp(arch, "gfx950", 6) == 0) return FLS_OK;
    if (say) std::fprintf(stderr, "[fls_reg] device %d is %s; this library is built for gfx950 only\n", device_id, arch);
    return FLS_ERR_DEVICE;
}

// guarded(), with a failed device allocation reported as what it is (the keyframe and local-map stores, whose size the caller decides)
template <typename F>
fls_status guarded_nomem(F&& f) {
    return guarded([&]() -> fls_status {
        try {
            return f();
        } catch (const HipError& e) {
            if (e.code != hipErrorOutOfMemory) throw;
            (void)hipGetLastError();
            return FLS_ERR_NOMEM;
        }
    });
}

// body() on the handle's device, no exception out: the form of every entry point that launches or copies for a handle
template <class H, class F>
fls_status on_device(H* h, F&& body) {
    return guarded([&]() -> fls_status { FLS_HIP(hipSetDevice(h->device)); return body(); });
}
template <class H, class F>
fls_status on_device_nomem(H* h, F&& body) {
    return guarded_nomem([&]() -> fls_status { FLS_HIP(hipSetDevice(h->device)); return body(); });
}

enum class Guard { kPlain, kNomem };  // guarded() or guarded_nomem()

// A T on device_id into *out (which the caller has set to null): the device check, `set` fills what init() reads besides the device,
// init() (a status, or void where it can only throw).  Nothing is left behind on failure.
template <class T, class Out, class Set>
fls_status create_handle(int device_id, Out* out, Set&& set, Guard guard = Guard::kPlain, bool say = false) {
    const auto body = [&]() -> fls_status {
        const fls_status dev = gfx950_device(device_id, say);
        if (dev != FLS_OK) return dev;
        std::unique_ptr<T> t(new T());
        t->device = device_id;
        set(*t);
        if constexpr (std::is_void_v<decltype(t->init())>) {
            t->init();
        } else {
            const fls_status rc = t->init();
            if (rc != FLS_OK) return rc;
        }
        *out = t.release();
        return FLS_OK;
    };
    return guard == Guard::kNomem ? guarded_nomem(body) : guarded(body);
}

// the handle's device buffers are freed on its device; `first` runs there before the delete
template <class H, class F>
void destroy_handle(H* h, F&& first) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    first();
    delete h;
}
template <class H>
void destroy_handle(H* h) { destroy_handle(h, [] {}); }

// The arguments the batch forms share, then call().  The forms differ in two ways: check_rows tests src0[j] job by job (the replica forms
// leave that to the per-device calls they make), and with empty_is_ok a batch of no jobs is FLS_OK without a call.
template <class H, class F>
fls_status batch_call(H* h, size_t n_jobs, const float* const* src0, const size_t* n0, const float* const* src1, const size_t* n1, int stride, const double* T,
                      bool check_rows, bool empty_is_ok, F&& call) {
    if (!h || stride < 3 || (n_jobs && (!src0 || !n0 || !T))) return FLS_ERR_INVALID;
    if ((src1 == nullptr) != (n1 == nullptr)) return FLS_ERR_INVALID;
    for (size_t j = 0; check_rows && j < n_jobs; ++j)
        if (!src0[j] && n0[j]) return FLS_ERR_INVALID;
    if (empty_is_ok && n_jobs == 0) return FLS_OK;
    return call();
}

// A front end's device cloud into a consumer's stream: the copies call() queues on `consumer` wait for everything queued on the producer's
// stream (the scan or the extraction that made the cloud), and the producer's next writes wait for the copies.
template <class P, class F>
fls_status handoff(P& producer, hipStream_t consumer, F&& call) {
    FLS_HIP(hipEventRecord(producer.ev_ready, producer.stream));
    FLS_HIP(hipStreamWaitEvent(consumer, producer.ev_ready, 0));
    const fls_status rc = call();
    FLS_HIP(hipEventRecord(producer.next_consumed_event(), consumer));
    return rc;
}

inline bool pre_cloud_ok(int what) { return what == FLS_PRE_ORDERED || what == FLS_PRE_PLANAR || what == FLS_PRE_PLANAR_FILTERED; }

}  // namespace fls

using namespace fls;
