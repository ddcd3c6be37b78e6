// abi_loop_device.hpp -- include/fls_loop_device.h (the loop-closure Match from device clouds) and include/fls_debug_loop_leaves.h (the test
// hooks of its leaf build).  Includes the leaf-build kernels and LoopMatcher::match with its two entries (loop_device.hpp), which this translation unit
// names last: the code object keeps the order of every kernel in front of them.
#pragma once
#include "abi_matcher.hpp"
#include "abi_stores.hpp"
#include "abi_debug_loop.hpp"
#include "loop_device.hpp"
#include "../../include/fls_loop_device.h"
#include "../../include/fls_debug_loop_leaves.h"

namespace {

constexpr size_t kLoopDeviceMaxPoints = 4000000000u;

bool loop_planes_ok(const float* x, const float* y, const float* z, const float* in, size_t n) {
    if (n > kLoopDeviceMaxPoints) return false;
    if (n && (!x || !y || !z)) return false;
    for (const float* p : {x, y, z, in})
        if (reinterpret_cast<uintptr_t>(p) % sizeof(float) != 0) return false;
    return true;
}

// the Match on the device's own matcher, under its run mutex; `after`: an event the matcher's stream waits for first (may be null)
fls_status loop_match_device_on(int device_id, const LoopMatcher::DevInput& src, const LoopMatcher::DevInput& tgt, hipEvent_t after, double* T, float* fitness,
                                fls_loop_stats* stats) {
    *fitness = std::numeric_limits<float>::max();
    if (stats) std::memset(stats, 0, sizeof(*stats));
    return guarded([&]() -> fls_status {
        const bool timing = host_timing_enabled();
        const auto t0 = std::chrono::steady_clock::now();
        LoopMatcher* m = nullptr;
        const fls_status got = loop_matcher_for(device_id, m);
        if (got != FLS_OK) return got;
        std::lock_guard<std::mutex> run_lk(m->run_mx);
        if (timing) std::fprintf(stderr, "[fls loop] ms: matcher set-up %.2f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        FLS_HIP(hipSetDevice(m->device));
        if (after) FLS_HIP(hipStreamWaitEvent(m->stream, after, 0));
        const fls_status rc = m->run_device(src, tgt, T, fitness);
        if (stats) *stats = m->st;
        return rc;
    });
}

}  // namespace

extern "C" {

int fls_loop_device_revision(void) { return FLS_LOOP_DEVICE_REVISION; }

fls_status fls_loop_match_device(int device_id, const float* src_x, const float* src_y, const float* src_z, const float* src_i, size_t n_src, const float* tgt_x,
                                 const float* tgt_y, const float* tgt_z, const float* tgt_i, size_t n_tgt, double T[16], float* fitness, fls_loop_stats* stats) {
    if (!T || !fitness || !loop_planes_ok(src_x, src_y, src_z, src_i, n_src) || !loop_planes_ok(tgt_x, tgt_y, tgt_z, tgt_i, n_tgt)) return FLS_ERR_INVALID;
    const LoopMatcher::DevInput src{src_x, src_y, src_z, src_i, n_src}, tgt{tgt_x, tgt_y, tgt_z, tgt_i, n_tgt};
    return loop_match_device_on(device_id, src, tgt, nullptr, T, fitness, stats);
}

fls_status fls_keyframes_loop_match_device(fls_keyframes_handle h, const int32_t* src_ids, const double* src_poses, size_t n_src, const int32_t* tgt_ids,
                                           const double* tgt_poses, size_t n_tgt, double T[16], float* fitness, fls_loop_stats* stats) {
    if (!h || !T || !fitness || (n_src && (!src_ids || !src_poses)) || (n_tgt && (!tgt_ids || !tgt_poses)) || !kf_ids_ok(*h, src_ids, n_src) ||
        !kf_ids_ok(*h, tgt_ids, n_tgt))
        return FLS_ERR_INVALID;
    size_t ns = 0, nt = 0;
    const fls_status rc = on_device_nomem(h, [&] {  // GetSubMap's leaf (loop_closure.cpp:219); both merges queued, neither waited for
        const fls_status a = h->merge(src_ids, src_poses, n_src, 0.2f, 0.f, nullptr, 0, &ns, nullptr, 0);
        const fls_status b = a != FLS_OK ? a : h->merge(tgt_ids, tgt_poses, n_tgt, 0.2f, 0.f, nullptr, 0, &nt, nullptr, 1);
        if (b != FLS_OK) { FLS_HIP(hipStreamSynchronize(h->stream)); return b; }
        FLS_HIP(hipEventRecord(h->ev_sub, h->stream));
        return FLS_OK;
    });
    if (rc != FLS_OK) return rc;
    const auto planes = [](const DevBuf<float>& b, size_t n) {
        return n ? LoopMatcher::DevInput{b.p, b.p + n, b.p + 2 * n, b.p + 3 * n, n} : LoopMatcher::DevInput{};
    };
    const fls_status out = loop_match_device_on(h->device, planes(h->d_sub[0], ns), planes(h->d_sub[1], nt), h->ev_sub, T, fitness, stats);
    if (out != FLS_OK) (void)on_device(h, [&] { FLS_HIP(hipStreamSynchronize(h->stream)); return FLS_OK; });  // (a Match that stopped early: the merges still end here)
    return out;
}

size_t fls_loop_device_stat(int device_id, int slot) {
    if (slot < 0 || slot >= int(LoopMatcher::kStatSlots)) return 0;
    size_t v = 0;
    (void)guarded([&]() -> fls_status {
        LoopMatcher* m = nullptr;
        const fls_status got = loop_matcher_for(device_id, m);
        if (got != FLS_OK) return got;
        std::lock_guard<std::mutex> run_lk(m->run_mx);
        v = size_t(m->dstat[slot]);
        return FLS_OK;
    });
    return v;
}

// ---- include/fls_debug_loop_leaves.h ------------------------------------------------------------------------------------------------
int fls_debug_loop_leaves_revision(void) { return FLS_DEBUG_LOOP_LEAVES_REVISION; }

fls_status fls_debug_loop_leaves(int device_id, const float* tgt, int nt, int stride, float resolution, int on_device, int32_t* cell, int32_t* n_points,
                                 double* mean, double* icov, float* centroid, int cap, int32_t* n_leaves, int32_t* sparse) {
    if (!tgt || !n_leaves || !sparse || nt < 0 || stride < 3 || cap < 0 || (cap && (!cell || !n_points || !mean || !icov || !centroid)) || !(resolution > 0.f) ||
        !std::isfinite(resolution) || (on_device != 0 && on_device != 1))
        return FLS_ERR_INVALID;
    *n_leaves = 0;
    *sparse = 0;
    if (nt == 0) return FLS_OK;
    return debug_loop_run(device_id, [&](LoopMatcher& m) -> fls_status {
        LoopMatcher::Filtered t;
        t.dev = &m.tgt_filtered;
        t.set_rows(cloud_from(tgt, size_t(nt), stride));
        LoopMatcher::TargetLeaves& tl = m.leaves;
        if (!m.target_leaves(t, resolution, tl, on_device != 0, on_device != 0)) return FLS_OK;
        m.download_leaves(tl);
        *n_leaves = int32_t(tl.rows);
        *sparse = tl.sparse ? 1 : 0;
        if (tl.rows > size_t(cap)) return FLS_ERR_INVALID;
        for (size_t r = 0; r < tl.rows; ++r) { cell[r] = tl.row_cell[r]; n_points[r] = tl.row_n[r]; }
        std::memcpy(mean, tl.mean.data(), 3 * tl.rows * sizeof(double));
        std::memcpy(icov, tl.icov.data(), 9 * tl.rows * sizeof(double));
        std::memcpy(centroid, tl.centroid.data(), 3 * tl.rows * sizeof(float));
        return FLS_OK;
    });
}

fls_status fls_debug_loop_ndt_device(int device_id, const float* src, int ns, const float* tgt, int nt, int stride, float resolution, const double* p,
                                     int want_hessian, double* score, double* grad, double* hess, int64_t* pairs, int32_t* leaves, int32_t* sparse) {
    return debug_loop_ndt(device_id, src, ns, tgt, nt, stride, resolution, p, want_hessian, score, grad, hess, pairs, leaves, sparse, true);
}

}  // extern "C"
