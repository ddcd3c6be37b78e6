// abi_debug_voxel.hpp -- test hooks of fls_reg.h for the device VoxelGrid filter and its exact sort (fls_voxel_grid_cloud's device mode is
// fls_debug_voxel_grid).
#pragma once
#include "abi_common.hpp"

extern "C" {

fls_status fls_debug_voxel_grid(int device_id, const float* pts, size_t n, int stride, float leaf, float* out, size_t cap, size_t* n_out) {
    if (!pts || !n_out || stride < 3 || !(leaf > 0.f) || (cap && !out)) return FLS_ERR_INVALID;
    *n_out = 0;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        DevScan raw;
        DeviceVoxelGrid vg;
        raw.upload_raw(pts, n, stride, nullptr, true);
        if (n == 0 || !vg.run(raw.x.p, raw.y.p, raw.z.p, raw.xyz.p + 3 * n, n, leaf, nullptr)) return FLS_ERR_STATE;
        *n_out = vg.n_out;
        if (vg.n_out > cap) return FLS_ERR_INVALID;
        std::vector<float> tmp;
        const std::vector<PtI> c = vg.download(nullptr, tmp);
        std::memcpy(out, c.data(), c.size() * sizeof(PtI));
        return FLS_OK;
    });
}

fls_status fls_debug_voxel_grid_timed(int device_id, const float* pts, size_t n, int stride, float leaf, int reps, double* ms, size_t* n_out) {
    if (!pts || !n_out || !ms || reps <= 0 || stride < 3 || !(leaf > 0.f)) return FLS_ERR_INVALID;
    *n_out = 0;
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        DevScan raw;
        DeviceVoxelGrid vg;  // one filter object for all repetitions: the buffers are allocated by the first one, as in a matcher
        raw.upload_raw(pts, n, stride, nullptr, true);
        FLS_HIP(hipDeviceSynchronize());
        for (int r = 0; r < reps; ++r) {
            const auto t0 = std::chrono::steady_clock::now();
            const bool ok = n != 0 && vg.run(raw.x.p, raw.y.p, raw.z.p, raw.xyz.p + 3 * n, n, leaf, nullptr);
            FLS_HIP(hipStreamSynchronize(nullptr));
            ms[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (!ok) return FLS_ERR_STATE;
        }
        *n_out = vg.n_out;
        return FLS_OK;
    });
}

fls_status fls_debug_exact_sort(int device_id, uint32_t* key, uint32_t* val, size_t n, int on_host) {
    if ((!key || !val) && n) return FLS_ERR_INVALID;
    if (on_host != 0 && on_host != 1 && on_host != 2) return FLS_ERR_INVALID;
    if (on_host == 1)
        return guarded([&]() -> fls_status {  // (an allocation failure must not cross the C ABI)
            std::vector<VoxelLeafRec> r(n);
            for (size_t i = 0; i < n; ++i) r[i] = VoxelLeafRec{key[i], val[i]};
            std::sort(r.begin(), r.end());  // operator< compares idx only: libstdc++'s introsort decides the order of equal keys
            for (size_t i = 0; i < n; ++i) { key[i] = r[i].idx; val[i] = r[i].pt; }
            return FLS_OK;
        });
    return guarded([&]() -> fls_status {
        FLS_HIP(hipSetDevice(device_id));
        if (n == 0) return FLS_OK;
        DevBuf<unsigned> dk, dv;
        dk.reserve(n); dv.reserve(n);
        FLS_HIP(hipMemcpy(dk.p, key, n * sizeof(unsigned), hipMemcpyHostToDevice));
        FLS_HIP(hipMemcpy(dv.p, val, n * sizeof(unsigned), hipMemcpyHostToDevice));
        DeviceExactSort es;  // (on_host 0 and 2: the same launch sequence, the one the VoxelGrid queues)
        if (!es.run_sync(dk.p, dv.p, n)) return FLS_ERR_STATE;
        FLS_HIP(hipMemcpy(key, dk.p, n * sizeof(unsigned), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(val, dv.p, n * sizeof(unsigned), hipMemcpyDeviceToHost));
        return FLS_OK;
    });
}

int fls_debug_exact_sort_marks(unsigned* out, int n) {  // diagnostics only: progress stamps of the sort in flight
    if (!out || n <= 0) return -1;
    EsMailbox* m = es_debug_mailbox().load(std::memory_order_acquire);
    if (!m) return -1;
    for (int i = 0; i < n && i < 12; ++i) out[i] = __atomic_load_n(&m->mark[i], __ATOMIC_RELAXED);
    return 0;
}

}  // extern "C"
