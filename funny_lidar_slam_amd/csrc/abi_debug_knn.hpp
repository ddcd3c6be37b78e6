// abi_debug_knn.hpp -- test hooks of the cooperative grid k-NN kernels (include/fls_debug_knn.h): one search (map cloud, its cell grid, queries,
// the three output arrays of grid_knn_kernel<5>) with buffers of its own on the null stream; the outputs are filled with the byte 0x7b before
// the launch, so a row the kernel did not write shows.
#pragma once
#include "abi_common.hpp"

namespace {

fls_status debug_knn_device(int device_id) {
    const fls_status dev = gfx950_device(device_id);
    if (dev == FLS_OK) FLS_HIP(hipSetDevice(device_id));
    return dev;
}
inline bool debug_knn_common_ok(const float* map, int nm, const float* query, int nq, int stride, float cell, int host_grid) {
    return map && query && nm >= 0 && nq >= 0 && stride >= 3 && cell > 0.f && std::isfinite(cell) && (host_grid == 0 || host_grid == 1);
}
struct DebugKnnSide {
    LoopMatcher::DevCloud map, query;
    CellGridImage grid;
    DeviceGridBuilder builder;
    DevBuf<float4> pts;
    DevBuf<unsigned char> cnt, flag;
    DevBuf<float> kth;
    int nq = 0;
    // the grid as KdLocalMap::rebuild (kd_map.hpp) makes it: on the device, else (or with host_grid) on the host
    fls_status prepare_grid(const float* m, int nm, const float* q, int n_query, int stride, float cell, int rings, bool host_grid) {
        const std::vector<PtI> mc = cloud_from(m, size_t(nm), stride), qc = cloud_from(q, size_t(n_query), stride);
        nq = n_query;
        map.upload(mc, nullptr);
        query.upload(qc, nullptr);
        if (!host_grid && builder.run(grid, map.x(), map.y(), map.z(), mc.size(), cell, rings, false, nullptr)) return FLS_OK;
        return grid.build(mc, cell, nullptr, rings, false);
    }
    void prepare_outputs() {
        pts.reserve(size_t(nq) * 5); cnt.reserve(size_t(nq)); flag.reserve(size_t(nq)); kth.reserve(size_t(nq));
        FLS_HIP(hipMemset(pts.p, 0x7b, size_t(nq) * 5 * sizeof(float4)));
        FLS_HIP(hipMemset(cnt.p, 0x7b, size_t(nq)));
        FLS_HIP(hipMemset(flag.p, 0x7b, size_t(nq)));
        FLS_HIP(hipMemset(kth.p, 0x7b, size_t(nq) * sizeof(float)));
    }
    GridKnnArgs args(float gate) { return GridKnnArgs{query.x(), query.y(), query.z(), nq, cell_dev(grid), gate, pts.p, cnt.p, kth.p, flag.p}; }
    void fetch(float* out_pts, uint8_t* out_cnt, float* out_kth, int32_t* out_has_window) {
        FLS_HIP(hipMemcpy(out_pts, pts.p, size_t(nq) * 5 * sizeof(float4), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(out_cnt, cnt.p, size_t(nq), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(out_kth, kth.p, size_t(nq) * sizeof(float), hipMemcpyDeviceToHost));
        *out_has_window = grid.have_window ? 1 : 0;
    }
};
inline void debug_knn_empty(int nq, float* out_pts, uint8_t* out_cnt, float* out_kth, int32_t* out_has_window) {
    const int32_t none = -1;
    for (size_t i = 0; i < size_t(nq) * 5; ++i) {
        out_pts[4 * i] = out_pts[4 * i + 1] = out_pts[4 * i + 2] = 0.f;
        std::memcpy(out_pts + 4 * i + 3, &none, sizeof(none));
    }
    for (int i = 0; i < nq; ++i) { out_cnt[i] = 0; out_kth[i] = INFINITY; }
    *out_has_window = 0;
}
inline Pose16 debug_knn_pose(const double* T16) { Pose16 T; std::memcpy(T.m, T16, sizeof(T.m)); return T; }

}  // namespace

extern "C" {

int fls_debug_knn_revision(void) { return FLS_DEBUG_KNN_REVISION; }

// include/fls_debug_ivox_knn.h: the limits of the iVox kNN kernel's shared-run gate, as compiled
int fls_debug_ivox_knn_revision(void) { return FLS_DEBUG_IVOX_KNN_REVISION; }
fls_status fls_debug_ivox_knn_limits(int* r_max, int* cap) {
    if (!r_max || !cap) return FLS_ERR_INVALID;
    *r_max = kIvoxKnnRunMax;
    *cap = kIvoxKnnStageCap;
    return FLS_OK;
}

fls_status fls_debug_grid_knn5(int device_id, const float* map, int nm, const float* query, int nq, int stride, float cell, int rings, float gate,
                               const double* T16, int host_grid, float* out_pts, uint8_t* out_cnt, float* out_kth, int32_t* out_has_window) {
    if (!debug_knn_common_ok(map, nm, query, nq, stride, cell, host_grid) || !T16 || !out_pts || !out_cnt || !out_kth || !out_has_window || (rings != 1 && rings != 2) ||
        gate != gate)
        return FLS_ERR_INVALID;
    if (nm == 0 || nq == 0) { debug_knn_empty(nq, out_pts, out_cnt, out_kth, out_has_window); return FLS_OK; }
    return guarded([&]() -> fls_status {
        fls_status rc = debug_knn_device(device_id);
        if (rc != FLS_OK) return rc;
        DebugKnnSide s;
        rc = s.prepare_grid(map, nm, query, nq, stride, cell, rings, host_grid != 0);
        if (rc != FLS_OK) return rc;
        s.prepare_outputs();
        DevBuf<GnState> st;
        st.reserve(1);
        FLS_HIP(hipMemset(st.p, 0, sizeof(GnState)));
        const GridKnnArgs a = s.args(gate);
        const dim3 knn_grid_dim(knn_grid_blocks(size_t(nq)));
        const Pose16 T0 = debug_knn_pose(T16);
        if (std::isinf(gate))  // (FeatureDev::launch)
            hipLaunchKernelGGL((grid_knn_kernel<5, false, true>), knn_grid_dim, dim3(256), 0, nullptr, a.sx, a.sy, a.sz, a.n, (const GnState*)st.p, 1, T0, a.cg, gate, a.nn_pts,
                               a.nn_cnt, a.kth_d2, a.flag_to_clear);
        else
            hipLaunchKernelGGL((grid_knn_kernel<5, false>), knn_grid_dim, dim3(256), 0, nullptr, a.sx, a.sy, a.sz, a.n, (const GnState*)st.p, 1, T0, a.cg, gate, a.nn_pts,
                               a.nn_cnt, a.kth_d2, a.flag_to_clear);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipDeviceSynchronize());
        s.fetch(out_pts, out_cnt, out_kth, out_has_window);
        return FLS_OK;
    });
}

fls_status fls_debug_grid_knn5_dual(int device_id, const float* map_a, int nm_a, const float* query_a, int nq_a, float cell_a, int rings_a, float gate_a,
                                    const float* map_b, int nm_b, const float* query_b, int nq_b, float cell_b, int rings_b, float gate_b, int stride,
                                    const double* T16, int host_grid, float* out_pts_a, uint8_t* out_cnt_a, float* out_kth_a, int32_t* out_has_window_a,
                                    float* out_pts_b, uint8_t* out_cnt_b, float* out_kth_b, int32_t* out_has_window_b) {
    if (!debug_knn_common_ok(map_a, nm_a, query_a, nq_a, stride, cell_a, host_grid) || !debug_knn_common_ok(map_b, nm_b, query_b, nq_b, stride, cell_b, host_grid) || !T16 ||
        !out_pts_a || !out_cnt_a || !out_kth_a || !out_has_window_a || !out_pts_b || !out_cnt_b || !out_kth_b || !out_has_window_b || (rings_a != 1 && rings_a != 2) ||
        (rings_b != 1 && rings_b != 2) || !std::isfinite(gate_a) || !std::isfinite(gate_b) || nm_a == 0 || nq_a == 0 || nm_b == 0 || nq_b == 0)
        return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        fls_status rc = debug_knn_device(device_id);
        if (rc != FLS_OK) return rc;
        DebugKnnSide sa, sb;
        rc = sa.prepare_grid(map_a, nm_a, query_a, nq_a, stride, cell_a, rings_a, host_grid != 0);
        if (rc != FLS_OK) return rc;
        rc = sb.prepare_grid(map_b, nm_b, query_b, nq_b, stride, cell_b, rings_b, host_grid != 0);
        if (rc != FLS_OK) return rc;
        sa.prepare_outputs();
        sb.prepare_outputs();
        DevBuf<GnState> st;
        st.reserve(1);
        FLS_HIP(hipMemset(st.p, 0, sizeof(GnState)));
        const int ka = int(knn_grid_blocks(size_t(nq_a))), kb = int(knn_grid_blocks(size_t(nq_b)));  // (LoamFullMatcher::match_resident)
        hipLaunchKernelGGL((grid_knn_dual_kernel<5, false>), dim3(unsigned(ka + kb)), dim3(256), 0, nullptr, (const GnState*)st.p, 1, debug_knn_pose(T16), sa.args(gate_a),
                           sb.args(gate_b), ka);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipDeviceSynchronize());
        sa.fetch(out_pts_a, out_cnt_a, out_kth_a, out_has_window_a);
        sb.fetch(out_pts_b, out_cnt_b, out_kth_b, out_has_window_b);
        return FLS_OK;
    });
}

fls_status fls_debug_icp_knn1(int device_id, const float* map, int nm, const float* query, int nq, int stride, float cell, double max_corr_sq,
                              const double* T16, int host_grid, int32_t* out_id, uint8_t* out_eff, int32_t* out_has_window) {
    if (!debug_knn_common_ok(map, nm, query, nq, stride, cell, host_grid) || !T16 || !out_id || !out_eff || !out_has_window || !(max_corr_sq > 0.0) ||
        !std::isfinite(max_corr_sq))
        return FLS_ERR_INVALID;
    if (nm == 0 || nq == 0) {
        for (int i = 0; i < nq; ++i) { out_id[i] = -1; out_eff[i] = 0; }
        *out_has_window = 0;
        return FLS_OK;
    }
    return guarded([&]() -> fls_status {
        fls_status rc = debug_knn_device(device_id);
        if (rc != FLS_OK) return rc;
        DebugKnnSide s;
        rc = s.prepare_grid(map, nm, query, nq, stride, cell, 1, host_grid != 0);
        if (rc != FLS_OK) return rc;
        const unsigned rows = knn_grid_blocks(size_t(nq));
        DevBuf<GnState> st;
        DevBuf<int> nn_id;
        DevBuf<unsigned char> eff;
        DevBuf<double> partials;
        st.reserve(1); nn_id.reserve(size_t(nq)); eff.reserve(size_t(nq)); partials.reserve(size_t(rows) * kPartialStride);
        FLS_HIP(hipMemset(st.p, 0, sizeof(GnState)));
        FLS_HIP(hipMemset(nn_id.p, 0x7b, size_t(nq) * sizeof(int)));
        FLS_HIP(hipMemset(eff.p, 0x7b, size_t(nq)));
        const LuTailArgs tail{0, 0.0, 0.0, 0, nullptr, 0u};
        // (IcpMatcher::match_launch: gate = float(point_search_thres), max_corr = point_search_thres; no ticket: the tail does not run)
        hipLaunchKernelGGL(icp_knn_fit_kernel, dim3(rows), dim3(256), 0, nullptr, s.query.x(), s.query.y(), s.query.z(), nq, st.p, 1, debug_knn_pose(T16), cell_dev(s.grid),
                           float(max_corr_sq), max_corr_sq, nn_id.p, eff.p, partials.p, (unsigned*)nullptr, kTicketShards, tail);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipDeviceSynchronize());
        FLS_HIP(hipMemcpy(out_id, nn_id.p, size_t(nq) * sizeof(int), hipMemcpyDeviceToHost));
        FLS_HIP(hipMemcpy(out_eff, eff.p, size_t(nq), hipMemcpyDeviceToHost));
        *out_has_window = s.grid.have_window ? 1 : 0;
        return FLS_OK;
    });
}

}  // extern "C"
