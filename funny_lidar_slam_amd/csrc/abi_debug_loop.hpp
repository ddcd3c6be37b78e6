// abi_debug_loop.hpp -- test hooks of the stages of the loop-closure matcher (include/fls_debug_loop.h): each stages the buffers the test supplies
// on the device's own LoopMatcher (loop_matcher_for, abi_matcher.hpp) and calls the stage function the Match calls.
#pragma once
#include "abi_matcher.hpp"

namespace {

// the hook's body on the device's own LoopMatcher, under its run mutex (the ticket is NOT reset: see the header)
template <class F>
fls_status debug_loop_run(int device_id, F&& body) {
    return guarded([&]() -> fls_status {
        LoopMatcher* m = nullptr;
        const fls_status got = loop_matcher_for(device_id, m);
        if (got != FLS_OK) return got;
        std::lock_guard<std::mutex> run_lk(m->run_mx);
        m->read_env();
        FLS_HIP(hipSetDevice(m->device));
        return body(*m);
    });
}

// a hook's cloud: the rows the test supplies, uploaded into `dev`
LoopMatcher::Filtered debug_loop_cloud(LoopMatcher& m, LoopMatcher::DevCloud& dev, const float* pts, int n, int stride) {
    LoopMatcher::Filtered c;
    c.dev = &dev;
    c.set_rows(cloud_from(pts, size_t(n), stride));
    m.planes(c);
    return c;
}

LoopMat4f debug_loop_mat(const float* T) { LoopMat4f r; for (int i = 0; i < 16; ++i) r.m[i] = T[i]; return r; }

// fls_debug_loop_ndt (the leaves by build_target) and fls_debug_loop_ndt_device (on the device, counted): the target's leaves, then ONE ndt_eval
fls_status debug_loop_ndt(int device_id, const float* src, int ns, const float* tgt, int nt, int stride, float resolution, const double* p, int want_hessian,
                          double* score, double* grad, double* hess, int64_t* pairs, int32_t* leaves, int32_t* sparse, bool on_device) {
    if (!src || !tgt || !p || !score || !grad || !hess || !pairs || !leaves || !sparse || ns < 0 || nt < 0 || stride < 3 || !(resolution > 0.f) ||
        !std::isfinite(resolution))
        return FLS_ERR_INVALID;
    *score = 0.0; *pairs = 0; *leaves = 0; *sparse = 0;
    for (int i = 0; i < 6; ++i) grad[i] = 0.0;
    if (want_hessian) for (int i = 0; i < 36; ++i) hess[i] = 0.0;
    if (ns == 0 || nt == 0) return FLS_OK;
    return debug_loop_run(device_id, [&](LoopMatcher& m) -> fls_status {
        LoopMatcher::Filtered t;
        t.dev = &m.tgt_filtered;
        t.set_rows(cloud_from(tgt, size_t(nt), stride));
        if (!m.target_leaves(t, resolution, m.leaves, on_device, on_device)) return FLS_OK;
        *leaves = int32_t(m.leaves.rows);
        *sparse = m.leaves.sparse ? 1 : 0;
        LoopMatcher::NdtRun run;
        run.resolution = resolution;
        loop::ndt_gauss(run);
        debug_loop_cloud(m, m.src_dev, src, ns, stride);
        run.src = &m.src_dev;
        run.tl = &m.leaves;
        *score = m.ndt_eval(run, loop::pose_xyz(p), p, want_hessian != 0, grad, hess);
        *pairs = int64_t(m.mail_host->v[want_hessian ? 43 : 7]);
        return FLS_OK;
    });
}

}  // namespace

extern "C" {

int fls_debug_loop_revision(void) { return FLS_DEBUG_LOOP_REVISION; }

fls_status fls_debug_loop_ndt(int device_id, const float* src, int ns, const float* tgt, int nt, int stride, float resolution, const double* p,
                              int want_hessian, double* score, double* grad, double* hess, int64_t* pairs, int32_t* leaves, int32_t* sparse) {
    return debug_loop_ndt(device_id, src, ns, tgt, nt, stride, resolution, p, want_hessian, score, grad, hess, pairs, leaves, sparse, false);
}

fls_status fls_debug_loop_gicp_cov(int device_id, const float* cloud, int n, int stride, float cell, double epsilon, int host_grid, double* cov) {
    if (!cloud || !cov || n < 20 || stride < 3 || !(cell > 0.f) || !std::isfinite(cell) || !(epsilon > 0.0) || (host_grid != 0 && host_grid != 1)) return FLS_ERR_INVALID;
    return debug_loop_run(device_id, [&](LoopMatcher& m) -> fls_status {
        LoopMatcher::Filtered c = debug_loop_cloud(m, m.src_own, cloud, n, stride);
        const fls_status rc = m.cell_grid(m.src_grid, c, cell, false, host_grid != 0);
        if (rc != FLS_OK) return rc;
        m.g.cov_src.reserve(size_t(n) * 9);
        m.gicp_cov(m.src_own, m.src_grid, epsilon, m.g.cov_src.p);
        FLS_HIP(hipMemcpyAsync(cov, m.g.cov_src.p, size_t(n) * 9 * sizeof(double), hipMemcpyDeviceToHost, m.stream));
        FLS_HIP(hipStreamSynchronize(m.stream));
        return FLS_OK;
    });
}

fls_status fls_debug_loop_gicp_corr(int device_id, const float* moved, int ns, const float* tgt, int nt, int stride, const float* T, const double* R,
                                    const double* cov_src, const double* cov_tgt, double corr_dist, int host_grid, int32_t* corr, double* mahal) {
    if (!moved || !tgt || !T || !R || !cov_src || !cov_tgt || !corr || !mahal || ns < 0 || nt < 0 || stride < 3 || !(corr_dist > 0.0) || !std::isfinite(corr_dist) ||
        (host_grid != 0 && host_grid != 1))
        return FLS_ERR_INVALID;
    if (ns == 0) return FLS_OK;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (nt == 0) {
        for (int i = 0; i < ns; ++i) corr[i] = -1;
        std::fill(mahal, mahal + size_t(ns) * 9, nan);
        return FLS_OK;
    }
    return debug_loop_run(device_id, [&](LoopMatcher& m) -> fls_status {
        debug_loop_cloud(m, m.g.moved, moved, ns, stride);
        LoopMatcher::Filtered t = debug_loop_cloud(m, m.tgt_dev, tgt, nt, stride);
        const fls_status rc = m.cell_grid(m.g.tgt_grid, t, LoopMatcher::kGicpCell, true, host_grid != 0);
        if (rc != FLS_OK) return rc;
        m.g.cov_src.reserve(size_t(ns) * 9); m.g.cov_tgt.reserve(size_t(nt) * 9); m.g.mahal.reserve(size_t(ns) * 9); m.g.corr.reserve(size_t(ns));
        std::fill(mahal, mahal + size_t(ns) * 9, nan);
        FLS_HIP(hipMemcpyAsync(m.g.cov_src.p, cov_src, size_t(ns) * 9 * sizeof(double), hipMemcpyHostToDevice, m.stream));
        FLS_HIP(hipMemcpyAsync(m.g.cov_tgt.p, cov_tgt, size_t(nt) * 9 * sizeof(double), hipMemcpyHostToDevice, m.stream));
        FLS_HIP(hipMemcpyAsync(m.g.mahal.p, mahal, size_t(ns) * 9 * sizeof(double), hipMemcpyHostToDevice, m.stream));
        GicpRot rot;
        for (int i = 0; i < 9; ++i) rot.R[i] = R[i];
        m.gicp_corr(ns, debug_loop_mat(T), corr_dist * corr_dist, rot);
        FLS_HIP(hipMemcpyAsync(corr, m.g.corr.p, size_t(ns) * sizeof(int), hipMemcpyDeviceToHost, m.stream));
        FLS_HIP(hipMemcpyAsync(mahal, m.g.mahal.p, size_t(ns) * 9 * sizeof(double), hipMemcpyDeviceToHost, m.stream));
        FLS_HIP(hipStreamSynchronize(m.stream));
        return FLS_OK;
    });
}

fls_status fls_debug_loop_gicp_fdf(int device_id, const float* moved, int ns, const float* tgt, int nt, int stride, const double* x, const int32_t* corr,
                                   const double* mahal, int want_grad, double* v) {
    if (!moved || !tgt || !x || !corr || !mahal || !v || ns < 0 || nt < 0 || stride < 3) return FLS_ERR_INVALID;
    for (int i = 0; i < ns; ++i) if (corr[i] < -1 || corr[i] >= nt) return FLS_ERR_INVALID;  // (the kernel indexes the target with it)
    const int nv = want_grad ? 14 : 2;
    if (ns == 0) { for (int i = 0; i < nv; ++i) v[i] = 0.0; return FLS_OK; }
    return debug_loop_run(device_id, [&](LoopMatcher& m) -> fls_status {
        debug_loop_cloud(m, m.g.moved, moved, ns, stride);
        std::vector<Pt4> by_id(size_t(std::max(nt, 1)), Pt4{0.f, 0.f, 0.f, 0});
        for (int i = 0; i < nt; ++i) by_id[size_t(i)] = Pt4{tgt[size_t(i) * stride], tgt[size_t(i) * stride + 1], tgt[size_t(i) * stride + 2], i};
        m.g.tgt_grid.d_by_id.reserve(by_id.size());
        m.g.corr.reserve(size_t(ns)); m.g.mahal.reserve(size_t(ns) * 9);
        FLS_HIP(hipMemcpyAsync(m.g.tgt_grid.d_by_id.p, by_id.data(), by_id.size() * sizeof(Pt4), hipMemcpyHostToDevice, m.stream));
        FLS_HIP(hipMemcpyAsync(m.g.corr.p, corr, size_t(ns) * sizeof(int), hipMemcpyHostToDevice, m.stream));
        FLS_HIP(hipMemcpyAsync(m.g.mahal.p, mahal, size_t(ns) * 9 * sizeof(double), hipMemcpyHostToDevice, m.stream));
        FLS_HIP(hipStreamSynchronize(m.stream));  // (by_id is a local)
        m.g.n_src = size_t(ns); m.g.n_tgt = size_t(nt);
        double f, grad[6];
        m.gicp_fdf(m.g, x, &f, want_grad ? grad : nullptr);
        for (int i = 0; i < nv; ++i) v[i] = m.mail_host->v[i];
        return FLS_OK;
    });
}

fls_status fls_debug_loop_fitness(int device_id, const float* src, int ns, const float* tgt, int nt, int stride, const float* T, int host_grid,
                                  double* sum_d2, int64_t* count) {
    if (!src || !tgt || !T || !sum_d2 || !count || ns < 0 || nt < 0 || stride < 3 || (host_grid != 0 && host_grid != 1)) return FLS_ERR_INVALID;
    if (ns == 0 || nt == 0) { *sum_d2 = 0.0; *count = 0; return FLS_OK; }
    return debug_loop_run(device_id, [&](LoopMatcher& m) -> fls_status {
        debug_loop_cloud(m, m.src_own, src, ns, stride);
        LoopMatcher::Filtered t = debug_loop_cloud(m, m.tgt_dev, tgt, nt, stride);
        const fls_status rc = m.cell_grid(m.g.tgt_grid, t, LoopMatcher::kGicpCell, true, host_grid != 0);
        if (rc != FLS_OK) return rc;
        const double* v = m.fitness_sums(ns, debug_loop_mat(T));
        *sum_d2 = v[0];
        *count = int64_t(v[1]);
        FLS_HIP(hipStreamSynchronize(m.stream));
        return FLS_OK;
    });
}

}  // extern "C"
