// loop_device.hpp -- LoopMatcher::run_device: LoopMatcher::run (loop_closure.hpp) from clouds that lie on the matcher's device
// (include/fls_loop_device.h).  T, *fitness and every field of the stats equal run()'s for the same points, bit for bit: the ten filters
// are the device VoxelGrid (bit-identical to the exact host filter) or that host filter itself, the leaf Gaussians come from
// kernels_loop_leaves.hpp or build_target, and everything from ndt_align on is run()'s own code on the same buffers.
//
// What moves: nothing of an input cloud unless a filter declines (then that cloud is downloaded once per call, counter 5); of a filtered
// cloud, the target of a stage whose leaf build goes through the host, and a GICP cloud whose cell grid DeviceGridBuilder declines
// (counter 6).  A filter's output is used where DeviceVoxelGrid left it (the target of an NDT stage) or after one device-to-device copy
// (the source, which the target's filter would overwrite; both GICP clouds).  `moved` is made by loop_moved_kernel: 0 bytes.
#pragma once
#include "kernels_loop_leaves.hpp"

namespace fls {

inline fls_status LoopMatcher::run_device(const DevInput& source, const DevInput& target, double* T, float* fitness) {
    std::memset(&st, 0, sizeof(st));
    *fitness = std::numeric_limits<float>::max();
    read_env();
    FLS_HIP(hipSetDevice(device));
    if (d_ticket.p) FLS_HIP(hipMemsetAsync(d_ticket.p, 0, kTicketWords * sizeof(unsigned), stream));
    ++dstat[kStatMatches];
    const bool filter_on_device = device_voxelgrid_mode() != 0;
    const bool timing = host_timing_enabled();
    double t_filter = 0, t_leaves = 0, t_ndt = 0, t_gicp_setup = 0, t_gicp = 0, t_fit = 0;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t0 = now();
    auto lap = [&](double& acc) { const double t = now(); acc += t - t0; t0 = t; };

    const DevInput* const input[2] = {&source, &target};
    {   // a cloud without an intensity plane reads zeros (written once, when the plane grows)
        size_t need = 0;
        for (int w = 0; w < 2; ++w) if (!input[w]->in) need = std::max(need, input[w]->n);
        if (need) d_zero.reserve(need, false, stream, /*zero_new=*/true);
    }
    // the host copy of an input: made when a filter declines, once per call and cloud
    std::vector<PtI> host_in[2];
    bool have_host[2] = {false, false};
    std::vector<float> tmp;
    auto host_input = [&](const int w) -> const std::vector<PtI>& {
        if (have_host[w]) return host_in[w];
        const DevInput& c = *input[w];
        const size_t n = c.n;
        const int planes = c.in ? 4 : 3;
        host_in[w].resize(n);
        if (n) {
            tmp.resize(size_t(planes) * n);
            const float* const src[4] = {c.x, c.y, c.z, c.in};
            for (int a = 0; a < planes; ++a) FLS_HIP(hipMemcpyAsync(tmp.data() + size_t(a) * n, src[a], n * sizeof(float), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            for (size_t i = 0; i < n; ++i) host_in[w][i] = PtI{tmp[i], tmp[n + i], tmp[2 * n + i], planes == 4 ? tmp[3 * n + i] : 0.f};
            dstat[kStatInputBytes] += size_t(planes) * n * sizeof(float);
        }
        have_host[w] = true;
        return host_in[w];
    };
    // VoxelGridCloud(input w, leaf): true = on the device, the result in vg.out (n = vg.n_out); false = declined, the result in `rows`
    auto filter_dev = [&](const int w, const float leaf, std::vector<PtI>& rows) {
        const DevInput& c = *input[w];
        if (filter_on_device && vg.run(c.x, c.y, c.z, c.in ? c.in : d_zero.p, c.n, leaf, stream)) { ++dstat[kStatFiltersDevice]; return true; }
        ++dstat[kStatFiltersHost];
        rows = voxel_grid(host_input(w), leaf);
        return false;
    };
    // a filtered cloud's rows on the host (x, y, z; nothing downstream reads the intensity)
    auto download_filtered = [&](const DevCloud& c) {
        std::vector<PtI> rows(c.n);
        if (!c.n) return rows;
        tmp.resize(3 * c.n);
        FLS_HIP(hipMemcpyAsync(tmp.data(), c.x(), c.n * sizeof(float), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipMemcpyAsync(tmp.data() + c.n, c.y(), c.n * sizeof(float), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipMemcpyAsync(tmp.data() + 2 * c.n, c.z(), c.n * sizeof(float), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        for (size_t i = 0; i < c.n; ++i) rows[i] = PtI{tmp[i], tmp[c.n + i], tmp[2 * c.n + i], 0.f};
        dstat[kStatFilteredBytes] += 3 * c.n * sizeof(float);
        return rows;
    };
    // filter input w into `own`: a copy of the device filter's output, or the uploaded host result.  true: `rows` holds it too
    auto filter_into = [&](const int w, const float leaf, DevCloud& own, std::vector<PtI>& rows) {
        if (filter_dev(w, leaf, rows)) { own.copy_from(vg.ox(), vg.oy(), vg.oz(), vg.n_out, stream); return false; }
        own.upload(rows, stream);
        return true;
    };

    // ---- four NDT stages ----------------------------------------------------------------------------------------------------------
    static const float resolution[4] = {10.0f, 5.0f, 3.0f, 2.0f};
    std::vector<PtI> src_rows, tgt_rows;
    for (int s = 0; s < 4; ++s) {
        const float r = resolution[s];
        filter_into(0, r * 0.2f, src_dev, src_rows);
        bool tgt_on_host = false;
        if (filter_dev(1, r * 0.2f, tgt_rows)) tgt_filtered.attach(vg.ox(), vg.oy(), vg.oz(), vg.n_out);  // used where the filter left it
        else { tgt_filtered.upload(tgt_rows, stream); tgt_on_host = true; }
        lap(t_filter);
        NdtRun run;
        run.resolution = r;
        bool have = false, built = false;
        if (device_leaves) {
            const LeafBuild rc = build_target_device(tgt_filtered.x(), tgt_filtered.y(), tgt_filtered.z(), tgt_filtered.n, r, leaves);
            if (rc != kLeavesDeclined) { ++dstat[kStatLeavesDevice]; have = rc == kLeavesBuilt; built = true; }
        }
        if (!built) {
            ++dstat[kStatLeavesHost];
            if (!tgt_on_host) tgt_rows = download_filtered(tgt_filtered);
            have = build_target(tgt_rows, r, leaves);
        }
        lap(t_leaves);
        run.src = &src_dev;
        run.tl = have ? &leaves : nullptr;
        int iters = 0;
        double score = 0.0;
        const LoopMat4f fin = ndt_align(run, from_d(T), iters, score);
        for (int i = 0; i < 16; ++i) T[i] = double(fin.m[i]);
        st.ndt_iterations[s] = iters; st.ndt_evaluations[s] = run.evaluations; st.ndt_source_points[s] = int(src_dev.n);
        st.ndt_target_leaves[s] = have ? int(leaves.rows) : 0; st.ndt_score[s] = score;
        lap(t_ndt);
    }
    for (int i = 0; i < 16; ++i) st.T_after_ndt[i] = T[i];
    // ---- GICP -----------------------------------------------------------------------------------------------------------------------
    const bool src_on_host = filter_into(0, 0.5f, src_own, src_rows);
    const bool tgt_on_host = filter_into(1, 0.4f, tgt_dev, tgt_rows);
    lap(t_filter);
    const size_t n_src = src_own.n, n_tgt = tgt_dev.n;
    st.gicp_source_points = int(n_src);
    st.gicp_target_points = int(n_tgt);
    if (n_src < 20 || n_tgt < 20) { FLS_HIP(hipStreamSynchronize(stream)); return FLS_OK; }
    g.n_src = n_src; g.n_tgt = n_tgt;
    g.evaluations = g.inner_total = g.n_corr = 0;
    const LoopMat4f guess = from_d(T);
    const float cell = 1.5f;
    if (!builder.run(g.tgt_grid, tgt_dev.x(), tgt_dev.y(), tgt_dev.z(), n_tgt, cell, 1, true, stream)) {
        if (!tgt_on_host) tgt_rows = download_filtered(tgt_dev);
        const fls_status rc = g.tgt_grid.build(tgt_rows, cell, stream, 1, true);
        if (rc != FLS_OK) return rc;
    }
    if (!builder.run(src_grid, src_own.x(), src_own.y(), src_own.z(), n_src, cell, 1, false, stream)) {
        if (!src_on_host) src_rows = download_filtered(src_own);
        const fls_status rc = src_grid.build(src_rows, cell, stream, 1, false);
        if (rc != FLS_OK) return rc;
    }
    g.cov_src.reserve(n_src * 9); g.cov_tgt.reserve(n_tgt * 9); g.mahal.reserve(n_src * 9); g.corr.reserve(n_src);
    hipLaunchKernelGGL(gicp_cov_kernel, dim3(unsigned((n_tgt + kCovWaves - 1) / kCovWaves)), dim3(64 * kCovWaves), 0, stream, tgt_dev.x(), tgt_dev.y(), tgt_dev.z(), int(n_tgt),
                       cell_dev(g.tgt_grid), 0.001, g.cov_tgt.p);
    hipLaunchKernelGGL(gicp_cov_kernel, dim3(unsigned((n_src + kCovWaves - 1) / kCovWaves)), dim3(64 * kCovWaves), 0, stream, src_own.x(), src_own.y(), src_own.z(), int(n_src),
                       cell_dev(src_grid), 0.001, g.cov_src.p);
    FLS_HIP(hipGetLastError());
    // `output` = the source moved by the guess
    g.moved.ext[0] = g.moved.ext[1] = g.moved.ext[2] = nullptr;
    g.moved.n = n_src;
    g.moved.xyz.reserve(3 * n_src);
    hipLaunchKernelGGL(loop_moved_kernel<kVgBlock>, dim3(unsigned((n_src + kVgBlock - 1) / kVgBlock)), dim3(kVgBlock), 0, stream, src_own.x(), src_own.y(), src_own.z(), int(n_src), guess,
                       g.moved.xyz.p, g.moved.xyz.p + n_src, g.moved.xyz.p + 2 * n_src);
    FLS_HIP(hipGetLastError());
    if (timing) FLS_HIP(hipStreamSynchronize(stream));
    lap(t_gicp_setup);
    const LoopMat4f fin = gicp_outer(int(n_src), guess, T);
    lap(t_gicp);
    fitness_score(int(n_src), fin, fitness);
    lap(t_fit);
    if (timing) print_timing(t_filter, t_leaves, t_ndt, t_gicp_setup, t_gicp, t_fit);
    return FLS_OK;
}

}  // namespace fls
