// loop_device.hpp -- the loop-closure Match, written once (LoopMatcher::match), and its two entry points, which differ in where a filtered
// cloud comes from: run() from host clouds (the exact host filter one stage ahead on a side thread, or filter() under
// FLS_DEVICE_VOXELGRID=1), run_device() from clouds that lie on the matcher's device (include/fls_loop_device.h).  T, *fitness and every
// field of the stats are the same bits from both for the same points: the ten filters are the device VoxelGrid (bit-identical to the exact
// host filter) or that host filter itself, the leaf Gaussians come from kernels_loop_leaves.hpp or build_target, `moved` from
// loop_moved_kernel or the host loop over the same loop_xform, and everything else is the same code on the same buffers.
//
// What moves in run_device: nothing of an input cloud unless a filter declines (then that cloud is downloaded once per call, counter 5); of
// a filtered cloud, the target of a stage whose leaf build goes through the host, and a GICP cloud whose cell grid DeviceGridBuilder
// declines (counter 6, rows_of).  A filter's output is used where DeviceVoxelGrid left it (the target of an NDT stage) or after one
// device-to-device copy (the source, which the target's filter would overwrite; both GICP clouds).
#pragma once
#include "kernels_loop_leaves.hpp"

namespace fls {

// VoxelGridCloud(input w, leaf) for the Match, which asks in the order the stages consume the ten clouds.  `keep`: the cloud has to outlive
// the next get().  device_entry: leaf grids through build_target_device (when device_leaves), `moved` by loop_moved_kernel, dstat counted;
// otherwise build_target, the host loop and one upload, and dstat is left alone
struct LoopMatcher::CloudSource {
    const bool device_entry;
    explicit CloudSource(bool dev) : device_entry(dev) {}
    virtual void get(int w, float leaf, Filtered& out, bool keep) = 0;
};

// the leaf Gaussians of a filtered target: on the device when asked to, and on the host (build_target on the rows) when not or when the
// device build declines; `counted`: which of the two it was goes to dstat.  false: no leaf
inline bool LoopMatcher::target_leaves(Filtered& tgt, const float resolution, TargetLeaves& tl, const bool on_device, const bool counted) {
    if (on_device) {
        const DevCloud& d = planes(tgt);
        const LeafBuild rc = build_target_device(d.x(), d.y(), d.z(), d.n, resolution, tl);
        if (rc != kLeavesDeclined) { if (counted) ++dstat[kStatLeavesDevice]; return rc == kLeavesBuilt; }
    }
    if (counted) ++dstat[kStatLeavesHost];
    return build_target(rows_of(tgt), resolution, tl);
}

inline fls_status LoopMatcher::match(CloudSource& clouds, double* T, float* fitness) {
    std::memset(&st, 0, sizeof(st));
    *fitness = std::numeric_limits<float>::max();
    if (d_ticket.p) FLS_HIP(hipMemsetAsync(d_ticket.p, 0, kTicketWords * sizeof(unsigned), stream));  // (a Match that failed half-way must not poison the next)
    // FLS_HOST_TIMING=1: where the wall time of one Match goes (stderr)
    const bool timing = host_timing_enabled();
    double t_filter = 0, t_leaves = 0, t_ndt = 0, t_gicp_setup = 0, t_gicp = 0, t_fit = 0;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t0 = now();
    auto lap = [&](double& acc) { const double t = now(); acc += t - t0; t0 = t; };
    const bool on_device = clouds.device_entry;
    // ---- four NDT stages ----------------------------------------------------------------------------------------------------------
    static const float resolution[4] = {10.0f, 5.0f, 3.0f, 2.0f};
    Filtered src, tgt;
    for (int s = 0; s < 4; ++s) {
        const float r = resolution[s];
        src.dev = &src_dev; tgt.dev = &tgt_filtered;
        clouds.get(0, r * 0.2f, src, true);
        clouds.get(1, r * 0.2f, tgt, false);
        lap(t_filter);
        NdtRun run;
        run.resolution = r;
        const bool have = target_leaves(tgt, r, leaves, on_device && device_leaves, on_device);
        run.src = &planes(src);
        lap(t_leaves);
        run.tl = have ? &leaves : nullptr;
        int iters = 0;
        double score = 0.0;
        const auto eval = [&](const LoopMat4f& Tp, const double* p, bool hessian, double* grad, double* hess) { return ndt_eval(run, Tp, p, hessian, grad, hess); };
        const LoopMat4f fin = loop::ndt_align(run, eval, have && leaves.rows != 0, src_dev.n, loop::from_d(T), iters, score);
        for (int i = 0; i < 16; ++i) T[i] = double(fin.m[i]);
        st.ndt_iterations[s] = iters; st.ndt_evaluations[s] = run.evaluations; st.ndt_source_points[s] = int(src_dev.n);
        st.ndt_target_leaves[s] = have ? int(leaves.rows) : 0; st.ndt_score[s] = score;
        lap(t_ndt);
    }
    for (int i = 0; i < 16; ++i) st.T_after_ndt[i] = T[i];
    // ---- GICP -----------------------------------------------------------------------------------------------------------------------
    src.dev = &src_own; tgt.dev = &tgt_dev;
    clouds.get(0, 0.5f, src, true);
    clouds.get(1, 0.4f, tgt, true);
    lap(t_filter);
    const size_t n_src = src.size(), n_tgt = tgt.size();
    st.gicp_source_points = int(n_src);
    st.gicp_target_points = int(n_tgt);
    // computeCovariances refuses (k_correspondences_ > cloud size): no alignment
    if (n_src < 20 || n_tgt < 20) { FLS_HIP(hipStreamSynchronize(stream)); return FLS_OK; }
    g.n_src = n_src; g.n_tgt = n_tgt;
    g.evaluations = g.inner_total = g.n_corr = 0;
    const LoopMat4f guess = loop::from_d(T);
    // target grid (ids = cloud indices) + 20-NN covariances of both clouds, each in its own grid
    planes(tgt);
    planes(src);
    if (const fls_status rc = cell_grid(g.tgt_grid, tgt, kGicpCell, true)) return rc;
    if (const fls_status rc = cell_grid(src_grid, src, kGicpCell, false)) return rc;
    g.cov_src.reserve(n_src * 9); g.cov_tgt.reserve(n_tgt * 9); g.mahal.reserve(n_src * 9); g.corr.reserve(n_src);
    gicp_cov(tgt_dev, g.tgt_grid, 0.001, g.cov_tgt.p);
    gicp_cov(src_own, src_grid, 0.001, g.cov_src.p);
    // `output` = the source moved by the guess
    if (on_device) {
        g.moved.ext[0] = g.moved.ext[1] = g.moved.ext[2] = nullptr;
        g.moved.n = n_src;
        g.moved.xyz.reserve(3 * n_src);
        hipLaunchKernelGGL(loop_moved_kernel<kVgBlock>, dim3(unsigned((n_src + kVgBlock - 1) / kVgBlock)), dim3(kVgBlock), 0, stream, src_own.x(), src_own.y(), src_own.z(), int(n_src), guess,
                           g.moved.xyz.p, g.moved.xyz.p + n_src, g.moved.xyz.p + 2 * n_src);
        FLS_HIP(hipGetLastError());
    } else {
        std::vector<PtI> moved(n_src);
        for (size_t i = 0; i < n_src; ++i) { float o[3]; loop_xform(guess, src.rows[i].x, src.rows[i].y, src.rows[i].z, o); moved[i] = PtI{o[0], o[1], o[2], src.rows[i].i}; }
        g.moved.upload(moved, stream);
    }
    if (timing) FLS_HIP(hipStreamSynchronize(stream));
    lap(t_gicp_setup);
    const LoopMat4f fin = gicp_outer(int(n_src), guess, T);
    lap(t_gicp);
    fitness_score(int(n_src), fin, fitness);
    lap(t_fit);
    if (timing) print_timing(t_filter, t_leaves, t_ndt, t_gicp_setup, t_gicp, t_fit);
    return FLS_OK;
}

inline fls_status LoopMatcher::run(const std::vector<PtI>& source, const std::vector<PtI>& target, double* T, float* fitness) {
    read_env();
    FLS_HIP(hipSetDevice(device));
    // The ten VoxelGridCloud calls depend on the inputs only: with the exact host filter they run on a side thread (which borrows the
    // worker pool), one stage ahead of the optimiser that spins on the device's result block on this thread.
    struct HostSource : CloudSource {
        LoopMatcher& m;
        const std::vector<PtI>* const input[2];
        FilterAhead ahead;
        int next = 0;
        HostSource(LoopMatcher& m_, const std::vector<PtI>& s, const std::vector<PtI>& t) : CloudSource(false), m(m_), input{&s, &t} {
            if (!m.device_filter) ahead.start(s, t);
        }
        void get(int w, float leaf, Filtered& out, bool) override { out.set_rows(m.device_filter ? m.filter(*input[w], leaf) : ahead.take(next++)); }
    } clouds(*this, source, target);
    return match(clouds, T, fitness);
}

inline fls_status LoopMatcher::run_device(const DevInput& source, const DevInput& target, double* T, float* fitness) {
    read_env();
    FLS_HIP(hipSetDevice(device));
    ++dstat[kStatMatches];
    struct DeviceSource : CloudSource {
        LoopMatcher& m;
        const DevInput* const input[2];
        const bool filter_on_device = device_voxelgrid_mode() != 0;
        std::vector<PtI> host_in[2];  // the host copy of an input: made when a filter declines, once per call and cloud
        bool have_host[2] = {false, false};
        DeviceSource(LoopMatcher& m_, const DevInput& s, const DevInput& t) : CloudSource(true), m(m_), input{&s, &t} {
            // a cloud without an intensity plane reads zeros (written once, when the plane grows)
            size_t need = 0;
            for (int w = 0; w < 2; ++w) if (!input[w]->in) need = std::max(need, input[w]->n);
            if (need) m.d_zero.reserve(need, false, m.stream, /*zero_new=*/true);
        }
        const std::vector<PtI>& host_input(const int w) {
            const DevInput& c = *input[w];
            if (!have_host[w]) m.dstat[kStatInputBytes] += m.download_rows(c.x, c.y, c.z, c.in, c.n, host_in[w]);
            have_host[w] = true;
            return host_in[w];
        }
        void get(int w, float leaf, Filtered& out, bool keep) override {
            const DevInput& c = *input[w];
            DeviceVoxelGrid& vg = m.vg;
            if (filter_on_device && vg.run(c.x, c.y, c.z, c.in ? c.in : m.d_zero.p, c.n, leaf, m.stream)) {
                ++m.dstat[kStatFiltersDevice];
                if (keep) out.dev->copy_from(vg.ox(), vg.oy(), vg.oz(), vg.n_out, m.stream);
                else out.dev->attach(vg.ox(), vg.oy(), vg.oz(), vg.n_out);  // used where the filter left it
                out.on_dev = true; out.on_host = false;
                return;
            }
            ++m.dstat[kStatFiltersHost];
            out.set_rows(voxel_grid(host_input(w), leaf));
            m.planes(out);
        }
    } clouds(*this, source, target);
    return match(clouds, T, fitness);
}

}  // namespace fls
