// loop_closure.hpp -- host side of fls_loop_match, the replacement of LoopClosure::Match (src/slam/loop_closure.cpp:233-267):
//
//     static const std::vector<float> resolution{10.0, 5.0, 3.0, 2.0};
//     pcl::NormalDistributionsTransform ndt;  setStepSize(0.5)  setMaximumIterations(30)           :239-242
//     for r: setResolution(r); source / target = VoxelGridCloud(.., r * 0.2f); align(pose)          :244-252
//     pcl::GeneralizedIterativeClosestPoint gicp over VoxelGridCloud(source, 0.5f) / (target, 0.4f),
//         setMaximumIterations(30) setMaxCorrespondenceDistance(2.0); align(pose)                    :254-263
//     return gicp.getFitnessScore()                                                                  :265
//
// PCL is a third-party dependency that is not under /root/reference; what is implemented is the published algorithm each PCL 1.10
// class implements, with the parameters the reference sets and PCL's defaults for the rest:
//   NormalDistributionsTransform (ndt.hpp)       Magnusson 2009 P2D-NDT: leaf Gaussians of VoxelGridCovariance (>= 6 points, eigenvalue
//                                                floor 0.01), outlier ratio 0.55, Newton step from a 6x6 SVD solve, More-Thuente line
//                                                search (mu 1e-4, nu 0.9, <= 10 trials, step in [epsilon / 2, step size]), stop when the
//                                                step length drops below transformation epsilon 0.1
//   GeneralizedIterativeClosestPoint (gicp.hpp)  Segal 2009: 20-NN covariances with singular values (1, 1, 1e-3), nearest-neighbour
//                                                correspondences inside the gate, BFGS (GSL vector_bfgs2, <= 20 inner iterations,
//                                                gradient tolerance 1e-2) on sum res^T (C2 + R C1 R^T)^-1 res, stop on rotation 2e-3 /
//                                                translation 5e-4 change
// Division of labour: everything per POINT runs on the device (kernels_loop.hpp: score / gradient / Hessian sums, 20-NN covariances,
// correspondences + Mahalanobis matrices, cost + gradient sums, fitness); the six-parameter optimisers and the leaf statistics of
// the (already down-sampled) target run on the host, which learns every reduction result through a host-mapped block (no stream
// synchronisation per evaluation).  The VoxelGridCloud calls use the exact host filter by default, the device filter with
// FLS_DEVICE_VOXELGRID=1.
// Layout: loop_optim.hpp    the optimisers and the pose algebra, which know neither this struct nor the device;
//         this file         LoopMatcher: buffers, reduce(), build_target, the device sums the optimisers are given (ndt_eval, gicp_fdf) and one
//                           function per stage (cell_grid, gicp_cov, gicp_corr, fitness_sums), which the Match and the test hooks both call;
//         loop_device.hpp   (behind the leaf-build kernels of kernels_loop_leaves.hpp) the one Match sequence and its two cloud sources.
#pragma once
#include <chrono>
#include "device_voxelgrid.hpp"
#include "kernels_loop.hpp"
#include "fitness_host.hpp"
#include "loop_optim.hpp"
#include <map>
#include <thread>
#include <mutex>
#include <exception>
#include <condition_variable>

namespace fls {

struct LoopMatcher {
    std::mutex run_mx;  // held by fls_loop_match for the duration of a Match
    int device = 0;
    hipStream_t stream = nullptr;
    LoopMail* mail_host = nullptr;
    LoopMail* mail_dev = nullptr;
    unsigned seq = 0;
    DevBuf<double> d_rows;
    DevBuf<unsigned> d_ticket;
    bool device_filter = false;
    bool debug = false;  // FLS_LOOP_DEBUG=1: one line per GICP outer iteration on stderr
    fls_loop_stats st{};

    ~LoopMatcher() {
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        if (mail_host) (void)hipHostFree(mail_host);
    }
    void init(int dev) {
        device = dev;
        FLS_HIP(hipSetDevice(device));
        FLS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        FLS_HIP(hipHostMalloc((void**)&mail_host, sizeof(LoopMail), hipHostMallocMapped));
        std::memset(mail_host, 0, sizeof(LoopMail));
        FLS_HIP(hipHostGetDevicePointer((void**)&mail_dev, mail_host, 0));
        if (const char* e = std::getenv("FLS_LOOP_DEVICE_LEAVES")) device_leaves = std::atoi(e) != 0;
        read_env();
    }
    void read_env() {  // per Match: one matcher per device is kept alive across calls (fls_reg.hip)
        device_filter = false; debug = false;
        if (const char* e = std::getenv("FLS_DEVICE_VOXELGRID")) device_filter = std::atoi(e) != 0;
        if (const char* e = std::getenv("FLS_LOOP_DEBUG")) debug = std::atoi(e) != 0;
    }

    // ---- reductions: launch `fill` (writes nrows partial rows, its last workgroup sums them), wait for the host-mapped block ---------
    template <class F>
    const double* reduce(int nrows, F&& fill) {
        d_rows.reserve(size_t(std::max(nrows, 1)) * kLoopMaxV);
        if (!d_ticket.p) {
            d_ticket.reserve(kTicketWords);
            FLS_HIP(hipMemsetAsync(d_ticket.p, 0, kTicketWords * sizeof(unsigned), stream));
        }
        seq = (seq + 1u) & 0x7fffffffu;
        if (seq == 0u) seq = 1u;
        fill(LoopOut{d_rows.p, d_ticket.p, mail_dev, seq});
        FLS_HIP(hipGetLastError());
        const auto published = [&] { return __atomic_load_n(&mail_host->seq, __ATOMIC_ACQUIRE) == seq; };
        // (the stream went idle: the block must be there -- anything else is a lost fan-in, never a result to use)
        if (!spin_until(stream, published) && !published()) throw HipError(hipErrorUnknown, "fls_loop_match: the device left no result block for an evaluation");
        return mail_host->v;
    }

    // a cloud as x | y | z planes on the device
    struct DevCloud {
        DevBuf<float> xyz;
        PinnedBuf<float> stage;
        size_t n = 0;
        const float* ext[3] = {nullptr, nullptr, nullptr};  // attach(): planes that lie elsewhere on the device (a filter's output), not owned
        const float* x() const { return ext[0] ? ext[0] : xyz.p; }
        const float* y() const { return ext[0] ? ext[1] : xyz.p + n; }
        const float* z() const { return ext[0] ? ext[2] : xyz.p + 2 * n; }
        void attach(const float* px, const float* py, const float* pz, size_t count) { ext[0] = px; ext[1] = py; ext[2] = pz; n = count; }
        // the same planes copied into this cloud's own buffer, device to device on `s` (no wait)
        void copy_from(const float* px, const float* py, const float* pz, size_t count, hipStream_t s) {
            ext[0] = ext[1] = ext[2] = nullptr;
            n = count;
            if (!n) return;
            xyz.reserve(3 * n);
            FLS_HIP(hipMemcpyAsync(xyz.p, px, n * sizeof(float), hipMemcpyDeviceToDevice, s));
            FLS_HIP(hipMemcpyAsync(xyz.p + n, py, n * sizeof(float), hipMemcpyDeviceToDevice, s));
            FLS_HIP(hipMemcpyAsync(xyz.p + 2 * n, pz, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        void upload(const std::vector<PtI>& c, hipStream_t s) {
            ext[0] = ext[1] = ext[2] = nullptr;
            n = c.size();
            if (!n) return;
            stage.reserve(3 * n);
            xyz.reserve(3 * n);
            for (size_t i = 0; i < n; ++i) { stage.p[i] = c[i].x; stage.p[n + i] = c[i].y; stage.p[2 * n + i] = c[i].z; }
            FLS_HIP(hipMemcpyAsync(xyz.p, stage.p, 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
            FLS_HIP(hipStreamSynchronize(s));
        }
    };

    // a filtered cloud of a Match: its planes on the device, its rows on the host, or both.  planes() / rows_of() make the missing side
    struct Filtered {
        DevCloud* dev = nullptr;
        std::vector<PtI> rows;
        bool on_dev = false, on_host = false;
        size_t size() const { return on_dev ? dev->n : rows.size(); }
        void set_rows(std::vector<PtI>&& r) { rows = std::move(r); on_host = true; on_dev = false; }
    };
    const DevCloud& planes(Filtered& c) {
        if (!c.on_dev) { c.dev->upload(c.rows, stream); c.on_dev = true; }
        return *c.dev;
    }
    // n points of device planes (in == nullptr: intensity 0) as rows on the host; returns the bytes that crossed the bus
    size_t download_rows(const float* x, const float* y, const float* z, const float* in, const size_t n, std::vector<PtI>& rows) {
        const float* const src[4] = {x, y, z, in};
        const size_t planes = in ? 4 : 3;
        rows.resize(n);
        if (!n) return 0;
        std::vector<float> tmp(planes * n);
        for (size_t a = 0; a < planes; ++a) FLS_HIP(hipMemcpyAsync(tmp.data() + a * n, src[a], n * sizeof(float), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        for (size_t i = 0; i < n; ++i) rows[i] = PtI{tmp[i], tmp[n + i], tmp[2 * n + i], in ? tmp[3 * n + i] : 0.f};
        return planes * n * sizeof(float);
    }
    // the rows a host fallback needs (x, y, z; nothing downstream reads the intensity): nothing to do when they are on the host already
    const std::vector<PtI>& rows_of(Filtered& c) {
        if (!c.on_host) dstat[kStatFilteredBytes] += download_rows(c.dev->x(), c.dev->y(), c.dev->z(), nullptr, c.dev->n, c.rows);
        c.on_host = true;
        return c.rows;
    }

    DevScan raw;  // (device filter's staging + kernels' scratch: kept across calls)
    DeviceVoxelGrid vg;
    std::vector<PtI> filter(const std::vector<PtI>& c, float leaf) {  // VoxelGridCloud (pointcloud_utility.h:216-271)
        if (device_filter && !c.empty()) {
            raw.upload_raw(&c[0].x, c.size(), 4, stream, true);
            if (vg.run(raw.x.p, raw.y.p, raw.z.p, raw.xyz.p + 3 * c.size(), c.size(), leaf, stream)) {
                std::vector<float> tmp;
                return vg.download(stream, tmp);
            }
        }
        return voxel_grid(c, leaf);
    }

    // ======================================================================================================================
    // NormalDistributionsTransform
    // ======================================================================================================================
    struct TargetLeaves {  // VoxelGridCovariance(leaf = resolution, min_points_per_voxel 6, min_covar_eigvalue_mult 0.01), searchable
        int min_b[3] = {0, 0, 0}, div_b[3] = {0, 0, 0};
        float inv = 1.f;
        std::vector<int> leaf_row;
        std::vector<double> mean, icov;
        std::vector<float> centroid;
        std::vector<int> row_cell, row_n;  // per row: the leaf's cell index and number of points (fls_debug_loop_leaves)
        bool rows_on_host = false;         // mean .. row_n hold this build (build_target; a device build after download_leaves)
        size_t rows = 0;
        DevBuf<int> d_leaf_row;
        DevBuf<int> d_row_cell, d_row_n;   // the same, written by the device build
        DevBuf<double> d_mean, d_icov;
        DevBuf<float> d_centroid;
        // sparse form (grid volume above kMaxDenseLeafCells: a stray far point must not cost gigabytes): cell -> row through an
        // open-addressing table of {cell, row} pairs instead of the dense [div2][div1][div0] table
        std::vector<int2> leaf_hash;
        DevBuf<int2> d_leaf_hash;
        unsigned hash_mask = 0;
        bool sparse = false;
    };
    static constexpr size_t kMaxDenseLeafCells = size_t(32) << 20;  // 32 Mi cells: 128 MiB per dense int table (host x 2, device x 1)
    static unsigned leaf_hash_of(const int cell) { return unsigned(cell) * 2654435761u; }
    // release host / device tables an outlier call inflated (the matcher is cached for the life of the process)
    template <class V> static void shrink_if_oversized(V& v, const size_t need) {
        if (v.capacity() > (size_t(4) << 20) && v.capacity() > 4 * need) { V().swap(v); }
    }
    template <class T> static void shrink_if_oversized(DevBuf<T>& b, const size_t need) {
        if (b.cap > (size_t(4) << 20) && b.cap > 4 * need) { (void)hipDeviceSynchronize(); (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    }
    struct LeafAcc { int n = 0; double sum[3] = {0, 0, 0}, xx[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; float csum[3] = {0, 0, 0}; };
    std::vector<int> acc_of;
    std::vector<LeafAcc> accs;

    bool build_target(const std::vector<PtI>& in, float resolution, TargetLeaves& tl) {
        tl.rows = 0;
        tl.rows_on_host = true;
        tl.inv = 1.0f / resolution;
        const float inv = tl.inv;
        float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        bool any = false;
        for (const PtI& p : in) {
            if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z)) continue;
            any = true;
            mn[0] = std::min(mn[0], p.x); mx[0] = std::max(mx[0], p.x);
            mn[1] = std::min(mn[1], p.y); mx[1] = std::max(mx[1], p.y);
            mn[2] = std::min(mn[2], p.z); mx[2] = std::max(mx[2], p.z);
        }
        if (!any) return false;
        const long long dx = (long long)((mx[0] - mn[0]) * inv) + 1, dy = (long long)((mx[1] - mn[1]) * inv) + 1, dz = (long long)((mx[2] - mn[2]) * inv) + 1;
        if (dx * dy * dz > (long long)INT_MAX) return false;
        for (int a = 0; a < 3; ++a) { tl.min_b[a] = int(std::floor(mn[a] * inv)); tl.div_b[a] = int(std::floor(mx[a] * inv)) - tl.min_b[a] + 1; }
        const int m1 = tl.div_b[0], m2 = tl.div_b[0] * tl.div_b[1];
        // PCL keeps the leaves in a std::map (ascending leaf index) and adds a leaf's points in cloud order; the same sums and the same
        // emission order come from a dense cell -> accumulator table (the grid volume is bounded above) walked in ascending cell index.
        // (A std::map here cost ~100 ns per point: 4-5 ms per Match.)
        const size_t n_cells = size_t(tl.div_b[0]) * tl.div_b[1] * tl.div_b[2];
        tl.sparse = n_cells > kMaxDenseLeafCells;
        accs.clear();
        auto accumulate = [](LeafAcc& l, const PtI& p) {
            const double q[3] = {double(p.x), double(p.y), double(p.z)};
            for (int a = 0; a < 3; ++a) l.sum[a] += q[a];
            for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) l.xx[r + 3 * c] += q[r] * q[c];
            l.csum[0] += p.x; l.csum[1] += p.y; l.csum[2] += p.z;
            ++l.n;
        };
        auto cell_of = [&](const PtI& p) {
            const int i0 = int(std::floor(p.x * inv) - float(tl.min_b[0])), i1 = int(std::floor(p.y * inv) - float(tl.min_b[1])), i2 = int(std::floor(p.z * inv) - float(tl.min_b[2]));
            return i0 + i1 * m1 + i2 * m2;  // < INT_MAX (checked above)
        };
        // occupied cells in ascending cell index with their accumulators: `order` = {cell, accumulator}
        std::vector<std::pair<int, int>> order;
        if (!tl.sparse) {
            shrink_if_oversized(acc_of, n_cells);
            acc_of.assign(n_cells, -1);
            for (const PtI& p : in) {
                if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z)) continue;
                int& slot = acc_of[size_t(cell_of(p))];
                if (slot < 0) { slot = int(accs.size()); accs.emplace_back(); }
                accumulate(accs[size_t(slot)], p);
            }
            order.reserve(accs.size());
            for (size_t cell_i = 0; cell_i < n_cells; ++cell_i)
                if (acc_of[cell_i] >= 0) order.emplace_back(int(cell_i), acc_of[cell_i]);
        } else {
            // sparse: O(points) memory whatever the extent.  (cell, point) pairs sorted: ascending cell, a cell's points in cloud order --
            // the same sums in the same order as the dense table gives
            std::vector<std::pair<int, unsigned>> cp;
            cp.reserve(in.size());
            for (size_t k = 0; k < in.size(); ++k) {
                const PtI& p = in[k];
                if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z)) continue;
                cp.emplace_back(cell_of(p), unsigned(k));
            }
            std::sort(cp.begin(), cp.end());
            for (size_t a = 0; a < cp.size();) {
                size_t b = a;
                accs.emplace_back();
                for (; b < cp.size() && cp[b].first == cp[a].first; ++b) accumulate(accs.back(), in[cp[b].second]);
                order.emplace_back(cp[a].first, int(accs.size()) - 1);
                a = b;
            }
            std::vector<int>().swap(acc_of);
        }
        if (!tl.sparse) { shrink_if_oversized(tl.leaf_row, n_cells); tl.leaf_row.assign(n_cells, -1); }
        else {
            std::vector<int>().swap(tl.leaf_row);
            size_t hs = 1024;
            while (hs < 2 * order.size() + 2) hs <<= 1;
            tl.hash_mask = unsigned(hs - 1);
            tl.leaf_hash.assign(hs, make_int2(-1, -1));
        }
        tl.mean.clear(); tl.icov.clear(); tl.centroid.clear(); tl.row_cell.clear(); tl.row_n.clear();
        for (const std::pair<int, int>& oc : order) {
            const size_t cell_i = size_t(oc.first);
            const LeafAcc& l = accs[size_t(oc.second)];
            const int n = l.n;
            if (n < 6) continue;
            double mean[3], icov[9];
            loop::leaf_gaussian(n, l.sum, l.xx, mean, icov);
            if (!tl.sparse) tl.leaf_row[cell_i] = int(tl.rows);
            else {
                unsigned h = leaf_hash_of(int(cell_i)) & tl.hash_mask;
                while (tl.leaf_hash[h].x >= 0) h = (h + 1) & tl.hash_mask;
                tl.leaf_hash[h] = make_int2(int(cell_i), int(tl.rows));
            }
            for (int a = 0; a < 3; ++a) { tl.mean.push_back(mean[a]); tl.centroid.push_back(l.csum[a] / float(n)); }
            for (int a = 0; a < 9; ++a) tl.icov.push_back(icov[a]);
            tl.row_cell.push_back(int(cell_i)); tl.row_n.push_back(n);
            ++tl.rows;
        }
        if (tl.rows == 0) return false;
        shrink_if_oversized(tl.d_leaf_row, tl.leaf_row.size());
        tl.d_mean.reserve(tl.mean.size()); tl.d_icov.reserve(tl.icov.size()); tl.d_centroid.reserve(tl.centroid.size());
        if (!tl.sparse) {
            tl.d_leaf_row.reserve(tl.leaf_row.size());
            FLS_HIP(hipMemcpyAsync(tl.d_leaf_row.p, tl.leaf_row.data(), tl.leaf_row.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        } else {
            tl.d_leaf_hash.reserve(tl.leaf_hash.size());
            FLS_HIP(hipMemcpyAsync(tl.d_leaf_hash.p, tl.leaf_hash.data(), tl.leaf_hash.size() * sizeof(int2), hipMemcpyHostToDevice, stream));
        }
        FLS_HIP(hipMemcpyAsync(tl.d_mean.p, tl.mean.data(), tl.mean.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        FLS_HIP(hipMemcpyAsync(tl.d_icov.p, tl.icov.data(), tl.icov.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        FLS_HIP(hipMemcpyAsync(tl.d_centroid.p, tl.centroid.data(), tl.centroid.size() * sizeof(float), hipMemcpyHostToDevice, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        return true;
    }

    struct NdtRun : loop::NdtRun {
        const DevCloud* src = nullptr;
        const TargetLeaves* tl = nullptr;
        int evaluations = 0;
    };
    // computeDerivatives / computeHessian on the device: score, gradient (6), Hessian (36, column-major)
    double ndt_eval(NdtRun& r, const LoopMat4f& T, const double* p, bool hessian, double* grad, double* hess) {
        loop::angle_derivatives(p, r.pose);
        r.pose.T = T;
        const TargetLeaves& tl = *r.tl;
        NdtP2dTarget tg{tl.sparse ? nullptr : tl.d_leaf_row.p, tl.d_mean.p, tl.d_icov.p, tl.d_centroid.p, {tl.min_b[0], tl.min_b[1], tl.min_b[2]}, {tl.div_b[0], tl.div_b[1], tl.div_b[2]},
                        tl.inv, r.resolution * r.resolution, tl.sparse ? tl.d_leaf_hash.p : nullptr, tl.hash_mask};
        const int n = int(r.src->n), nb = (n + kLoopBlock - 1) / kLoopBlock;
        ++r.evaluations;
        const double* v = reduce(nb, [&](const LoopOut rows) {
            if (hessian) hipLaunchKernelGGL(ndt_p2d_kernel<true>, dim3(unsigned(nb)), dim3(kLoopBlock), 0, stream, r.src->x(), r.src->y(), r.src->z(), n, tg, r.pose, rows);
            else hipLaunchKernelGGL(ndt_p2d_kernel<false>, dim3(unsigned(nb)), dim3(kLoopBlock), 0, stream, r.src->x(), r.src->y(), r.src->z(), n, tg, r.pose, rows);
        });
        if (grad) for (int i = 0; i < 6; ++i) grad[i] = v[1 + i];
        if (hessian && hess) for (int i = 0; i < 36; ++i) hess[i] = v[7 + i];
        return v[0];
    }

    // ======================================================================================================================
    // GeneralizedIterativeClosestPoint
    // ======================================================================================================================
    struct GicpRun {
        DevCloud moved;           // `output`: the source transformed by the guess (float)
        CellGridImage tgt_grid;   // target cloud, ids = cloud indices, by_id copy for the cost kernel
        DevBuf<double> cov_src, cov_tgt, mahal;
        DevBuf<int> corr;
        size_t n_src = 0, n_tgt = 0;
        int evaluations = 0, inner_total = 0, n_corr = 0;
    };
    // OptimizationFunctorWithIndices: f (and g) at x, sums on the device
    void gicp_fdf(GicpRun& g, const double* x, double* f, double* grad) {
        ++g.evaluations;
        LoopMat4f T = loop::ident();
        loop::apply_state(T, x);
        const int n = int(g.n_src), nb = (n + kLoopBlock - 1) / kLoopBlock;
        const bool with_g = grad != nullptr;
        const double* v = reduce(nb, [&](const LoopOut rows) {
            if (with_g) hipLaunchKernelGGL(gicp_fdf_kernel<true>, dim3(unsigned(nb)), dim3(kLoopBlock), 0, stream, g.moved.x(), g.moved.y(), g.moved.z(), n, T,
                                           (const float4*)g.tgt_grid.d_by_id.p, (const int*)g.corr.p, (const double*)g.mahal.p, rows);
            else hipLaunchKernelGGL(gicp_fdf_kernel<false>, dim3(unsigned(nb)), dim3(kLoopBlock), 0, stream, g.moved.x(), g.moved.y(), g.moved.z(), n, T,
                                    (const float4*)g.tgt_grid.d_by_id.p, (const int*)g.corr.p, (const double*)g.mahal.p, rows);
        });
        const double m = v[with_g ? 13 : 1];
        if (f) *f = v[0] / m;
        if (!with_g) return;
        double Racc[9];
        for (int a = 0; a < 3; ++a) grad[a] = v[1 + a] * (2.0 / m);
        for (int q = 0; q < 9; ++q) Racc[q] = v[4 + q] * (2.0 / m);
        loop::gicp_rotation_gradient(x, Racc, grad);
    }

    // the ten filtered clouds of one Match, produced in the order the stages consume them
    struct FilterAhead {
        static constexpr int kN = 10;
        std::vector<PtI> out[kN];
        std::mutex mx;
        std::condition_variable cv;
        int ready = 0;
        bool stop = false;
        std::exception_ptr error;
        std::thread th;
        void start(const std::vector<PtI>& source, const std::vector<PtI>& target) {
            th = std::thread([this, &source, &target] {
                static const float resolution[4] = {10.0f, 5.0f, 3.0f, 2.0f};
                for (int k = 0; k < kN; ++k) {
                    {
                        std::lock_guard<std::mutex> lk(mx);
                        if (stop) return;
                    }
                    try {
                        const float l = k < 8 ? resolution[k / 2] * 0.2f : (k == 8 ? 0.5f : 0.4f);  // NDT stages: resolution * 0.2f; GICP: 0.5 / 0.4
                        out[k] = voxel_grid((k & 1) ? target : source, l);
                    } catch (...) {
                        std::lock_guard<std::mutex> lk(mx);
                        error = std::current_exception();
                        ready = kN;
                        cv.notify_all();
                        return;
                    }
                    {
                        std::lock_guard<std::mutex> lk(mx);
                        ready = k + 1;
                    }
                    cv.notify_all();
                }
            });
        }
        std::vector<PtI> take(int k) {
            std::unique_lock<std::mutex> lk(mx);
            cv.wait(lk, [&] { return ready > k; });
            if (error) std::rethrow_exception(error);
            return std::move(out[k]);
        }
        ~FilterAhead() {
            if (th.joinable()) {
                { std::lock_guard<std::mutex> lk(mx); stop = true; }
                th.join();
            }
        }
    };

    // buffers that live as long as the matcher (one per device, fls_reg.hip): no allocation on the second Match
    DeviceGridBuilder builder;
    DevCloud src_dev, tgt_dev, src_own;
    TargetLeaves leaves;
    GicpRun g;
    CellGridImage src_grid;

    // ---- the GICP stages, one function each: the Match (loop_device.hpp) and the test hooks (abi_debug_loop.hpp) call these -----------------
    // 20 neighbours of a 0.4-0.5 m down-sampled cloud lie within ~1.2 m on a surface: the 27 cells certify most queries
    static constexpr float kGicpCell = 1.5f;
    // a cloud's cell grid (ids = cloud indices; by_id: with the copy the cost kernel reads): on the device, else -- or with host_grid -- on the host
    fls_status cell_grid(CellGridImage& grid, Filtered& c, float cell, bool by_id, bool host_grid = false) {
        const DevCloud& d = planes(c);
        if (!host_grid && builder.run(grid, d.x(), d.y(), d.z(), d.n, cell, 1, by_id, stream)) return FLS_OK;
        return grid.build(rows_of(c), cell, stream, 1, by_id);
    }
    // computeCovariances: the 20-NN covariances of a cloud in its own grid -> cov[n][9] on the device
    void gicp_cov(const DevCloud& c, const CellGridImage& grid, double epsilon, double* cov) {
        hipLaunchKernelGGL(gicp_cov_kernel, dim3(unsigned((c.n + kCovWaves - 1) / kCovWaves)), dim3(64 * kCovWaves), 0, stream, c.x(), c.y(), c.z(), int(c.n), cell_dev(grid), epsilon, cov);
        FLS_HIP(hipGetLastError());
    }
    // one outer iteration's correspondences of g.moved (n points) under `transformation` in g.tgt_grid -> g.corr, g.mahal
    void gicp_corr(const int n, const LoopMat4f& transformation, const double dist_threshold, const GicpRot& rot) {
        hipLaunchKernelGGL(gicp_corr_kernel, dim3(unsigned((n + 63) / 64)), dim3(64), 0, stream, g.moved.x(), g.moved.y(), g.moved.z(), n, transformation, cell_dev(g.tgt_grid),
                           float(dist_threshold), dist_threshold, rot, (const double*)g.cov_src.p, (const double*)g.cov_tgt.p, g.corr.p, g.mahal.p);
        FLS_HIP(hipGetLastError());
    }
    // getFitnessScore's sums over src_own (n points) under `fin` against g.tgt_grid: v[0] squared distances, v[1] their number
    const double* fitness_sums(const int n, const LoopMat4f& fin) {
        const CellGridDev cg_tgt = cell_dev(g.tgt_grid);
        const int nb = (n + kLoopBlock - 1) / kLoopBlock;
        return reduce(nb, [&](const LoopOut rows) {
            hipLaunchKernelGGL(loop_fitness_kernel, dim3(unsigned(nb)), dim3(kLoopBlock), 0, stream, src_own.x(), src_own.y(), src_own.z(), n, fin, cg_tgt, rows);
        });
    }

    void print_timing(double t_filter, double t_leaves, double t_ndt, double t_gicp_setup, double t_gicp, double t_fit) const {
        std::fprintf(stderr, "[fls loop] ms: 10 filters %.2f, leaf Gaussians + uploads %.2f, NDT align (%d evaluations) %.2f, GICP grids + covariances %.2f, GICP loop (%d evaluations) %.2f, fitness %.2f\n",
                     t_filter, t_leaves, st.ndt_evaluations[0] + st.ndt_evaluations[1] + st.ndt_evaluations[2] + st.ndt_evaluations[3], t_ndt, t_gicp_setup, st.gicp_evaluations, t_gicp, t_fit);
    }

    // the outer GICP iterations over g.moved / g.tgt_grid / the covariances (n = source points): T = the final transformation, which is returned
    LoopMat4f gicp_outer(const int n, const LoopMat4f& guess, double* T) {
        LoopMat4f transformation = loop::ident(), previous = loop::ident();
        const double corr_dist = 2.0, dist_threshold = corr_dist * corr_dist, rotation_epsilon = 2e-3, transformation_epsilon = 5e-4;
        const auto fdf = [&](const double* x, double* f, double* grad) { gicp_fdf(g, x, f, grad); };
        int nr = 0;
        for (bool converged = false; !converged;) {
            GicpRot rot;
            for (int j = 0; j < 3; ++j)
                for (int i = 0; i < 3; ++i) {
                    double sum = 0.0;
                    for (int k = 0; k < 4; ++k) sum += double(transformation.m[i + 4 * k]) * double(guess.m[k + 4 * j]);
                    rot.R[i + 3 * j] = sum;
                }
            gicp_corr(n, transformation, dist_threshold, rot);
            {   // number of correspondences (the cost kernel's count column at the current pose; also warms nothing else)
                double f0;
                const double x0[6] = {0, 0, 0, 0, 0, 0};
                const int before = g.evaluations;
                gicp_fdf(g, x0, &f0, nullptr);
                g.evaluations = before;
                g.n_corr = int(mail_host->v[1]);
            }
            previous = transformation;
            if (!loop::gicp_estimate(g.n_corr, transformation, fdf, g.inner_total)) { st.gicp_failed = 1; break; }
            double delta = 0.0;
            for (int k = 0; k < 4; ++k)
                for (int l = 0; l < 4; ++l) {
                    const double ratio = (k < 3 && l < 3) ? 1.0 / rotation_epsilon : 1.0 / transformation_epsilon;
                    delta = std::max(delta, ratio * std::fabs(double(previous.m[k + 4 * l]) - double(transformation.m[k + 4 * l])));
                }
            ++nr;
            if (debug) std::fprintf(stderr, "[fls loop] gicp outer %d: corr %d inner_total %d evals %d delta %.9g t = %.9g %.9g %.9g\n", nr, g.n_corr, g.inner_total, g.evaluations, delta,
                                    double(transformation.m[12]), double(transformation.m[13]), double(transformation.m[14]));
            if (nr >= 30 || delta < 1) { converged = true; previous = transformation; }
        }
        const LoopMat4f fin = loop::mul(previous, guess);
        for (int i = 0; i < 16; ++i) T[i] = double(fin.m[i]);
        st.gicp_iterations = nr; st.gicp_inner_iterations = g.inner_total; st.gicp_evaluations = g.evaluations; st.gicp_correspondences = g.n_corr;
        return fin;
    }

    // getFitnessScore of src_own (n points) under `fin` against g.tgt_grid; ends with the stream drained
    void fitness_score(const int n, const LoopMat4f& fin, float* fitness) {
        const double* v = fitness_sums(n, fin);
        if (v[1] > 0) *fitness = float(v[0] / v[1]);
        FLS_HIP(hipStreamSynchronize(stream));
    }

    // ======================================================================================================================
    // The Match, from host clouds (run) and from clouds that lie on this device (run_device, include/fls_loop_device.h).  Defined in
    // kernels_loop_leaves.hpp (the leaf build) and loop_device.hpp, which fls_reg.hip includes last: the code object keeps the order of
    // the kernels in front.
    // ======================================================================================================================
    struct DevInput {  // x | y | z | intensity planes of n floats each, any 4-byte alignment; in == nullptr: intensity 0
        const float *x = nullptr, *y = nullptr, *z = nullptr, *in = nullptr;
        size_t n = 0;
    };
    enum { kStatMatches = 0, kStatFiltersDevice, kStatFiltersHost, kStatLeavesDevice, kStatLeavesHost, kStatInputBytes, kStatFilteredBytes, kStatSlots };
    unsigned long long dstat[kStatSlots] = {0, 0, 0, 0, 0, 0, 0};
    bool device_leaves = true;  // FLS_LOOP_DEVICE_LEAVES=0 (read by init()): every leaf grid through build_target
    enum LeafBuild { kLeavesNone, kLeavesBuilt, kLeavesDeclined };
    DevicePairSort leaf_sort;
    DevBuf<VgHeader> d_leaf_hdr;
    PinnedBuf<VgHeader> h_leaf_hdr;
    DevBuf<unsigned> d_leaf_lx, d_leaf_bt;
    DevBuf<float> d_zero;             // the intensity plane of a cloud that has none
    DevCloud tgt_filtered;           // a declined target filter's result, uploaded
    LeafBuild build_target_device(const float* x, const float* y, const float* z, size_t n, float resolution, TargetLeaves& tl);
    void download_leaves(TargetLeaves& tl);
    bool target_leaves(Filtered& tgt, float resolution, TargetLeaves& tl, bool on_device, bool counted);
    struct CloudSource;
    fls_status match(CloudSource& clouds, double* T, float* fitness);
    fls_status run(const std::vector<PtI>& source, const std::vector<PtI>& target, double* T, float* fitness);
    fls_status run_device(const DevInput& source, const DevInput& target, double* T, float* fitness);
};

}  // namespace fls
