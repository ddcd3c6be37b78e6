// matcher_p2plane_ivox.hpp -- the Match side of FLS_P2PLANE_IVOX, the replacement of
// LoamPointToPlaneIVOX<double> (include/registration/loam_point_to_plane_ivox.h:30-355).  The map itself (InitIVox, the insert side of
// AddCloudToLocalMap on host and device, export / import / replicas) is ivox_map.hpp's IvoxMap; this file decides what goes into it and
// matches against it.
//
//   AddCloudToLocalMap  :60-139   first call / localization: insert all; later: the
//                                 centre-distance down-sampling rule on the last kNN result
//   Match               :141-216  device-resident Gauss-Newton loop (2 launches / iteration, the host waits on a
//                                 mailbox word instead of synchronising the stream)
//   GetFitnessScore     :225-253  localization mode only (FloatNaN otherwise)
//   fls_match_batch_shared_ivox   groups of batch jobs in shared launches (include/fls_batch_ivox.h; the group driver is matcher_base.hpp's)
#pragma once
#include "matcher_base.hpp"
#include "kernels_p2plane.hpp"
#include "kernels_knn.hpp"
#include "kernels_ivox_coop.hpp"
#include "kernels_ivox_update.hpp"
#include "ivox_map.hpp"
#include "kernels_localmap.hpp"
#include "fitness_host.hpp"
#include <thread>
#include <chrono>
#include <hip/hip_ext.h>

namespace fls {

constexpr int kIvoxXcdChunk = 8;  // workgroups per XCD chunk of the kNN block re-map (ivox_knn_kernel's `chunk`)

// The two launches around the map-update decision, each written once: the matcher below and the test hooks of include/fls_debug_ivox_decide.h
// (abi_debug_ivox_decide.hpp) launch through these, so the grid rule and the argument order cannot drift apart.
inline void launch_nn_materialize(const unsigned* nn_ids, unsigned char* nn_cnt, const size_t nn_n, const float4* map_pts, const unsigned n_slots, float4* nn_pts,
                                  hipStream_t stream) {
    hipLaunchKernelGGL(ivox_nn_materialize_kernel, dim3(unsigned((nn_n + 255) / 256)), dim3(256), 0, stream, nn_ids, nn_cnt, int(nn_n), map_pts, n_slots, nn_pts);
}
struct DecideLaunch {
    const float *sx, *sy, *sz;  // the source points, n of them
    size_t n;
    const double* T;            // the pose as a launch argument (a speculative launch takes GnState::T instead)
    float4* nn_pts;             // [nn_n][5] neighbour rows
    unsigned char* nn_cnt;      // [nn_n]
    size_t nn_n;
    double fs;                  // filter_size_map_min
    unsigned char* code;        // [n]
    float4* pw;                 // [n]
    const unsigned* nn_ids;     // [nn_n][8], may be null
    const float4* map_pts;
    unsigned n_slots;
    uint2 *lx, *bt;             // lx null: no counting
    unsigned *status, *apply;
    const GnState* gn;          // non-null: the speculative form
    int max_it;
    bool rows_too;              // the MATERIALIZE form: the grid covers max(n, nn_n) points
};
inline void launch_add_decide(const DecideLaunch& a, hipStream_t stream) {
    Pose16 Tw;
    std::memcpy(Tw.m, a.T, sizeof(Tw.m));
    const size_t m = a.rows_too ? std::max(a.n, a.nn_n) : a.n;
    with_bools([&](auto ROWS) {
        hipLaunchKernelGGL(ivox_add_decide_kernel<ROWS.value>, dim3(unsigned((m + 255) / 256)), dim3(256), 0, stream, a.sx, a.sy, a.sz, int(a.n), Tw, a.nn_pts,
                           a.nn_cnt, int(a.nn_n), a.fs, a.code, a.pw, a.nn_ids, a.map_pts, a.n_slots, a.lx, a.bt, a.status, a.apply, a.gn, a.max_it);
    }, a.rows_too);
}

// pcl::transformPoint with Affine3d(T_): double evaluation, float result
inline PtI ivox_xform_d(const PtI& p, const double* T) {
    PtI r = p;
    const double x = p.x, y = p.y, z = p.z;
    r.x = float(((T[0] * x + T[4] * y) + T[8] * z) + T[12]);
    r.y = float(((T[1] * x + T[5] * y) + T[9] * z) + T[13]);
    r.z = float(((T[2] * x + T[6] * y) + T[10] * z) + T[14]);
    return r;
}
// AddCloudToLocalMap's rule (:79-131) on the host, over arrays: point i is src[i * src_stride ..+3], its list near[(i * 5 + k) * near_stride ..+3] with
// cnt[i] entries (no list at all from nn_n on) -> code[i] (0 drop, 1 points_to_add, 2 point_no_need_downsample), pw[3 * i ..+3] the world point.
// What add_cloud_impl runs for a cloud that is not the resident scan, and fls_debug_ivox_decide_host.
inline void ivox_decide_host(const float* src, const size_t src_stride, const size_t n, const double* T, const double fs, const float* near_rows,
                             const size_t near_stride, const unsigned char* cnt_of, const size_t nn_n, unsigned char* code, float* pw_out) {
    const double half = 0.5 * fs;
    for (size_t i = 0; i < n; ++i) {
        const PtI pw = ivox_xform_d(PtI{src[i * src_stride], src[i * src_stride + 1], src[i * src_stride + 2], 0.0f}, T);
        pw_out[3 * i] = pw.x; pw_out[3 * i + 1] = pw.y; pw_out[3 * i + 2] = pw.z;
        const int cnt = i < nn_n ? cnt_of[i] : 0;
        code[i] = 1;
        if (cnt > 0) {
            const auto near = [&](const int k, const int a) { return double(near_rows[(i * 5 + size_t(k)) * near_stride + size_t(a)]); };
            const double c[3] = {(std::floor(double(pw.x) / fs) + 0.5) * fs, (std::floor(double(pw.y) / fs) + 0.5) * fs,
                                 (std::floor(double(pw.z) / fs) + 0.5) * fs};
            const double d0[3] = {near(0, 0) - c[0], near(0, 1) - c[1], near(0, 2) - c[2]};
            if (std::fabs(d0[0]) > half && std::fabs(d0[1]) > half && std::fabs(d0[2]) > half) {
                code[i] = 2;
                continue;
            }
            bool need_add = true;
            const double e[3] = {double(pw.x) - c[0], double(pw.y) - c[1], double(pw.z) - c[2]};
            const double dist = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
            if (cnt >= 5) {
                for (int k = 0; k < 5; ++k) {
                    const double f[3] = {near(k, 0) - c[0], near(k, 1) - c[1], near(k, 2) - c[2]};
                    if ((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2] < dist + 1.0e-6) { need_add = false; break; }
                }
            }
            code[i] = need_add ? 1 : 0;
        }
    }
}

struct P2PlaneIvoxMatcher final : fls_matcher {
    IvoxMap map;
    // a batch lane (fls_match_batch) reads its owner's map; its own stays empty and idle
    const IvoxMap* borrowed = nullptr;
    const IvoxMap& read_map() const { return borrowed ? *borrowed : map; }
    bool host_timing = false;  // FLS_HOST_TIMING=1: print the host-side cost of every map update
    // the decision + update chain queued behind the iterations the Match is expected to need, gated on the device (ivox_add_decide_kernel):
    // removes the host's mailbox turnaround + first-launch latency (~14 us) in front of the map update
    bool spec_pending = false;
    // what the decision launch writes from Match state: insertion code + world point per point of the resident scan
    DevBuf<unsigned char> d_code;
    DevBuf<float4> d_pw;
    std::vector<unsigned char> h_code;
    std::vector<Pt4> h_pw;
    DevBuf<unsigned> d_ticket;
    const double filter_size_map_min = 0.5;  // :351

    DevScan scan;
    // per-point state that outlives an iteration (Q1) or a Match (nearest_points_, :257)
    DevBuf<float4> d_nn;          // [n][5]
    DevBuf<unsigned char> d_nn_cnt;   // neighbour count (bits 0-2) | 0x80 when the point's list is in rows form
    DevBuf<unsigned> d_nn_ids;        // [n][8] map slots of the neighbours (ids form: what the kNN kernel writes)
    bool nn_rows_current = true;      // every list is in rows form
    size_t nn_n = 0;              // logical size of nearest_points_
    int nn_prev = 0;              // its size before the Match in flight
    DevBuf<double> d_J;           // [7][n]
    DevBuf<unsigned char> d_flag;
    size_t number_planar_point = 0;
    double T_[16]{}, final_T[16]{};
    bool have_final = false;
    // localization-mode fitness map (kd-tree stand-in)
    CellGridImage fitness_grid;
    bool have_fitness_grid = false;
    // a whole cloud on its way into the empty map (IvoxMap::bulk_build): staged and uploaded apart from the resident scan, which a reload must not disturb
    DevScan cloud_dev;
    DeviceGridBuilder fitness_builder;
    std::vector<Pt4> h_nn;
    std::vector<unsigned char> h_cnt, h_flag;
    // fls_knn_order.h: the kNN launches in the reference's neighbour order (kernels_ivox_knn_reforder.hpp), FLS_IVOX_KNN_ORDER=reference at creation
    bool knn_reference = false;
    size_t n_ref_launches = 0;                     // kNN launches run in reference order (fls_map_size slot 177, with the lanes')
    DevBuf<unsigned long long> d_ref_fallbacks;    // queries that kept the default order because of the per-query limit W, since creation
    size_t n_ref_fallbacks = 0;                    // ... as of the last reference-order Match (slot 178, with the lanes')

    ~P2PlaneIvoxMatcher() override { if (stream) (void)hipStreamSynchronize(stream); }
    fls_status init() {
        if (unset_d(p.point_to_planar_thres) || unset_d(p.position_converge_thres) || unset_d(p.rotation_converge_thres))
            return FLS_ERR_INVALID;  // CHECK_NE(..., max()) at :45-48
        init_common();
        host_timing = host_timing_enabled();
        init_tickets(d_ticket);
        map.init(stream, unsigned(kind), p.is_localization_mode != 0);
        if (const char* e = std::getenv("FLS_IVOX_KNN_ORDER")) knn_reference = std::strcmp(e, "reference") == 0;
        d_ref_fallbacks.reserve(1);
        FLS_HIP(hipMemsetAsync(d_ref_fallbacks.p, 0, sizeof(unsigned long long), stream));
        return FLS_OK;
    }
    fls_status set_knn_order(const int mode) override { knn_reference = mode == FLS_KNN_ORDER_REFERENCE; return FLS_OK; }
    int knn_order() const override { return knn_reference ? FLS_KNN_ORDER_REFERENCE : FLS_KNN_ORDER_DEFAULT; }
    void tune_lane(fls_matcher& lane) override { static_cast<P2PlaneIvoxMatcher&>(lane).knn_reference = knn_reference; }
    // what earlier Matches left behind, forgotten (nearest_points_ of a fresh matcher is empty): per batch job, and whenever the map is replaced
    void reset_match_state() { nn_n = 0; have_final = false; nn_rows_current = true; spec_pending = false; }
    void reset_job_state() override { reset_match_state(); }

    // ids form -> rows form for every point (the ids are slots of the image as it is NOW: call before anything moves slots)
    void ensure_nn_rows() {
        if (nn_rows_current || nn_n == 0) { nn_rows_current = true; return; }
        const IvoxImage& im = read_map().image;
        // (slot bound = the allocation: in device mode the host's `used` is stale)
        launch_nn_materialize(d_nn_ids.p, d_nn_cnt.p, nn_n, im.d_pts.p, unsigned(im.d_pts.cap), d_nn.p, stream);
        FLS_HIP(hipGetLastError());
        nn_rows_current = true;
    }
    void download_nn() {
        ensure_nn_rows();
        const size_t n = nn_n;
        h_nn.resize(n * 5);
        h_cnt.resize(n);
        if (n == 0) return;
        FLS_HIP(hipMemcpyAsync(h_nn.data(), d_nn.p, n * 5 * sizeof(float4), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipMemcpyAsync(h_cnt.data(), d_nn_cnt.p, n, hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        for (unsigned char& c : h_cnt) c &= 7;  // (bit 7 = rows form)
    }

    fls_status add_cloud(const float* c0, size_t n0, const float* c1, size_t n1, int stride) override {
        if (c1 != nullptr && n1 != 0) return FLS_ERR_INVALID;  // CHECK_EQ(cloud_list.size(), 1) :61
        if (!map.is_replica() && (p.is_localization_mode || map.is_first)) {  // the cloud goes in whole
            fls_status rc = FLS_OK;
            if (add_cloud_bulk(c0, n0, stride, rc)) return rc;
        }
        const std::vector<PtI> cloud = cloud_from(c0, n0, stride);
        return add_cloud_impl(cloud);
    }
    // add_cloud from a cloud on the device: the same decisions, the bounds by a device reduction (equal to plane_bounds: min and max of the same floats)
    DeviceBounds cloud_bounds;
    fls_status add_cloud_device(const HandoffCloud& c, const HostRows& rows, bool* took_planes) override {
        *took_planes = false;
        if (!map.is_replica() && (p.is_localization_mode || map.is_first) && c.n != 0 && bulk_admits(c.n)) {
            const auto t0 = std::chrono::steady_clock::now();
            ensure_nn_rows();
            float lo[3], hi[3];
            cloud_bounds.run(c.x, c.y, c.z, c.n, stream, lo, hi);
            fls_status rc = FLS_OK;
            if (bulk_core(c.x, c.y, c.z, c.n, lo, hi, rows, rc, t0)) { *took_planes = true; return rc; }
        }
        return add_cloud_impl(rows());
    }
    // coordinate bounds of the staged cloud per axis, NaN ignored (an infinite coordinate shows: the build declines on it)
    static void plane_bounds(const float* v, const size_t n, float& lo, float& hi) {
        float mn = std::numeric_limits<float>::infinity(), mx = -mn;
        size_t i = 0;
#if defined(__SSE__)
        __m128 vmn = _mm_set1_ps(mn), vmx = _mm_set1_ps(mx);
        for (; i + 4 <= n; i += 4) {  // (min / max return their second operand when the first is NaN)
            const __m128 q = _mm_loadu_ps(v + i);
            vmn = _mm_min_ps(q, vmn); vmx = _mm_max_ps(q, vmx);
        }
        float a[4], b[4];
        _mm_storeu_ps(a, vmn); _mm_storeu_ps(b, vmx);
        for (int k = 0; k < 4; ++k) { if (a[k] < mn) mn = a[k]; if (b[k] > mx) mx = b[k]; }
#endif
        for (; i < n; ++i) { if (v[i] < mn) mn = v[i]; if (v[i] > mx) mx = v[i]; }
        lo = mn; hi = mx;
    }
    // The first cloud of a mapping handle / every reload of a localization handle, built on the device.  true: `rc` answers the call.
    // false: declined (IvoxMap counts why; an empty cloud and a map that is not blank count nowhere), the host path runs as ever.
    bool add_cloud_bulk(const float* c0, const size_t n0, const int stride, fls_status& rc) {
        if (n0 == 0 || c0 == nullptr) return false;
        if (!bulk_admits(n0)) return false;
        const auto t0 = std::chrono::steady_clock::now();
        ensure_nn_rows();  // (lists in ids form name slots of the image about to be replaced)
        cloud_dev.upload_raw(c0, n0, stride, stream);
        float lo[3], hi[3];
        for (int a = 0; a < 3; ++a) plane_bounds(cloud_dev.stage.p + size_t(a) * n0, n0, lo[a], hi[a]);
        return bulk_core(cloud_dev.x.p, cloud_dev.y.p, cloud_dev.z.p, n0, lo, hi, [&] { return cloud_from(c0, n0, stride); }, rc, t0);
    }
    // what add_cloud_bulk can say before the cloud is touched (a decline is counted by IvoxMap)
    bool bulk_admits(const size_t n0) {
        if (!p.is_localization_mode && !map.is_blank()) return false;  // (an imported map with is_first set: the cloud joins what is there)
        return map.bulk_build_applies(n0);
    }
    // the build itself, from x | y | z on the device with their bounds; host_cloud(): the same cloud on the host (the fitness grid's fallback)
    template <class HostCloud>
    bool bulk_core(const float* x, const float* y, const float* z, const size_t n0, const float (&lo)[3], const float (&hi)[3], HostCloud&& host_cloud,
                   fls_status& rc, const std::chrono::steady_clock::time_point t0) {
        const auto t1 = std::chrono::steady_clock::now();
        if (p.is_localization_mode) { map.become_empty(); map.is_first = true; }
        if (!map.bulk_build(x, y, z, n0, lo, hi)) return false;
        map.is_first = false;
        const auto t2 = std::chrono::steady_clock::now();
        rc = FLS_OK;
        if (p.is_localization_mode) {  // :134-138 kd-tree for GetFitnessScore, from the cloud already on the device
            if (!fitness_builder.run(fitness_grid, x, y, z, n0, 1.0f, 1, false, stream))
                rc = fitness_grid.build(host_cloud(), 1.0f, stream);
            FLS_HIP(hipStreamSynchronize(stream));
            have_fitness_grid = (rc == FLS_OK);
        }
        if (host_timing) {
            const auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            std::fprintf(stderr, "[fls host] device map build: %zu points into %zu voxels: stage+upload %.3f ms, keys+sort+scans %.3f ms, pool+cells+points %.3f ms, "
                         "fitness grid %.3f ms, total %.3f ms\n", n0, map.dev_n_alive, ms(t0, t1), map.build_ms[0], map.build_ms[1], ms(t2, std::chrono::steady_clock::now()),
                         ms(t0, std::chrono::steady_clock::now()));
        }
        return true;
    }

    // the decision launch (ivox_add_decide_kernel): codes + world points of the resident scan; while the device holds the map it also counts
    // the codes and opens the batch (IvoxMap::count_args).  speculative: gated on the device by the Gauss-Newton state, pose read from it.
    // Returns "counted".
    bool launch_decide(const size_t n, const bool speculative) {
        d_code.reserve(n);
        d_pw.reserve(n);
        const GnState* const gn = speculative ? (const GnState*)d_state.p : nullptr;
        const IvoxMap::CountArgs c = map.count_args(n);
        // (the update moves map slots: lists still in ids form become rows in the same launch)
        const bool rows_too = (speculative || !nn_rows_current) && nn_n > 0;
        launch_add_decide(DecideLaunch{scan.x.p, scan.y.p, scan.z.p, n, T_, d_nn.p, d_nn_cnt.p, nn_n, filter_size_map_min, d_code.p, d_pw.p, d_nn_ids.p,
                                       map.image.d_pts.p, unsigned(map.image.d_pts.cap), c.lx, c.bt, c.status, c.apply, gn, int(p.max_iterations), rows_too},
                          stream);
        if (rows_too && !speculative) nn_rows_current = true;
        FLS_HIP(hipGetLastError());
        return c.lx != nullptr;
    }

    // A decided batch into the map: insertion code + world point of n source points stand in d_code / d_pw (launch_decide, or the test hook
    // fls_debug_ivox_add_points), `counted` says the codes are counted per block (IvoxMap::count_args), `enqueued` that the update chain is
    // queued already (the speculative chain).  A Device map tries the device chain; a batch it refuses, and every batch of a map the host holds,
    // is replayed on the mirror in the reference's order (code 1 in source order, then code 2).  on_mirror false: the device applied the batch,
    // nothing is left to do.  on_mirror true: the mirror took the lists as far as `rc` says and the caller settles the image (settle_mirror).
    // chain_status (may be null): the status word the chain's commit published, 0xFFFFFFFF when no chain ran.
    fls_status apply_decided(const size_t n, const bool counted, const bool enqueued, const bool scan_intensities, const std::chrono::steady_clock::time_point tm0,
                             bool& on_mirror, unsigned* chain_status) {
        using Verdict = IvoxMap::Verdict;
        HostIvox& ivox = map.ivox;
        std::vector<PtI> to_add, no_downsample;
        on_mirror = true;
        if (chain_status) *chain_status = 0xFFFFFFFFu;
        if (n) {
            if (!enqueued && map.on_device() && !map.enqueue_update(d_code.p, d_pw.p, n, counted)) map.fall_back(Verdict::Refused);  // (too large for the device path)
            if (map.on_device()) {
                Verdict v = map.await_update(n);
                if (v == Verdict::Skipped) {
                    // a speculative chain that judged "no update here" although the host wants one (cannot happen while host and device
                    // read the same words; kept as a safe path): decide + apply the ordinary way
                    nn_rows_current = false;  // (the skipped launch materialised nothing)
                    const bool recounted = launch_decide(n, false);
                    ensure_nn_rows();
                    v = map.enqueue_update(d_code.p, d_pw.p, n, recounted) ? map.await_update(n) : Verdict::Refused;
                }
                if (chain_status) *chain_status = map.upd_mb_host->status;
                if (v == Verdict::Applied) {
                    if (host_timing)
                        std::fprintf(stderr, "[fls host] device AddPoints: %u points into %u voxels, %.3f ms\n", map.upd_mb_host->added, map.upd_mb_host->touched,
                                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tm0).count());
                    on_mirror = false;
                    return FLS_OK;
                }
                // refused (an eviction-order conflict, the point array or brick pool full): nothing was applied; the exact sequential
                // path below replays the batch on the host mirror
                map.fall_back(v);
            }
            map.to_mirror();   // (an ImageOnly map -- bulk-built, device update not allowed -- has no mirror yet)
            h_code.resize(n);  // (host copies only on this path: the device applied nothing)
            h_pw.resize(n);
            FLS_HIP(hipMemcpyAsync(h_code.data(), d_code.p, n, hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipMemcpyAsync(h_pw.data(), d_pw.p, n * sizeof(float4), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            if (scan_intensities) scan.fetch_stage(stream);  // (an attached scan's intensities are still on the device)
            for (size_t i = 0; i < n; ++i) {
                if (h_code[i] == 0) continue;
                const PtI pw{h_pw[i].x, h_pw[i].y, h_pw[i].z, scan_intensities ? scan.staged_intensity(i) : 0.0f};
                (h_code[i] == 1 ? to_add : no_downsample).push_back(pw);
            }
        }
        const auto tm1 = std::chrono::steady_clock::now();
        // (each list is all-or-nothing -- HostIvox::add_points checks every key first -- so a key beyond the limit among the code-2 points
        // leaves the code-1 points inserted: the caller settles the image whatever `rc` says)
        fls_status rc = ivox.add_points(to_add.data(), to_add.size());
        if (rc != FLS_OK) return rc;
        rc = ivox.add_points(no_downsample.data(), no_downsample.size());
        if (rc != FLS_OK) return rc;
        if (host_timing) {
            const auto tm2 = std::chrono::steady_clock::now();
            std::fprintf(stderr, "[fls host] decide+lists %.3f ms (%zu + %zu pts), AddPoints %.3f ms\n",
                         std::chrono::duration<double, std::milli>(tm1 - tm0).count(), to_add.size(), no_downsample.size(),
                         std::chrono::duration<double, std::milli>(tm2 - tm1).count());
        }
        return FLS_OK;
    }
    // the image behind a mirror that took insertions: the journal scattered (or the image re-flattened), the map back on the device where allowed
    void settle_mirror() {
        map.mirror_changed();
        const auto tr0 = std::chrono::steady_clock::now();
        map.refresh();
        if (host_timing)
            std::fprintf(stderr, "[fls host] refresh_image %.3f ms (%zu pt updates, %zu cell updates)\n",
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr0).count(), map.image.pt_upd.size(),
                         map.image.cell_upd.size());
    }
    // fls_debug_ivox_add_points (include/fls_debug_ivox_update.h): one decided batch, given by the caller instead of launch_decide
    fls_status debug_add_points(const float* world_xyz, const unsigned char* code, const size_t n, unsigned* chain_status) {
        *chain_status = 0xFFFFFFFFu;
        const auto tm0 = std::chrono::steady_clock::now();
        bool counted = false;
        if (n) {
            ensure_nn_rows();  // (the update moves map slots)
            d_code.reserve(n);
            d_pw.reserve(n);
            h_pw.resize(n);
            for (size_t i = 0; i < n; ++i) h_pw[i] = Pt4{world_xyz[3 * i], world_xyz[3 * i + 1], world_xyz[3 * i + 2], 0};  // (w = 0.f, as the decision launch writes it)
            FLS_HIP(hipMemcpyAsync(d_code.p, code, n, hipMemcpyHostToDevice, stream));
            FLS_HIP(hipMemcpyAsync(d_pw.p, h_pw.data(), n * sizeof(float4), hipMemcpyHostToDevice, stream));
            FLS_HIP(hipStreamSynchronize(stream));  // (pageable sources: both may change once the call returns)
            const IvoxMap::CountArgs c = map.count_args(n);
            if (c.lx) {  // what the decision launch does besides deciding: block-local counts, raw block totals, the two status words reset
                const IvoxUpdBatch b{d_code.p, d_pw.p, int(n), c.lx, c.bt, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
                hipLaunchKernelGGL(ivox_upd_count, dim3(unsigned(IvoxMap::update_blocks(n))), dim3(kUpdBlock), 0, stream, b);
                FLS_HIP(hipGetLastError());
                FLS_HIP(hipMemsetAsync(c.status, 0, sizeof(unsigned), stream));  // kUpdOk
                FLS_HIP(hipMemsetAsync(c.apply, 0, sizeof(unsigned), stream));
                counted = true;
            }
        }
        bool on_mirror = false;
        const fls_status rc = apply_decided(n, counted, /*enqueued=*/false, /*scan_intensities=*/false, tm0, on_mirror, chain_status);
        if (on_mirror) settle_mirror();
        return rc;
    }

    fls_status add_cloud_impl(const std::vector<PtI>& planar_cloud, const bool from_resident_scan = false, const bool pre_enqueued = false) {
        HostIvox& ivox = map.ivox;
        if (map.is_replica()) return FLS_ERR_STATE;
        if (p.is_localization_mode) { map.become_empty(); map.is_first = true; }
        fls_status rc = FLS_OK;
        if (!(from_resident_scan && !map.is_first)) { ensure_nn_rows(); map.to_mirror(); }  // every other branch works on the host mirror
        if (map.is_first) {
            const auto tm0 = std::chrono::steady_clock::now();
            rc = ivox.add_points(planar_cloud.data(), planar_cloud.size());
            if (rc != FLS_OK) return rc;
            map.is_first = false;
            if (host_timing)
                std::fprintf(stderr, "[fls host] host map build: AddPoints of %zu points into %zu voxels %.3f ms\n", planar_cloud.size(), ivox.n_alive,
                             std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tm0).count());
        } else if (from_resident_scan) {
            // :79-131 on the device (the cloud is the scan just matched, still resident): decision code + world point
            // per source point; the host only walks the codes to build the two insertion lists in index order.
            const size_t n = std::min(number_planar_point, scan.n);
            const auto tm0 = std::chrono::steady_clock::now();
            bool counted = false;
            if (n && !pre_enqueued) {
                counted = launch_decide(n, /*speculative=*/false);
                ensure_nn_rows();
            }
            bool on_mirror = false;
            rc = apply_decided(n, counted, pre_enqueued, /*scan_intensities=*/true, tm0, on_mirror, nullptr);
            if (!on_mirror) return rc;  // (the device applied the batch)
            if (rc != FLS_OK) { settle_mirror(); return rc; }
        } else {
            // external non-first call with an arbitrary cloud: same rule on the host (:79-131)
            download_nn();
            std::vector<PtI> to_add, no_downsample;
            const size_t n = std::min(number_planar_point, planar_cloud.size());
            static_assert(sizeof(PtI) == 4 * sizeof(float) && sizeof(Pt4) == 4 * sizeof(float), "ivox_decide_host strides");
            std::vector<unsigned char> code(n);
            std::vector<float> pw(3 * n);
            ivox_decide_host(reinterpret_cast<const float*>(planar_cloud.data()), 4, n, T_, filter_size_map_min, reinterpret_cast<const float*>(h_nn.data()), 4,
                             h_cnt.data(), nn_n, code.data(), pw.data());
            for (size_t i = 0; i < n; ++i) {
                if (code[i] == 0) continue;
                (code[i] == 1 ? to_add : no_downsample).push_back(PtI{pw[3 * i], pw[3 * i + 1], pw[3 * i + 2], planar_cloud[i].i});
            }
            rc = ivox.add_points(to_add.data(), to_add.size());
            if (rc != FLS_OK) return rc;
            rc = ivox.add_points(no_downsample.data(), no_downsample.size());
            if (rc != FLS_OK) return rc;
        }
        settle_mirror();
        if (p.is_localization_mode) {  // :134-138 kd-tree for GetFitnessScore
            const auto tf0 = std::chrono::steady_clock::now();
            rc = fitness_grid.build(planar_cloud, 1.0f, stream);
            have_fitness_grid = (rc == FLS_OK);
            if (host_timing)
                std::fprintf(stderr, "[fls host] host fitness grid %.3f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf0).count());
        }
        return rc;
    }

    // fls_match from host buffers: the scan stays in the pinned staging buffer; the first iteration's correspondence launch reads it
    // from there over PCIe (the kernel is latency bound: the reads hide behind its probe / candidate chains) and leaves the device copy
    // the later launches use.  No SDMA copy, no copy-engine -> compute-queue hand-off in front of the first kernel (8 us + 8 us for the
    // 10 k-point planar cloud the pipeline feeds).
    bool scan_in_staging = false;
    fls_status scan_upload_for_match(const float* s0, size_t n0, const float* s1, size_t n1, int stride) override {
        if (borrowed) return scan_upload(s0, n0, s1, n1, stride);
        (void)s1; (void)n1;
        scan.stage_raw(s0, n0, stride);
        scan_in_staging = n0 != 0;
        if (scan_in_staging) scan.reserve_device();
        return FLS_OK;
    }
    fls_status scan_upload(const float* s0, size_t n0, const float* s1, size_t n1, int stride) override {
        scan_in_staging = false;
        (void)s1; (void)n1;
        // (the pinned staging buffer is free again: fls_scan_upload synchronises, a Match ends after its copies)
        scan.upload_raw(s0, n0, stride, stream);
        return FLS_OK;
    }
    fls_status scan_attach_device(const HandoffCloud& c) override {
        scan_in_staging = false;
        scan.attach_device(c, stream, /*want_host=*/false);  // (scan.host stays empty, as after upload_raw)
        return FLS_OK;
    }

    // the map as the iteration launches get it, with the two predicates of its own that select the kNN kernel's form.  dense: the brick
    // window instead of the hash table.  general (GEN): only where it can matter -- voxels so large that a candidate of the 19 probed voxels
    // could lie beyond max_range (3 res per axis, one voxel more than the geometry allows, reaches 5 m), or a point array of 4 GiB and more
    struct MapView { DevGrid g; BrickDir win; float inv_resolution; unsigned pts_cap /* slot bound: the allocation */; bool dense, general; };
    MapView map_view() const {
        const IvoxMap& r = read_map();
        const DevGrid g = r.image.dev();
        const BrickDir win = r.use_dense ? r.image.bricks() : BrickDir{nullptr, 0u, nullptr, 0u};
        return MapView{g, win, r.ivox.inv_resolution, unsigned(r.image.d_pts.cap), win.cells != nullptr,
                       !(27.0f * r.ivox.resolution * r.ivox.resolution < 25.0f) || size_t(g.n_pts) > (size_t(1) << 28)};
    }

    // One Match in three parts -- prepare (checks, buffers, nn_prev, the grids, the initial pose), launch (the iteration launches and the wait for the
    // mailbox), finish (the epilogue) -- so that a group of batch jobs can share the middle part (match_batch_shared_ivox) around the same prepare and finish.
    struct MatchPlan {
        bool go = false;      // false: prepare has answered the call (an error, or the empty scan)
        size_t n = 0;
        int fit_threads = 256, nwg = 0;
        unsigned knn_blocks = 0;  // workgroups of the kNN grid: a multiple of 8 * kIvoxXcdChunk, so that the XCD re-map is a bijection
        MapView v{};
        Pose16 T0{};
        bool spec = false;    // the speculative map-update chain rides behind the iteration chunks (single-job launch only)
    };
    static unsigned knn_grid_blocks(const size_t n) {
        const size_t nblk = (n + 63) / 64, gran = size_t(8) * size_t(kIvoxXcdChunk);
        return unsigned((nblk + gran - 1) / gran * gran);
    }
    fls_status match_prepare(double* T, int update_map, fls_stats* out, MatchPlan& m) {
        m.go = false;
        if (map.is_replica() && update_map) return FLS_ERR_STATE;  // (a replica's image has no AddPoints side and no mirror)
        const size_t n = scan.n;
        number_planar_point = n;
        stats = fls_stats{};
        stats.n_source = int(n);
        std::memcpy(T_, T, sizeof(T_));
        if (n == 0) {
            // empty planar cloud: H = g = 0 -> dx = 0 -> stop rule fires in iteration 0, n_valid = 0 < 50 -> false (:201-203)
            stats.iterations = 1; stats.converged = 0;
            if (out) *out = stats;
            // the iteration log of that one iteration (fls_get_iteration_log; the oracle keeps the same row): the input pose, no valid point, no residual
            log_n = 0; log_stale = false;
            if (h_state.p) {
                std::memcpy(h_state.p->log_T[0], T, sizeof(double) * 16);
                h_state.p->log_nv[0] = 0; h_state.p->log_res[0] = 0.0; h_state.p->iter = 1;
                log_n = 1;
            }
            return FLS_NOT_CONVERGED;
        }
        if (!borrowed) map.refresh();
        // nearest_points_.resize(n) semantics (:257): grown tail is empty, shrink forgets
        d_nn.reserve(n * 5, /*keep=*/true, stream);
        d_nn_cnt.reserve(n, /*keep=*/true, stream);
        d_nn_ids.reserve(n * 8, /*keep=*/true, stream);
        nn_prev = int(std::min(nn_n, n));  // the first iteration's kNN launch clears the counts of the grown tail [nn_prev, n)
        nn_n = n;
        d_J.reserve(7 * n);
        d_flag.reserve(n);  // cleared by the first iteration's kNN kernel (std::fill(flags, false) once per Match, :156, Q1)
        // workgroup size of the fit kernel: 512 threads (two waves per SIMD of a CU) when the scan fills the machine anyway; 256 (one wave per
        // SIMD) up to 65,536 points, where 256 workgroups spread the same waves over every CU -- the 9.8k-point planar cloud the pipeline feeds
        // ran its 2,500-instruction fit phase two waves deep on 20 CUs with 236 CUs idle
        m.n = n;
        m.fit_threads = n <= 65536 ? 256 : kFitThreads;
        m.nwg = int((n + size_t(m.fit_threads) - 1) / size_t(m.fit_threads));
        m.knn_blocks = knn_grid_blocks(n);
        d_partials_b.reserve(size_t(m.nwg) * kPartialStride);
        m.v = map_view();
        std::memcpy(m.T0.m, T, sizeof(m.T0.m));
        // speculative map update (see spec_pending): only where the short chain applies and the call would update the map if it converges
        m.spec = update_map && !p.is_localization_mode && !borrowed && !map.is_first && map.short_chain_applies(n);
        spec_pending = false;
        m.go = true;
        return FLS_OK;
    }
    void launch_knn_reforder(const MatchPlan& m, bool first, const float* src_x, const float* src_y, const float* src_z, float* dev_copy, hipEvent_t e0,
                             hipEvent_t e1);  // kernels_ivox_knn_reforder.hpp
    unsigned match_launch(const MatchPlan& m) {
        const size_t n = m.n;
        auto after_chunk = [&](int) {
            if (!m.spec) return;
            if (spec_pending) ++map.n_speculative_skipped;  // (the chain behind the previous chunk found the Match unfinished)
            const bool counted = launch_decide(n, /*speculative=*/true);
            spec_pending = counted && map.enqueue_update(d_code.p, d_pw.p, n, counted);
            ++map.n_speculative;
        };
        return run_mailbox_loop(int(p.max_iterations), n, [&](int it, int first) {
            // e0 / e1 (profiling only): start / stop events attached to the kernel's own dispatch packet (hipExtLaunchKernelGGL),
            // i.e. the kernel's execution time as a kernel trace sees it -- a hipEventRecord bracket also times the dispatch of
            // the kernel between its two marker packets (about 3 us more on an 18 us kernel)
            const hipEvent_t e0 = profiling ? ev[2 * it] : nullptr, e1 = profiling ? ev[2 * it + 1] : nullptr;
            // first launch of a Match whose scan is still in the staging buffer: read it there, write the device copy
            const bool from_host = first && scan_in_staging;
            const float* const hx = from_host ? scan.stage_dev() : nullptr;
            const float* const src_x = from_host ? hx : (const float*)scan.x.p;
            const float* const src_y = from_host ? hx + n : (const float*)scan.y.p;
            const float* const src_z = from_host ? hx + 2 * n : (const float*)scan.z.p;
            float* const dev_copy = from_host ? scan.xyz.p : nullptr;
            if (knn_reference) launch_knn_reforder(m, first != 0, src_x, src_y, src_z, dev_copy, e0, e1);
            else with_bools([&](auto COUNT, auto DENSE, auto FIRST, auto GEN) {  // (4 lanes per query: 64 queries per 256-thread workgroup)
                hipExtLaunchKernelGGL((ivox_knn_kernel<COUNT.value, DENSE.value, FIRST.value, GEN.value>), dim3(m.knn_blocks), dim3(256), 0, stream, e0, e1, 0,
                                      src_x, src_y, src_z, int(n), (const GnState*)d_state.p, m.T0, m.v.g, m.v.win, m.v.inv_resolution, d_nn.p, d_nn_cnt.p,
                                      d_flag.p, d_tc.p, kIvoxXcdChunk, d_nn_ids.p, nn_prev, dev_copy);
            }, count_traffic, m.v.dense, first != 0, m.v.general);
            with_bools([&](auto FIRST, auto SMALL) {
                constexpr int NT = SMALL.value ? 256 : kFitThreads;
                hipExtLaunchKernelGGL((p2plane_fit_solve_kernel<FIRST.value, NT>), dim3(m.nwg), dim3(NT), 0, stream, nullptr, nullptr, 0, scan.x.p, scan.y.p, scan.z.p,
                                      int(n), d_state.p, m.T0, (const float4*)d_nn.p, (const unsigned char*)d_nn_cnt.p, d_J.p, d_flag.p, d_partials_b.p, d_ticket.p,
                                      mb_dev, launch_word(), p.point_to_planar_thres, p.rotation_converge_thres, p.position_converge_thres, kTicketShards,
                                      (const unsigned*)d_nn_ids.p, (const float4*)m.v.g.pts, m.v.pts_cap);
            }, first != 0, m.fit_threads == 256);
        }, after_chunk);
    }
    fls_status match_finish(double* T, unsigned word, int update_map, fls_stats* out) {
        scan_in_staging = false;  // (the first launch left the device copy)
        nn_rows_current = false;  // the lists of every point with candidates are slots of the current image now
        if (knn_reference) {
            unsigned long long fb = 0;
            FLS_HIP(hipMemcpyAsync(&fb, d_ref_fallbacks.p, sizeof(fb), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            n_ref_fallbacks = size_t(fb);
        }
        const Mailbox& mb = take_result(word);
        std::memcpy(T, mb.T, sizeof(double) * 16);
        std::memcpy(T_, mb.T, sizeof(T_));
        std::memcpy(final_T, mb.T, sizeof(final_T));
        have_final = true;
        bool has_converge = true;
        if (mb.n_valid < 50) has_converge = false;  // :201-203
        stats.converged = has_converge ? 1 : 0;
        fls_status rc = has_converge ? FLS_OK : FLS_NOT_CONVERGED;
        if (has_converge && !p.is_localization_mode && update_map && !borrowed) {  // :205-206
            if (spec_pending) nn_rows_current = true;  // (the speculative decision launch turned the lists into rows)
            const fls_status arc = add_cloud_impl(scan.host, /*from_resident_scan=*/true, /*pre_enqueued=*/spec_pending);
            if (arc != FLS_OK) rc = arc; else stats.map_updated = 1;
        } else if (spec_pending) {
            ++map.n_speculative_skipped;  // not converged: the chain skipped itself on the device (n_valid < 50), nothing to collect
        }
        spec_pending = false;
        if (out) *out = stats;
        return rc;
    }
    fls_status match_resident(double* T, int update_map, fls_stats* out) override {
        MatchPlan m;
        const fls_status prc = match_prepare(T, update_map, out, m);
        if (!m.go) return prc;
        return match_finish(T, match_launch(m), update_map, out);
    }

    // ---- fls_match_batch_shared_ivox (include/fls_batch_ivox.h): groups of up to n_slots jobs share the two launches of an iteration ----
    // The group driver is the base's (matcher_base.hpp::run_job_groups).  Slots are the lane clones (they read this handle's map and upload with
    // scan_upload, never from the staging buffer).  The job table holds the jobs of the 256-thread fit class first, then those of the 512-thread
    // class: the kNN launch takes the whole table, each fit launch its class's part (a class keeps the workgroup size the single-job path gives its
    // jobs, because another size regroups the wave sums) -- one fit launch per iteration for a group of one class, two for a mixed one.
    PinnedBuf<IvoxJob> h_jobs;
    DevBuf<IvoxJob> d_jobs;
    fls_status match_batch_shared_ivox(size_t n_jobs, const float* const* s0, const size_t* n0, const float* const*, const size_t*, int stride, double* T,
                                       fls_stats* st, int32_t* status, int n_slots) override {
        // (the shared launches are the default order's: a reference-order handle runs the jobs on its lanes, as a kind without a shared form does)
        if (knn_reference) return fls_matcher::match_batch_shared_ivox(n_jobs, s0, n0, nullptr, nullptr, stride, T, st, status, n_slots);
        std::vector<MatchPlan> plan(size_t(2) * kMaxLanes);  // per slot
        size_t n_class[2] = {0, 0};                           // jobs of the 256- / 512-thread fit class in the current group
        unsigned knn_rows_max = 0, fit_rows_max[2] = {0, 0};
        auto stats_of = [&](const size_t j) { return st ? &st[j] : nullptr; };
        MapView v{};  // the group's one map: this handle's (read once the driver's prepare_batch has made it current)
        // an empty scan is answered on the host, as the single-job path answers it
        auto prepare = [&](P2PlaneIvoxMatcher* q, const size_t s, const size_t j, bool& shared) -> fls_status {
            fls_status rc = q->scan_upload(s0[j], n0[j], nullptr, 0, stride);
            if (rc != FLS_OK) return rc;
            rc = q->match_prepare(T + 16 * j, 0, stats_of(j), plan[s]);
            shared = plan[s].go;
            return rc;
        };
        auto table = [&](GroupCall<P2PlaneIvoxMatcher>& c) {
            const size_t A = c.act.size();
            if (!h_jobs.p) { h_jobs.reserve(kMaxLanes); d_jobs.reserve(kMaxLanes); }
            v = map_view();
            n_class[0] = n_class[1] = 0;
            knn_rows_max = fit_rows_max[0] = fit_rows_max[1] = 0;
            for (size_t i = 0; i < A; ++i) ++n_class[plan[c.act_slot[i]].fit_threads == 256 ? 0 : 1];
            size_t at[2] = {0, n_class[0]};
            for (size_t i = 0; i < A; ++i) {
                P2PlaneIvoxMatcher* q = c.act[i];
                const MatchPlan& m = plan[c.act_slot[i]];
                const int k = m.fit_threads == 256 ? 0 : 1;
                IvoxJob& e = h_jobs.p[at[k]++];
                e.sx = q->scan.x.p; e.sy = q->scan.y.p; e.sz = q->scan.z.p;
                e.n = int(m.n); e.knn_blocks = int(m.knn_blocks); e.nwg = m.nwg; e.nn_prev = q->nn_prev;
                e.st = q->d_state.p; e.nn_pts = q->d_nn.p; e.nn_cnt = q->d_nn_cnt.p; e.flag = q->d_flag.p; e.nn_ids = q->d_nn_ids.p;
                e.Jst = q->d_J.p; e.partials = q->d_partials_b.p; e.ticket = q->d_ticket.p;
                e.mb = q->mb_dev; e.launch_word = q->launch_word(); e.pad = 0u;
                e.T0 = m.T0;
                knn_rows_max = std::max(knn_rows_max, m.knn_blocks);
                fit_rows_max[k] = std::max(fit_rows_max[k], unsigned(m.nwg));
            }
            // (the pinned table is free: every launch that could read the device copy of the previous group's has been waited for or exits at once,
            // and the copy below is ordered behind them on the batch stream)
            FLS_HIP(hipMemcpyAsync(d_jobs.p, h_jobs.p, A * sizeof(IvoxJob), hipMemcpyHostToDevice, batch_stream));
        };
        auto queue = [&](GroupCall<P2PlaneIvoxMatcher>& c, const int first) {
            with_bools([&](auto DENSE, auto FIRST, auto GEN) {
                hipLaunchKernelGGL((ivox_knn_jobs_kernel<DENSE.value, FIRST.value, GEN.value>), dim3(knn_rows_max, unsigned(c.act.size())), dim3(256), 0, batch_stream,
                                   (const IvoxJob*)d_jobs.p, v.g, v.win, v.inv_resolution, kIvoxXcdChunk);
            }, v.dense, first != 0, v.general);
            ++batch_ivox_counters[0];
            for (int k = 0; k < 2; ++k) {  // the 256-thread class, then the 512-thread class behind it in the table
                if (!n_class[k]) continue;
                with_bools([&](auto FIRST, auto SMALL) {
                    constexpr int NT = SMALL.value ? 256 : kFitThreads;
                    hipLaunchKernelGGL((p2plane_fit_solve_jobs_kernel<FIRST.value, NT>), dim3(fit_rows_max[k], unsigned(n_class[k])), dim3(NT), 0, batch_stream,
                                       (const IvoxJob*)(d_jobs.p + (k ? n_class[0] : 0)), p.point_to_planar_thres, p.rotation_converge_thres,
                                       p.position_converge_thres, kTicketShards, (const float4*)v.g.pts, v.pts_cap);
                }, first != 0, k == 0);
                ++batch_ivox_counters[1];
            }
        };
        auto finish = [&](P2PlaneIvoxMatcher* q, const size_t j, const unsigned word) -> fls_status {
            q->end_match(word, q->scan.n);
            return q->match_finish(T + 16 * j, word, 0, stats_of(j));
        };
        return run_job_groups<P2PlaneIvoxMatcher>(n_jobs, s0, n0, stride, T, st, status, n_slots,
                                                  GroupCounters{&batch_ivox_counters[2], &batch_ivox_counters[3], &batch_ivox_counters[4]}, prepare, table, queue, finish);
    }

    // ---- moving maps (fls_reg.h): the bodies are IvoxMap's; a lane has no map of its own to move, a replica no mirror to export ----
    size_t map_export(void* blob, size_t cap) override { return borrowed || map.is_replica() ? 0 : map.export_blob(blob, cap); }
    fls_status map_replaced(const fls_status rc) { if (rc == FLS_OK) reset_match_state(); return rc; }
    fls_status map_import(const void* blob, size_t n) override { return borrowed ? FLS_ERR_INVALID : map_replaced(map.import_blob(blob, n)); }
    // the same blob packed from / built into the device image (include/fls_map_ivox.h): a Match returns with its update chain collected, so
    // the image is settled; the map's own calls wait for the stream
    size_t ivox_blob_bytes() override { return borrowed || map.is_replica() ? 0 : map.blob_bytes(); }
    fls_status ivox_blob_export(void* dst, size_t cap, int on_device) override {
        return borrowed || map.is_replica() ? FLS_ERR_STATE : map.export_blob_to(dst, cap, on_device != 0);
    }
    fls_status ivox_blob_import(const void* src, size_t n, int on_device) override {
        return borrowed ? FLS_ERR_INVALID : map_replaced(map.import_blob_from(src, n, on_device != 0));
    }
    bool can_replicate() const override { return !borrowed; }
    fls_status replicate_from(fls_matcher& o) override {
        if (borrowed || o.kind != kind) return FLS_ERR_INVALID;
        auto& src = static_cast<P2PlaneIvoxMatcher&>(o);
        if (src.borrowed || src.map.is_replica() || src.map.ivox.resolution != map.ivox.resolution) return FLS_ERR_STATE;
        FLS_HIP(hipSetDevice(src.device));
        const fls_status prc = src.prepare_batch();  // image current, the owner's stream idle
        if (prc != FLS_OK) return prc;
        size_t nb = 0;
        const size_t used_now = src.map.live_counts(nb);
        FLS_HIP(hipSetDevice(device));
        map.replicate(src.map, used_now, nb, src.device, device);
        return map_replaced(FLS_OK);
    }
    size_t map_image_bytes() override { return borrowed || map.is_replica() || prepare_batch() != FLS_OK ? 0 : map.image_bytes(); }
    fls_status map_image_export(void* dst, size_t cap, int on_device) override {
        if (borrowed || map.is_replica() || !dst) return FLS_ERR_STATE;
        const fls_status prc = prepare_batch();  // image current, the stream idle
        return prc != FLS_OK ? prc : map.export_image(dst, cap, on_device != 0);
    }
    fls_status map_image_import(const void* src, size_t n, int on_device) override {
        return borrowed ? FLS_ERR_INVALID : map_replaced(map.import_image(src, n, on_device != 0));
    }

    std::unique_ptr<fls_matcher> clone_for_lane() override {
        auto q = make_lane(*this);
        if (q) q->borrowed = &map;
        return q;
    }
    fls_status prepare_batch() override {
        map.refresh();
        FLS_HIP(hipStreamSynchronize(stream));  // the image is complete before other streams read it
        return FLS_OK;
    }

    fls_status fitness(float max_range, float* score) override {
        if (!p.is_localization_mode) { *score = std::numeric_limits<float>::max(); return FLS_OK; }  // FloatNaN :226-228
        if (!have_fitness_grid || !have_final) return FLS_ERR_STATE;
        return fitness_score_device(*this, fitness_grid, scan, final_T, max_range, score);
    }

    int correspondences(int, int32_t* ids, uint8_t* cnt, uint8_t* valid, size_t cap) override {
        download_nn();
        const size_t n = std::min(cap, nn_n);
        h_flag.resize(nn_n);
        if (nn_n) {
            FLS_HIP(hipMemcpyAsync(h_flag.data(), d_flag.p, nn_n, hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
        }
        for (size_t i = 0; i < n; ++i) {
            cnt[i] = h_cnt[i];
            for (int j = 0; j < 5; ++j) ids[i * 5 + j] = j < h_cnt[i] ? h_nn[i * 5 + j].id : -1;
            valid[i] = h_flag[i];
        }
        return int(n);
    }
    size_t map_size(int slot) const override {
        if (slot == 177 || slot == 178) {  // reference-order kNN launches / queries that fell back to the default order: this handle's and its batch lanes'
            size_t v = slot == 177 ? n_ref_launches : n_ref_fallbacks;
            for (const auto& l : lanes) v += l->map_size(slot);
            return v;
        }
        return slot == 176 ? size_t(last_tc.shared) : map.counter(slot);  // (176: the last counting Match's kNN waves on the shared-run path)
    }
};

}  // namespace fls
