// matcher_ndt.hpp -- host side of FLS_INCREMENTAL_NDT, the replacement of IncrementalNDT
// (include/registration/incremental_ndt.h:16-383).
//   AddCloudToLocalMap :182-227  the two VoxelGrids and the fitness grid here; the voxel map itself -- insert with LRU eviction + UpdateVoxel
//                                (:130-179), on the device (kernels_ndt_update.hpp: a whole cloud through NdtMap::build, first-scan rule, later
//                                scans as incremental batches) and on the host for whatever the device declines (NdtMirror::insert) -- is
//                                ndt_map.hpp's NdtMap.  This file decides what goes into it.
//   Match              :229-337  device-resident loop: ndt_lanes_kernel (7-voxel Mahalanobis scoring,
//                                FP64, the Gauss-Newton tail in its last workgroup; mode 1).
//   the map as it travels        one flat image (include/fls_map_ndt.h): map_export / map_import, map_image_*, replicate_from -- forwarded to
//                                the map, which packs it from the device rows or from the mirror (ndt_image.hpp), the same bytes either way.
#pragma once
#include "matcher_base.hpp"
#include "ndt_map.hpp"
#include "fitness_host.hpp"

namespace fls {

struct NdtMatcher final : fls_matcher {
    NdtMap map;
    const NdtMatcher* owner = nullptr;
    const NdtMap& read_map() const { return owner ? owner->map : map; }  // a batch lane reads its owner's voxel tables

    DevScan scan;
    std::vector<PtI> source;
    SourceFilter src_filter;
    DevBuf<unsigned> d_ticket;
    DevBuf<int> d_hit_vid;
    DevBuf<unsigned char> d_eff7;
    double final_T[16]{};
    bool have_final = false;
    CellGridImage fitness_grid;
    bool have_fitness_grid = false;

    fls_status init() {
        if (unset_d(p.ndt_voxel_size) || unset_d(p.ndt_res_outlier_threshold) || unset_d(p.rotation_converge_thres) ||
            unset_d(p.position_converge_thres) || unset_f(p.source_cloud_filter_size) || p.ndt_min_points_in_voxel == 0x7fffffff ||
            p.ndt_max_points_in_voxel == 0x7fffffff || p.ndt_min_effective_pts == 0x7fffffff || p.ndt_capacity == 0x7fffffff)
            return FLS_ERR_INVALID;  // CHECK_NE block incremental_ndt.h:27-36
        if (!(p.ndt_voxel_size > 0.0) || !(p.source_cloud_filter_size > 0.f) || p.ndt_capacity <= 0) return FLS_ERR_INVALID;
        init_common();
        src_filter.init();
        init_tickets(d_ticket);
        map.init(stream, NdtImageParams{p.ndt_voxel_size, p.ndt_min_points_in_voxel, p.ndt_max_points_in_voxel, p.ndt_capacity}, p.is_localization_mode);
        return FLS_OK;
    }

    // opt-in device source filter (FLS_DEVICE_VOXELGRID=1): the filtered scan never left the device -- transform it, filter it
    // again (the reference's second VoxelGrid, :186) and update the map without touching the host.  false: not applied (the
    // caller takes the host path, which also reports a key out of range)
    DevBuf<float> w_cloud;
    DeviceVoxelGrid map_vg;
    unsigned long long resident_updates = 0;
    bool device_update_from_resident_source(const double* T_in) {
        const size_t n = src_filter.vg.n_out;
        if (n == 0) return false;
        const auto t0 = std::chrono::steady_clock::now();
        w_cloud.reserve(3 * n);
        XformF xf;
        for (int j = 0; j < 3; ++j) for (int i = 0; i < 3; ++i) xf.R[i + j * 3] = float(T_in[i + j * 4]);
        for (int i = 0; i < 3; ++i) xf.t[i] = float(T_in[12 + i]);
        hipLaunchKernelGGL(xform_cloud_f_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, stream, src_filter.vg.ox(), src_filter.vg.oy(), src_filter.vg.oz(),
                           int(n), xf, w_cloud.p, w_cloud.p + n, w_cloud.p + 2 * n);
        if (!map_vg.run(w_cloud.p, w_cloud.p + n, w_cloud.p + 2 * n, src_filter.vg.oi(), n, p.source_cloud_filter_size, stream)) return false;
        if (!map.device_add_cloud_dev(map_vg.ox(), map_vg.oy(), map_vg.oz(), map_vg.n_out)) {
            map.sync_host_from_device();
            return false;
        }
        ++resident_updates;
        if (map.host_timing)
            std::fprintf(stderr, "[fls_reg] ndt map update (device, resident source): %zu -> %zu pts | transform + VoxelGrid + UpdateVoxel x%u %.3f ms (%zu voxels)\n", n,
                         map_vg.n_out, map.last_touched, ndt_ms(t0, std::chrono::steady_clock::now()), map.dev_alive);
        return true;
    }

    // ---- the map built from a whole cloud on the device (NdtMap::build): the raw cloud goes up once, the device VoxelGrid filters it
    // (bit-identical to the host filter), the map takes the filter's output and, in localization mode, the fitness grid is built from the same
    // device cloud -- after the batch has been applied.  A decline leaves the handle as it was and the host path runs the call.
    DevScan build_raw;
    DeviceGridBuilder fitness_builder;
    std::vector<float> build_tmp;
    bool is_build_call() const { return !owner && map.wants_build(); }
    // true: applied (FLS_OK); false: declined, nothing changed
    bool add_cloud_build(const float* c0, const size_t n0, const int stride) {
        if (n0 == 0 || c0 == nullptr) return false;  // (counted nowhere)
        if (!map.build_admits(n0)) return false;
        const auto t0 = std::chrono::steady_clock::now();
        build_raw.upload_raw(c0, n0, stride, stream, true);
        return build_core(build_raw.x.p, build_raw.y.p, build_raw.z.p, build_raw.xyz.p + 3 * n0, n0, [&] { return cloud_from(c0, n0, stride); }, t0);
    }
    // the build itself, from the raw cloud's x | y | z | intensity on the device; host_cloud(): the same cloud on the host (a fitness-grid fallback)
    template <class HostCloud>
    bool build_core(const float* rx, const float* ry, const float* rz, const float* ri, const size_t n0, HostCloud&& host_cloud,
                    const std::chrono::steady_clock::time_point t0) {
        const float *fx = nullptr, *fy = nullptr, *fz = nullptr;  // the cloud the map takes, on the device
        size_t n = 0;
        if (map_vg.run(rx, ry, rz, ri, n0, p.source_cloud_filter_size, stream)) {
            fx = map_vg.ox(); fy = map_vg.oy(); fz = map_vg.oz();
            n = map_vg.n_out;
        } else {
            const unsigned vs = map_vg.vmb_host ? map_vg.vmb_host->status : unsigned(kVgOk);
            if (vs == kVgNoFinitePoint || vs == kVgNonFinitePoints) return map.decline_build(NdtMap::kWhyRange);
            if (vs != kVgLeafTooSmall) return map.decline_build(NdtMap::kWhyPoints);  // (the exact sort gave up)
            // PCL's "leaf size too small" (an extent of more than INT_MAX leaves, every point finite): the filter hands the cloud on as it came
            fx = rx; fy = ry; fz = rz;
            n = n0;
        }
        if (n == 0) return map.decline_build(NdtMap::kWhyPoints);
        const auto t1 = std::chrono::steady_clock::now();
        if (!map.build(fx, fy, fz, n)) return false;
        const auto t2 = std::chrono::steady_clock::now();
        if (p.is_localization_mode) {  // :188-190 kd-tree for GetFitnessScore, from the filtered cloud already on the device
            if (fitness_builder.run(fitness_grid, fx, fy, fz, n, 1.0f, 1, false, stream)) have_fitness_grid = true;
            else have_fitness_grid = fitness_grid.build(fx == rx ? host_cloud() : map_vg.download(stream, build_tmp), 1.0f, stream) == FLS_OK;
            FLS_HIP(hipStreamSynchronize(stream));
        }
        if (map.host_timing)
            std::fprintf(stderr, "[fls_reg] ndt map build (device): %zu -> %zu pts | upload + VoxelGrid %.3f ms | first-scan UpdateVoxel x%u %.3f ms | fitness grid %.3f ms (%zu voxels)\n",
                         n0, n, ndt_ms(t0, t1), map.last_touched, ndt_ms(t1, t2), ndt_ms(t2, std::chrono::steady_clock::now()), map.dev_alive);
        return true;
    }

    fls_status add_cloud_impl(const std::vector<PtI>& cloud_world_full) {  // :182-227
        const auto t0 = std::chrono::steady_clock::now();
        const std::vector<PtI> cloud_world = voxel_grid(cloud_world_full, p.source_cloud_filter_size);
        const auto t1 = std::chrono::steady_clock::now();
        if (!map.in_key_range(cloud_world)) return FLS_ERR_RANGE;  // range check first (all-or-nothing)
        if (p.is_localization_mode) { have_fitness_grid = fitness_grid.build(cloud_world, 1.0f, stream) == FLS_OK; }
        map.add_cloud(cloud_world, cloud_world_full.size(), t0, t1);
        return FLS_OK;
    }
    fls_status add_cloud(const float* c0, size_t n0, const float* c1, size_t n1, int stride) override {
        if (c1 != nullptr && n1 != 0) return FLS_ERR_INVALID;
        if (is_build_call() && add_cloud_build(c0, n0, stride)) return FLS_OK;  // the cloud goes in whole
        return add_cloud_impl(cloud_from(c0, n0, stride));
    }
    // add_cloud from a cloud on the device: the same decisions, the build reads the planes where they lie
    fls_status add_cloud_device(const HandoffCloud& c, const HostRows& rows, bool* took_planes) override {
        *took_planes = false;
        if (is_build_call() && c.n != 0 && map.build_admits(c.n) && build_core(c.x, c.y, c.z, c.in, c.n, rows, std::chrono::steady_clock::now())) {
            *took_planes = true;
            return FLS_OK;
        }
        return add_cloud_impl(rows());
    }
    fls_status scan_upload(const float* s0, size_t n0, const float*, size_t, int stride) override {
        src_filter.filter(s0, n0, stride, p.source_cloud_filter_size, stream, scan, source);  // :232
        return FLS_OK;
    }
    fls_status scan_upload_raw(const float* s0, size_t n0, const float*, size_t, int stride) override {
        src_filter.upload_raw_only(s0, n0, stride, p.source_cloud_filter_size, stream, scan, source);  // (no filtered scan is resident until the next Match: fitness answers FLS_ERR_STATE)
        return FLS_OK;
    }
    fls_status scan_attach_device(const HandoffCloud& c) override {
        src_filter.attach_raw_only(c, p.source_cloud_filter_size, stream, scan, source);
        return FLS_OK;
    }
    fls_status match_resident(double* T, int update_map, fls_stats* out) override {
        const NdtMap& M = read_map();
        if (M.alive() == 0 || !M.has_image()) return FLS_ERR_STATE;  // CHECK(!grids_.empty()) :230
        if (src_filter.raw_pending) src_filter.refilter(stream, scan, source);  // :231-232, on the resident raw scan
        const size_t n = scan.n;
        const int nblk = int((n + 63) / 64);
        stats = fls_stats{};
        stats.n_source = int(n);
        double T_in[16];
        std::memcpy(T_in, T, sizeof(T_in));
        d_hit_vid.reserve(std::max<size_t>(n * 7, 1));
        d_eff7.reserve(std::max<size_t>(n * 7, 1));
        d_partials_b.reserve(size_t(std::max(nblk, 1)) * kPartialStride);
        const NdtGridDev ng = M.grid();
        Pose16 T0;
        std::memcpy(T0.m, T, sizeof(T0.m));
        const unsigned word = run_mailbox_loop(int(p.max_iterations), n, [&](int it, int first) {
            if (profiling) FLS_HIP(hipEventRecord(ev[2 * it], stream));
            if (nblk > 0 && !count_traffic) {
                // one lane per neighbour voxel (64 points per workgroup: same row count) and the Gauss-Newton tail in the last workgroup: one launch
                // per iteration.  Rounds 3-5 measured the fused tail SLOWER on configs[2] (83.9 vs 76-80 us per Match): the kernel held the pose
                // (sixteen doubles) in registers across the per-point part for the tail -- 144 VGPRs = 3 waves per SIMD = ONE 512-thread workgroup per
                // CU, so its 457 workgroups ran in two rounds.  Round 6 parks the pose in LDS: 118 VGPRs like the plain kernel, one round, and the
                // launch the tail no longer needs is a gain: 73.5-74.1 vs 78.3-79.6 us per Match, same pose to the last bit (profiles/r06_ai_*).
                const LuTailArgs tail{1, p.rotation_converge_thres, p.position_converge_thres, p.ndt_min_effective_pts, mb_dev, launch_word()};
                hipLaunchKernelGGL(ndt_lanes_kernel<true>, dim3(nblk), dim3(kNdtLanesBlock), 0, stream, scan.x.p, scan.y.p, scan.z.p, int(n), d_state.p, first,
                                   T0, ng, p.ndt_res_outlier_threshold, d_hit_vid.p, d_eff7.p, d_partials_b.p, d_ticket.p, kTicketShards, tail);
                if (profiling) FLS_HIP(hipEventRecord(ev[2 * it + 1], stream));
                return;
            }
            if (nblk > 0)  // traffic counting: one lane per point, then the tail as its own launch
                hipLaunchKernelGGL(ndt_kernel<true>, dim3(nblk), dim3(64), 0, stream, scan.x.p, scan.y.p, scan.z.p, int(n), d_state.p, first, T0, ng,
                                   p.ndt_res_outlier_threshold, d_hit_vid.p, d_eff7.p, d_partials_b.p, d_tc.p);
            if (profiling) FLS_HIP(hipEventRecord(ev[2 * it + 1], stream));
            hipLaunchKernelGGL(gn_solve_lu_kernel, dim3(1), dim3(kSolveThreads), 0, stream, d_state.p, first, T0, (const double*)d_partials_b.p, nblk, 1,
                               p.rotation_converge_thres, p.position_converge_thres, p.ndt_min_effective_pts, mb_dev, launch_word());
        });
        const Mailbox& s = take_result(word);
        // the min_effective early-out sets done with converged == 0 on the device (:306-309: T = pose; return false)
        const bool early_fail = s.done && !s.converged && s.n_valid < p.ndt_min_effective_pts;
        if (early_fail) {
            std::memcpy(T, s.T, sizeof(double) * 16);
            stats.converged = 0;
            if (out) *out = stats;
            return FLS_NOT_CONVERGED;
        }
        // has_converge = true unconditionally (:325, Q10)
        fls_status rc = FLS_OK;
        if (!p.is_localization_mode && update_map && !owner) {
            // Q11: the cloud is transformed with the INPUT T (:327-329)
            if (map.on_device() && !map.mirror.flag_first_scan && src_filter.resident && device_update_from_resident_source(T_in)) {
                stats.map_updated = 1;
            } else {
                src_filter.materialize(stream, source);
                const fls_status arc = add_cloud_impl(hm::xform_cloud_f(source, T_in));
                if (arc != FLS_OK) rc = arc; else stats.map_updated = 1;
            }
        }
        std::memcpy(T, s.T, sizeof(double) * 16);
        std::memcpy(final_T, s.T, sizeof(final_T));
        have_final = true;
        stats.converged = 1;
        if (out) *out = stats;
        return rc;
    }
    std::unique_ptr<fls_matcher> clone_for_lane() override {
        auto q = make_owned_lane(*this);
        if (q) q->map.allow_device_update = q->map.allow_device_build = false;  // a batch lane has no map of its own: nothing of it goes to the device
        return q;
    }
    fls_status prepare_batch() override { FLS_HIP(hipStreamSynchronize(stream)); return map.has_image() ? FLS_OK : FLS_ERR_STATE; }
    fls_status fitness(float max_range, float* score) override {
        if (!p.is_localization_mode) { *score = std::numeric_limits<float>::max(); return FLS_OK; }  // :346-348
        if (!have_fitness_grid || src_filter.withdrawn) return FLS_ERR_STATE;
        // A Match that stops at the effective-point floor returns before `final_transformation_ = T` (incremental_ndt.h:306-309 vs :335): the score is then
        // taken with the PREVIOUS Match's transformation and the new source cloud -- and, when no Match of this matcher has got that far yet, with
        // the value-initialised member `final_transformation_{}` (:395), the zero matrix in the compiled reference: every point lands on the origin.
        // Found by running the localization-mode random scenarios on the GPU (round 6, `lfuzz3`: FLS_ERR_STATE where the reference answers).
        static const double zero_T[16] = {0.0};
        return fitness_score_device(*this, fitness_grid, scan, have_final ? final_T : zero_T, max_range, score);
    }
    int correspondences(int, int32_t* ids, uint8_t* cnt, uint8_t* valid, size_t cap) override {
        const size_t n = std::min(cap, scan.n);
        if (!n) return 0;
        std::vector<unsigned char> ef(n * 7);
        FLS_HIP(hipMemcpyAsync(ids, d_hit_vid.p, n * 7 * sizeof(int), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipMemcpyAsync(ef.data(), d_eff7.p, n * 7, hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        for (size_t i = 0; i < n; ++i) {
            int c = 0;
            for (int k = 0; k < 7; ++k) c += ef[i * 7 + k];
            cnt[i] = uint8_t(c);
            valid[i] = c > 0;
        }
        return int(n);
    }
    // ---- the map as one flat image (NdtMap::image_*): a batch lane has no map of its own
    size_t map_image_bytes() override { return owner ? 0 : map.image_bytes(); }
    fls_status map_image_export(void* dst, size_t cap, int dst_on_device) override { return owner ? FLS_ERR_STATE : map.image_export(dst, cap, dst_on_device); }
    size_t map_export(void* blob, size_t cap) override {
        const size_t need = map_image_bytes();
        if (need && blob && cap >= need && map_image_export(blob, cap, 0) != FLS_OK) return 0;
        return need;
    }
    // what an import leaves of the Match before it (as a replaced iVox map does)
    void map_replaced() {
        have_final = false; log_n = 0; log_stale = false;
        have_fitness_grid = false;  // not in the image: the next AddCloudToLocalMap of a localization handle builds it
    }
    fls_status map_image_import(const void* src, size_t n_bytes, int src_on_device) override {
        if (owner || !src) return FLS_ERR_INVALID;
        return map.image_import(src, n_bytes, src_on_device, [this] { map_replaced(); });
    }
    fls_status map_import(const void* blob, size_t n) override { return map_image_import(blob, n, 0); }
    // replica sets: the owner's image, exported on its device, copied device to device and imported on this handle's device.  The replica is an
    // ordinary handle holding the owner's map.
    bool can_replicate() const override { return !owner && map.image_fits(); }
    fls_status replicate_from(fls_matcher& o) override {
        if (o.kind != kind || owner) return FLS_ERR_STATE;
        NdtMatcher& src = static_cast<NdtMatcher&>(o);
        FLS_HIP(hipSetDevice(src.device));
        const fls_status prc = src.prepare_batch();  // image current, stream idle
        if (prc != FLS_OK) return prc;
        const size_t nbytes = src.map_image_bytes();
        if (!nbytes) return FLS_ERR_STATE;
        DevBuf<unsigned char>& out = src.map.replica_out;  // (kept by the owner: a refresh allocates nothing)
        out.reserve(nbytes);
        const fls_status erc = src.map_image_export(out.p, nbytes, 1);
        if (erc != FLS_OK) return erc;
        FLS_HIP(hipSetDevice(device));
        if (src.device == device) return map_image_import(out.p, nbytes, 1);
        map.replica_in.reserve(nbytes);
        FLS_HIP(hipMemcpyPeer(map.replica_in.p, device, out.p, src.device, nbytes));
        return map_image_import(map.replica_in.p, nbytes, 1);
    }
    size_t map_size(int slot) const override {
        if (slot == 105) return size_t(src_filter.device_runs);
        if (slot == 106) return size_t(src_filter.host_runs);
        if (slot == 111) return size_t(resident_updates);  // map updates fed by the device-resident filtered scan
        const bool counted = (slot >= 107 && slot <= 113) || slot == 117 || slot == 118 || slot == 126 || (slot >= 150 && slot <= 159);
        return counted ? map.counter(slot) : map.alive();
    }
};

}  // namespace fls
