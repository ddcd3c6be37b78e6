// matchers_kd.hpp -- host side of the three kinds whose reference uses pcl::KdTreeFLANN:
//   IcpMatcher       <- IcpOptimized<double>            include/registration/icp_optimized.h
//   LoamFullMatcher  <- LoamFull<double>                include/registration/loam_full_kdtree.h
//   P2PlaneKdMatcher <- LoamPointToPlaneKdtree<double>  include/registration/loam_point_to_plane_kdtree.h
// Map bookkeeping follows the reference's AddCloudToLocalMap (deque of clouds, VoxelGrid, rebuild): the handle's KdMaps (kd_map.hpp), one
// KdLocalMap per map, two for LoamFull; the kd-tree is replaced by an exact-kNN cell grid rebuilt at the same moments.  This file keeps the
// matchers: init checks, scan upload / attach, Match, fitness, correspondences, batch.
#pragma once
#include "matcher_base.hpp"
#include "host_math.hpp"
#include "device_voxelgrid.hpp"
#include "kernels_knn.hpp"
#include "kernels_grid_coop.hpp"
#include "fitness_host.hpp"
#include "kd_map.hpp"

namespace fls {

// LOAM feature maps: cells of half the gate radius, 5x5x5 block searched in two stages (kernels_grid_coop.hpp): the inner
// 27 cells hold 4-8x fewer candidates than 27 gate-sized cells and finish almost every query (-10 % kernel time; the
// kernel is bound by the 27 hash probes, not by the candidates)
constexpr int kGridRings = 2;
inline float cell_for_gate(double gate_sq) {  // smallest safe cell for a squared-distance gate
    return float(std::sqrt(gate_sq) * 1.0001);
}
// workgroups of a search launch (eight lanes per query) over n queries: a multiple of 64, so that the kernels' XCD chunk re-map is a bijection
inline unsigned knn_grid_blocks(size_t n) { return unsigned((((n * 8 + 255) / 256) + 63) / 64 * 64); }

// ---------------------------------------------------------------------------------------------
// What the three kinds share: the maps, a batch lane's view of its owner's, AddCloudToLocalMap, the image and replica calls, and the
// keyframe update that ends a Match.  A kind supplies the scan(s) of that keyframe: on the device where they lie there, else on the host.
struct KdMatcher : fls_matcher {
    KdMaps maps;
    const KdMatcher* owner = nullptr;  // batch lane: reads the owner's map grid(s)
    double final_T[16]{};              // the last Match's pose (Icp, P2PlaneKd: what the fitness score is taken at; LoamFull keeps none)
    bool have_final = false;
    bool xform_double = false;         // a keyframe is moved as hm::xform_cloud_d does (LoamFull); false: hm::xform_cloud_f's casts

    const KdMaps& read_maps() const { return owner ? owner->maps : maps; }
    bool map_ready() const { return owner ? owner->have_map : have_map; }
    // src[m] for map m: the scan(s) the Match just used, still on the device, with their intensities.  false: not there -- nothing has changed
    virtual bool keyframe_device(DeviceCloudRing::DeviceCloud* src) = 0;
    virtual void keyframe_host(const std::vector<PtI>** clouds) = 0;  // the same on the host, fetched only here

    fls_status add_cloud(const float* c0, size_t n0, const float* c1, size_t n1, int stride) override {
        // one map: no second cloud; LoamFull: CHECK_EQ(cloud_list.size(), 2) loam_full_kdtree.h:66
        if (maps.n_maps == 1 ? (c1 != nullptr && n1 != 0) : (c1 == nullptr && n1 != 0)) return FLS_ERR_INVALID;
        const std::vector<PtI> clouds[2] = {cloud_from(c0, n0, stride), maps.n_maps > 1 && c1 ? cloud_from(c1, n1, stride) : std::vector<PtI>()};
        return maps.add_host(clouds, have_map);
    }
    // The end of a Match.  icp_optimized.h:153 `has_converge_ && IsNeedAddCloud(T) && !is_localization_mode_` (loam_point_to_plane_kdtree.h:145-149;
    // loam_full_kdtree.h:185-193 has no mode term): the gate (and its last_T) is evaluated before the mode switch, as in the reference;
    // update_map == 0 (this ABI's "registration only" switch) skips the whole statement, so such a call leaves the keyframe gate alone.
    // The keyframe is the mapping branch of AddCloudToLocalMap: pushed on the device (every map's cloud in one launch), else through the host.
    fls_status finish_match(const double* T, const bool has_converge, const int update_map, fls_stats* out) {
        stats.converged = has_converge ? 1 : 0;
        fls_status rc = has_converge ? FLS_OK : FLS_NOT_CONVERGED;
        if (update_map && !owner && has_converge && maps.gate.need(T, p.dist_thre_add_cloud, p.rot_thre_add_cloud) && !maps.localization) {
            fls_status arc;
            DeviceCloudRing::DeviceCloud src[2];
            if (!(maps.can_push_device() && keyframe_device(src) &&
                  maps.push_keyframe_device(src, xform_double ? kd_push_xform_d(T) : kd_push_xform_f(T), have_map, arc))) {
                const std::vector<PtI>* at_sensor[2] = {nullptr, nullptr};
                keyframe_host(at_sensor);
                std::vector<PtI> clouds[2];
                for (int m = 0; m < maps.n_maps; ++m) clouds[m] = xform_double ? hm::xform_cloud_d(*at_sensor[m], T) : hm::xform_cloud_f(*at_sensor[m], T);
                arc = maps.add_host(clouds, have_map);
            }
            if (arc != FLS_OK) rc = arc; else stats.map_updated = 1;
        }
        if (out) *out = stats;
        return rc;
    }
    void reset_job_state() override { maps.gate = hm::KeyframeGate(); have_final = false; }  // function-static last_T of a fresh process (Q12)
    // ---- the map(s) as one flat image (KdMaps::image_*): a batch lane has no map of its own ----
    void map_replaced() { have_final = false; log_n = 0; log_stale = false; }  // fls_get_fitness_score answers FLS_ERR_STATE until the next Match
    size_t map_image_bytes() override { return owner ? 0 : maps.image_bytes(); }
    fls_status map_image_export(void* dst, size_t cap, int on_device) override { return owner ? FLS_ERR_STATE : maps.image_export(dst, cap, on_device); }
    fls_status map_image_import(const void* src, size_t n, int on_device) override {
        return owner ? FLS_ERR_INVALID : maps.image_import(src, n, on_device, have_map, [this] { map_replaced(); });
    }
    size_t map_export(void* blob, size_t cap) override { return owner ? 0 : maps.export_blob(blob, cap); }
    fls_status map_import(const void* blob, size_t n) override { return map_image_import(blob, n, 0); }
    bool can_replicate() const override { return !owner && have_map; }
    fls_status replicate_from(fls_matcher& o) override {
        if (o.kind != kind || owner) return FLS_ERR_STATE;
        KdMatcher& src = static_cast<KdMatcher&>(o);
        return maps.replicate_from(src.maps, [&src] { return src.prepare_batch(); }, have_map, [this] { map_replaced(); });
    }
    size_t map_size(int slot) const override {  // (any other slot: the map's points; LoamFull: slot 1 is the corner map)
        return KdMaps::counts(slot) ? maps.counter(slot) : maps.map[maps.n_maps > 1 && slot == 1].n;
    }
};

// ---------------------------------------------------------------------------------------------
struct IcpMatcher final : KdMatcher {
    std::vector<PtI> source;
    SourceFilter src_filter;
    DevBuf<unsigned> d_ticket;
    DevScan scan;
    size_t raw_n = 0;
    DevBuf<int> d_nn_id;
    DevBuf<unsigned char> d_eff;

    fls_status init() {
        if (unset_f(p.map_cloud_filter_size) || unset_f(p.source_cloud_filter_size) || unset_d(p.point_search_thres) ||
            unset_d(p.position_converge_thres) || unset_d(p.rotation_converge_thres) || unset_d(p.rot_thre_add_cloud) ||
            unset_d(p.dist_thre_add_cloud) || p.local_map_size == 0x7fffffffu)
            return FLS_ERR_INVALID;  // CHECK_NE block icp_optimized.h:33-41
        if (!(p.point_search_thres > 0.0) || !(p.map_cloud_filter_size > 0.f) || !(p.source_cloud_filter_size > 0.f)) return FLS_ERR_INVALID;
        init_common();
        src_filter.init();
        // AddCloudToLocalMap :165-189, Q13: always filtered.  Gate-sized cells here: the ICP scan starts far from the map (1-NN often beyond half the
        // gate in the early iterations), the two-stage search would run its second stage for most queries (measured 25 vs 13.5 us / launch)
        maps.init(kind, p, device, stream, {{true, p.map_cloud_filter_size, cell_for_gate(p.point_search_thres), 1, p.local_map_size}});
        init_tickets(d_ticket);
        return FLS_OK;
    }
    fls_status scan_upload(const float* s0, size_t n0, const float*, size_t, int stride) override {
        raw_n = n0;
        src_filter.filter(s0, n0, stride, p.source_cloud_filter_size, stream, scan, source);  // :57
        return FLS_OK;
    }
    fls_status scan_upload_raw(const float* s0, size_t n0, const float*, size_t, int stride) override {
        raw_n = n0;
        src_filter.upload_raw_only(s0, n0, stride, p.source_cloud_filter_size, stream, scan, source);
        have_final = false;  // (no filtered scan is resident until the next Match: fls_get_fitness_score answers FLS_ERR_STATE)
        return FLS_OK;
    }
    fls_status scan_attach_device(const HandoffCloud& c) override {
        raw_n = c.n;
        src_filter.attach_raw_only(c, p.source_cloud_filter_size, stream, scan, source);
        have_final = false;
        return FLS_OK;
    }
    // One Match in three parts -- prepare (checks, the source filter, buffers), launch (the iteration launches and the wait for the mailbox), finish
    // (the epilogue) -- so that a group of batch jobs can share the middle part (match_batch_fused) around the same prepare and finish.
    struct MatchPlan {
        size_t n = 0;       // filtered source points
        unsigned rows = 0;  // workgroups of the search grid = partial rows
        CellGridDev cg{};
        Pose16 T0{};
    };
    fls_status match_prepare(const double* T, MatchPlan& m) {
        if (raw_n <= 10) return FLS_ERR_INVALID;  // CHECK_GT(ordered_cloud_.size(), 10u) :55
        if (src_filter.raw_pending) src_filter.refilter(stream, scan, source);  // :57, on the resident raw scan
        if (!map_ready()) return FLS_ERR_STATE;
        const size_t n = scan.n;
        stats = fls_stats{};
        stats.n_source = int(n);
        d_nn_id.reserve(std::max<size_t>(n, 1));
        d_eff.reserve(std::max<size_t>(n, 1));
        m.n = n;
        m.cg = cell_dev(read_maps().map[0].grid);
        m.rows = knn_grid_blocks(n);
        d_partials_b.reserve(size_t(std::max(m.rows, 1u)) * kPartialStride);
        std::memcpy(m.T0.m, T, sizeof(m.T0.m));
        return FLS_OK;
    }
    unsigned match_launch(const MatchPlan& m) {
        const size_t n = m.n;
        const dim3 knn_grid_dim(m.rows);
        const CellGridDev& cg = m.cg;
        const Pose16& T0 = m.T0;
        return run_mailbox_loop(int(p.max_iterations), n, [&](int it, int first) {
            if (profiling) FLS_HIP(hipEventRecord(ev[2 * it], stream));
            // search + fit in one launch (one partial row per workgroup of the search grid) and the Gauss-Newton tail in its last
            // workgroup: one launch per iteration
            const LuTailArgs tail{0, p.rotation_converge_thres, p.position_converge_thres, 0, mb_dev, launch_word()};
            hipLaunchKernelGGL(icp_knn_fit_kernel, knn_grid_dim, dim3(256), 0, stream, scan.x.p, scan.y.p, scan.z.p, int(n), d_state.p, first,
                               T0, cg, float(p.point_search_thres), p.point_search_thres, d_nn_id.p, d_eff.p, d_partials_b.p, d_ticket.p,
                               kTicketShards, tail);
            if (profiling) FLS_HIP(hipEventRecord(ev[2 * it + 1], stream));
        });
    }
    fls_status match_finish(double* T, unsigned word, int update_map, fls_stats* out) {
        const Mailbox& mb = take_result(word);
        std::memcpy(T, mb.T, sizeof(double) * 16);
        std::memcpy(final_T, mb.T, sizeof(final_T));
        have_final = true;
        return finish_match(final_T, mb.converged != 0, update_map, out);  // Q10: not converged after max iterations
    }
    // the filtered scan the Match just used: the source filter's output planes while it is still on the device (false: the host filter ran)
    bool keyframe_device(DeviceCloudRing::DeviceCloud* src) override {
        if (!src_filter.resident) return false;
        const DeviceVoxelGrid& vg = src_filter.vg;
        src[0] = DeviceCloudRing::DeviceCloud{vg.ox(), vg.oy(), vg.oz(), vg.oi(), vg.n_out};
        return true;
    }
    void keyframe_host(const std::vector<PtI>** clouds) override {
        src_filter.materialize(stream, source);
        clouds[0] = &source;
    }
    fls_status match_resident(double* T, int update_map, fls_stats* out) override {
        MatchPlan m;
        const fls_status prc = match_prepare(T, m);
        if (prc != FLS_OK) return prc;
        return match_finish(T, match_launch(m), update_map, out);
    }

    // ---- fls_match_batch_fused: groups of up to n_slots jobs share one icp_knn_fit_jobs_kernel launch per iteration ----
    // The group driver is the base's (matcher_base.hpp::run_job_groups); this kind supplies the slot's upload + source filter + prepare, its job-table
    // entries and the one launch of an iteration.
    PinnedBuf<IcpJob> h_jobs;
    DevBuf<IcpJob> d_jobs;
    fls_status match_batch_fused(size_t n_jobs, const float* const* s0, const size_t* n0, const float* const*, const size_t*, int stride, double* T,
                                 fls_stats* st, int32_t* status, int n_slots) override {
        std::vector<MatchPlan> plan(size_t(2) * kMaxLanes);  // per slot
        unsigned rows_max = 0; CellGridDev cg{};              // of the group's launches (one map for every job: the owner's grid)
        auto stats_of = [&](const size_t j) { return st ? &st[j] : nullptr; };
        // a rejected job keeps its status; a job whose filtered scan is empty is the per-lane path's from here (its launches go to the slot's own stream)
        auto prepare = [&](IcpMatcher* q, const size_t s, const size_t j, bool& shared) -> fls_status {
            fls_status rc = q->scan_upload(s0[j], n0[j], nullptr, 0, stride);
            if (rc == FLS_OK) rc = q->match_prepare(T + 16 * j, plan[s]);
            if (rc == FLS_OK && plan[s].n == 0) return q->match_finish(T + 16 * j, q->match_launch(plan[s]), 0, stats_of(j));
            shared = rc == FLS_OK;
            return rc;
        };
        auto table = [&](GroupCall<IcpMatcher>& c) {
            const size_t A = c.act.size();
            if (!h_jobs.p) { h_jobs.reserve(kMaxLanes); d_jobs.reserve(kMaxLanes); }
            rows_max = 0;
            for (size_t i = 0; i < A; ++i) {
                IcpMatcher* q = c.act[i];
                const MatchPlan& m = plan[c.act_slot[i]];
                IcpJob& e = h_jobs.p[i];
                e.sx = q->scan.x.p; e.sy = q->scan.y.p; e.sz = q->scan.z.p;
                e.n = int(m.n); e.rows = int(m.rows);
                e.st = q->d_state.p; e.nn_id = q->d_nn_id.p; e.eff = q->d_eff.p; e.partials = q->d_partials_b.p; e.ticket = q->d_ticket.p;
                e.mb = q->mb_dev; e.launch_word = q->launch_word(); e.pad = 0u;
                e.T0 = m.T0;
                rows_max = std::max(rows_max, m.rows);
                cg = m.cg;
            }
            // (the pinned table is free: every launch that could read the device copy of the previous group's has been waited for or exits at once,
            // and the copy below is ordered behind them on the batch stream)
            FLS_HIP(hipMemcpyAsync(d_jobs.p, h_jobs.p, A * sizeof(IcpJob), hipMemcpyHostToDevice, batch_stream));
        };
        auto queue = [&](GroupCall<IcpMatcher>& c, const int first) {
            hipLaunchKernelGGL(icp_knn_fit_jobs_kernel, dim3(rows_max, unsigned(c.act.size())), dim3(256), 0, batch_stream, (const IcpJob*)d_jobs.p, first, cg,
                               float(p.point_search_thres), p.point_search_thres, kTicketShards, p.rotation_converge_thres, p.position_converge_thres);
            ++batch_counters[0];
        };
        auto finish = [&](IcpMatcher* q, const size_t j, const unsigned word) -> fls_status {
            q->end_match(word, q->scan.n);
            return q->match_finish(T + 16 * j, word, 0, stats_of(j));
        };
        return run_job_groups<IcpMatcher>(n_jobs, s0, n0, stride, T, st, status, n_slots, GroupCounters{&batch_counters[1], &batch_counters[2], &batch_counters[3]},
                                          prepare, table, queue, finish);
    }
    std::unique_ptr<fls_matcher> clone_for_lane() override { return make_owned_lane(*this); }
    fls_status fitness(float max_range, float* score) override {
        if (owner || !have_map || !have_final) return FLS_ERR_STATE;
        return fitness_score_device(*this, maps.map[0].grid, scan, final_T, max_range, score);
    }
    int correspondences(int, int32_t* ids, uint8_t* cnt, uint8_t* valid, size_t cap) override {
        const size_t n = std::min(cap, scan.n);
        if (!n) return 0;
        std::vector<int> id(n);
        std::vector<unsigned char> ef(n);
        FLS_HIP(hipMemcpyAsync(id.data(), d_nn_id.p, n * sizeof(int), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipMemcpyAsync(ef.data(), d_eff.p, n, hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        for (size_t i = 0; i < n; ++i) { ids[i] = id[i]; cnt[i] = id[i] >= 0 ? 1 : 0; valid[i] = ef[i]; }
        return int(n);
    }
    size_t map_size(int slot) const override {
        if (slot == 105) return size_t(src_filter.device_runs);  // source filters run on the device / on the host
        if (slot == 106) return size_t(src_filter.host_runs);
        return KdMatcher::map_size(slot);
    }
};

// ---------------------------------------------------------------------------------------------
// per-feature-class device buffers of the LOAM kinds
struct FeatureDev {
    DevScan scan;
    DevBuf<float4> nn_pts;           // [n][5] neighbours left by grid_knn_kernel<5>
    DevBuf<unsigned char> nn_cnt, flag, cnt_out;
    DevBuf<float> kth;               // d2 of the 5th neighbour
    DevBuf<int> nn_id;               // [n][5] reported ids (gate-accepted sets only)
    DevBuf<double> J;
    void prepare() {
        const size_t n = std::max<size_t>(scan.n, 1);
        nn_pts.reserve(n * 5); nn_cnt.reserve(n); cnt_out.reserve(n); kth.reserve(n); nn_id.reserve(n * 5); flag.reserve(n); J.reserve(7 * n);
    }
    int fetch(hipStream_t s, int32_t* ids, uint8_t* cnt, uint8_t* valid, size_t cap) {
        const size_t n = std::min(cap, scan.n);
        if (!n) return 0;
        FLS_HIP(hipMemcpyAsync(ids, nn_id.p, n * 5 * sizeof(int), hipMemcpyDeviceToHost, s));
        FLS_HIP(hipMemcpyAsync(cnt, cnt_out.p, n, hipMemcpyDeviceToHost, s));
        FLS_HIP(hipMemcpyAsync(valid, flag.p, n, hipMemcpyDeviceToHost, s));
        FLS_HIP(hipStreamSynchronize(s));
        return int(n);
    }
    GridKnnArgs knn_args(const CellGridDev& cg, float gate) {
        return GridKnnArgs{scan.x.p, scan.y.p, scan.z.p, int(scan.n), cg, gate, nn_pts.p, nn_cnt.p, kth.p, flag.p};
    }
    FeatureFitArgs fit_args(float gate, double thres, double* partials) {
        return FeatureFitArgs{scan.x.p, scan.y.p, scan.z.p, int(scan.n), nn_pts.p, nn_cnt.p, kth.p, gate, thres, nn_id.p, cnt_out.p, J.p, flag.p, partials};
    }
    // grid_knn_kernel<5> (flags cleared by the first iteration: once per Match, Q1) + feature_fit_kernel<LINE>
    template <bool LINE>
    void launch(hipStream_t s, GnState* st, int first, const Pose16& T0, const CellGridDev& cg, float gate, double thres, double* partials) {
        const size_t n = scan.n;
        if (n == 0) return;
        const dim3 knn_grid_dim(knn_grid_blocks(n));
        if (std::isinf(gate))  // un-gated search (LoamPointToPlaneKdtree): the instantiation with the ring walk
            hipLaunchKernelGGL((grid_knn_kernel<5, false, true>), knn_grid_dim, dim3(256), 0, s, scan.x.p, scan.y.p, scan.z.p, int(n), st, first, T0, cg, gate,
                               nn_pts.p, nn_cnt.p, kth.p, flag.p);
        else
            hipLaunchKernelGGL((grid_knn_kernel<5, false>), knn_grid_dim, dim3(256), 0, s, scan.x.p, scan.y.p, scan.z.p, int(n), st, first, T0, cg, gate,
                               nn_pts.p, nn_cnt.p, kth.p, flag.p);
        hipLaunchKernelGGL((feature_fit_kernel<LINE>), dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, scan.x.p, scan.y.p, scan.z.p, int(n), st,
                           first, T0, (const float4*)nn_pts.p, (const unsigned char*)nn_cnt.p, (const float*)kth.p, gate, thres, nn_id.p,
                           cnt_out.p, J.p, flag.p, partials);
    }
};

struct LoamFullMatcher final : KdMatcher {  // maps.map[0]: planar, [1]: corner
    FeatureDev corner, planar;
    DevBuf<unsigned> d_loam_ticket;

    fls_status init() {
        if (unset_d(p.point_to_planar_thres) || unset_d(p.point_search_thres) || unset_d(p.line_ratio_thres) ||
            unset_d(p.position_converge_thres) || unset_d(p.rotation_converge_thres) || unset_d(p.rot_thre_add_cloud) ||
            unset_d(p.dist_thre_add_cloud))
            return FLS_ERR_INVALID;  // CHECK_NE block loam_full_kdtree.h:44-53
        if (p.local_planar_size == 0 || p.local_corner_size == 0) return FLS_ERR_INVALID;  // CHECK_GT :55-56
        if (!(p.point_search_thres > 0.0) || !(p.corner_voxel_filter_size > 0.f) || !(p.planar_voxel_filter_size > 0.f)) return FLS_ERR_INVALID;
        init_common();
        init_tickets(d_loam_ticket);
        // AddCloudToLocalMap :65-104: half-gate cells + the two-stage kernel; the VoxelGrid only once the deque holds more than 5 frames (:92-100)
        const float cs = 0.5f * cell_for_gate(p.point_search_thres);
        maps.init(kind, p, device, stream, {{false, p.planar_voxel_filter_size, cs, kGridRings, p.local_planar_size},
                                            {false, p.corner_voxel_filter_size, cs, kGridRings, p.local_corner_size}});
        xform_double = true;
        return FLS_OK;
    }
    fls_status scan_upload(const float* s0, size_t n0, const float* s1, size_t n1, int stride) override {
        planar.scan.upload(cloud_from(s0, n0, stride), stream);
        corner.scan.upload(s1 ? cloud_from(s1, n1, stride) : std::vector<PtI>(), stream);
        return FLS_OK;
    }
    fls_status scan_attach_features(const HandoffCloud& planar_cloud, const HandoffCloud& corner_cloud) override {
        planar.scan.attach_device(planar_cloud, stream, /*want_host=*/true);  // (a cloud of no points is attached as the empty scan)
        corner.scan.attach_device(corner_cloud, stream, /*want_host=*/true);
        return FLS_OK;
    }
    fls_status match_resident(double* T, int update_map, fls_stats* out) override {
        if (!map_ready()) return FLS_ERR_STATE;
        const size_t np = planar.scan.n, nc = corner.scan.n;
        const int nbp = int((np + 255) / 256), nbc = int((nc + 255) / 256);
        stats = fls_stats{};
        stats.n_source = int(np);
        stats.n_source_corner = int(nc);
        planar.prepare();
        corner.prepare();
        d_partials_a.reserve(size_t(std::max(nbc, 1)) * kPartialStride);
        d_partials_b.reserve(size_t(std::max(nbp, 1)) * kPartialStride);
        const CellGridDev cgp = cell_dev(read_maps().map[0].grid), cgc = cell_dev(read_maps().map[1].grid);
        const float gate_f = float(p.point_search_thres);
        Pose16 T0;
        std::memcpy(T0.m, T, sizeof(T0.m));
        const unsigned word = run_mailbox_loop(int(p.max_iterations), np + nc, [&](int it, int first) {
            if (profiling) FLS_HIP(hipEventRecord(ev[2 * it], stream));
            if (nc != 0 && np != 0) {
                // both classes in one correspondence launch and one fit launch (they are independent until the solve), the Gauss-Newton
                // tail in the fit launch's last workgroup
                const int kc = int(knn_grid_blocks(nc)), kp = int(knn_grid_blocks(np));
                hipLaunchKernelGGL((grid_knn_dual_kernel<5, false>), dim3(unsigned(kc + kp)), dim3(256), 0, stream, (const GnState*)d_state.p, first, T0,
                                   corner.knn_args(cgc, gate_f), planar.knn_args(cgp, gate_f), kc);
                const LoamFusedTail tail{(const double*)d_partials_a.p, (const double*)d_partials_b.p, nbc, nbp, p.rotation_converge_thres, p.position_converge_thres,
                                         d_loam_ticket.p, kTicketShards, mb_dev, launch_word()};
                hipLaunchKernelGGL(feature_fit_dual_kernel, dim3(unsigned(nbc + nbp)), dim3(256), 0, stream, (const GnState*)d_state.p, first, T0,
                                   corner.fit_args(gate_f, p.line_ratio_thres, d_partials_a.p), planar.fit_args(gate_f, p.point_to_planar_thres, d_partials_b.p), nbc, tail);
                if (profiling) FLS_HIP(hipEventRecord(ev[2 * it + 1], stream));
                return;
            }
            // one feature class is empty: one correspondence + one fit launch per class, then the tail
            corner.launch<true>(stream, d_state.p, first, T0, cgc, gate_f, p.line_ratio_thres, d_partials_a.p);
            planar.launch<false>(stream, d_state.p, first, T0, cgp, gate_f, p.point_to_planar_thres, d_partials_b.p);
            if (profiling) FLS_HIP(hipEventRecord(ev[2 * it + 1], stream));
            hipLaunchKernelGGL(gn_solve_loam_kernel, dim3(1), dim3(kSolveThreads), 0, stream, d_state.p, first, T0, (const double*)d_partials_a.p,
                               nbc, (const double*)d_partials_b.p, nbp, p.rotation_converge_thres, p.position_converge_thres, mb_dev, launch_word());
        });
        const Mailbox& mb = take_result(word);
        std::memcpy(T, mb.T, sizeof(double) * 16);
        stats.n_valid_corner = mb.n_valid2;
        stats.sum_res_corner = mb.sum_res2;
        return finish_match(mb.T, mb.n_valid >= 50, update_map, out);  // number_valid_planar_ < 50 :181
    }
    // both feature scans, still on the device
    bool keyframe_device(DeviceCloudRing::DeviceCloud* src) override {
        const DevScan* scans[2] = {&planar.scan, &corner.scan};
        return maps.scan_sources(scans, src);
    }
    void keyframe_host(const std::vector<PtI>** clouds) override {
        planar.scan.fetch_host(stream);  // (attached scans are fetched only here)
        corner.scan.fetch_host(stream);
        clouds[0] = &planar.scan.host; clouds[1] = &corner.scan.host;
    }
    std::unique_ptr<fls_matcher> clone_for_lane() override { return make_owned_lane(*this); }
    fls_status fitness(float, float* score) override { *score = std::numeric_limits<float>::max(); return FLS_OK; }  // FloatNaN :206-208
    int correspondences(int slot, int32_t* ids, uint8_t* cnt, uint8_t* valid, size_t cap) override {
        return (slot == 1 ? corner : planar).fetch(stream, ids, cnt, valid, cap);
    }
};

// ---------------------------------------------------------------------------------------------
struct P2PlaneKdMatcher final : KdMatcher {
    FeatureDev planar;

    fls_status init() {
        if (unset_d(p.point_to_planar_thres) || unset_d(p.position_converge_thres) || unset_d(p.rotation_converge_thres) ||
            unset_d(p.rot_thre_add_cloud) || unset_d(p.dist_thre_add_cloud) || unset_f(p.map_cloud_filter_size))
            return FLS_ERR_INVALID;  // CHECK_NE block loam_point_to_plane_kdtree.h:43-50
        if (!(p.map_cloud_filter_size > 0.f)) return FLS_ERR_INVALID;
        init_common();
        // AddCloudToLocalMap :56-79.  un-gated 5-NN: ring search with a cell of two map leaves (>= 1 point per leaf after VoxelGrid)
        maps.init(kind, p, device, stream, {{true, p.map_cloud_filter_size, std::max(2.0f * p.map_cloud_filter_size, 0.5f), 1, p.local_map_size}});
        return FLS_OK;
    }
    fls_status scan_upload(const float* s0, size_t n0, const float*, size_t, int stride) override {
        planar.scan.upload(cloud_from(s0, n0, stride), stream);
        return FLS_OK;
    }
    fls_status scan_attach_device(const HandoffCloud& c) override {
        planar.scan.attach_device(c, stream, /*want_host=*/true);
        return FLS_OK;
    }
    fls_status match_resident(double* T, int update_map, fls_stats* out) override {
        if (!map_ready()) return FLS_ERR_STATE;
        const size_t n = planar.scan.n;
        const int nblk = int((n + 255) / 256);
        stats = fls_stats{};
        stats.n_source = int(n);
        planar.prepare();
        d_partials_b.reserve(size_t(std::max(nblk, 1)) * kPartialStride);
        const CellGridDev cg = cell_dev(read_maps().map[0].grid);
        Pose16 T0;
        std::memcpy(T0.m, T, sizeof(T0.m));
        const unsigned word = run_mailbox_loop(int(p.max_iterations), n, [&](int it, int first) {
            if (profiling) FLS_HIP(hipEventRecord(ev[2 * it], stream));
            planar.launch<false>(stream, d_state.p, first, T0, cg, INFINITY, p.point_to_planar_thres, d_partials_b.p);  // un-gated (:219)
            if (profiling) FLS_HIP(hipEventRecord(ev[2 * it + 1], stream));
            hipLaunchKernelGGL(gn_solve_loam_kernel, dim3(1), dim3(kSolveThreads), 0, stream, d_state.p, first, T0, (const double*)nullptr, 0,
                               (const double*)d_partials_b.p, nblk, p.rotation_converge_thres, p.position_converge_thres, mb_dev, launch_word());
        });
        const Mailbox& mb = take_result(word);
        std::memcpy(T, mb.T, sizeof(double) * 16);
        std::memcpy(final_T, mb.T, sizeof(final_T));
        have_final = true;
        return finish_match(final_T, mb.n_valid >= 50, update_map, out);
    }
    // the scan, still on the device
    bool keyframe_device(DeviceCloudRing::DeviceCloud* src) override {
        const DevScan* scans[1] = {&planar.scan};
        return maps.scan_sources(scans, src);
    }
    void keyframe_host(const std::vector<PtI>** clouds) override {
        planar.scan.fetch_host(stream);  // (an attached scan is fetched only here)
        clouds[0] = &planar.scan.host;
    }
    std::unique_ptr<fls_matcher> clone_for_lane() override { return make_owned_lane(*this); }
    fls_status fitness(float max_range, float* score) override {
        if (owner || !have_map || !have_final) return FLS_ERR_STATE;
        return fitness_score_device(*this, maps.map[0].grid, planar.scan, final_T, max_range, score);
    }
    int correspondences(int, int32_t* ids, uint8_t* cnt, uint8_t* valid, size_t cap) override { return planar.fetch(stream, ids, cnt, valid, cap); }
};

}  // namespace fls
