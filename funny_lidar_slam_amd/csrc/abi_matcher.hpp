// abi_matcher.hpp -- the matcher ABI: include/fls_reg.h (less its fls_debug_* hooks), fls_batch.h, fls_batch_ivox.h, fls_map_ivox.h,
// fls_map_ndt.h, fls_map_kd.h.  Host code only: argument checks, then the call on the handle's device (abi_common.hpp).
#pragma once
#include "abi_common.hpp"

namespace {

template <class M>
fls_status create_matcher(fls_kind kind, const fls_params& params, int device_id, fls_handle* out) {
    return create_handle<M>(device_id, out, [&](M& m) { m.kind = kind; m.p = params; }, Guard::kPlain, /*say=*/true);
}

// one matcher per device, kept for the life of the process (stream, result block, device buffers: ~3 ms to set up, the reference's
// loop-closure thread calls Match once per candidate); calls on one device are serialised (run_mx).  Never destroyed: static
// destruction would run after the HIP runtime's own teardown.
fls_status loop_matcher_for(int device_id, LoopMatcher*& m) {
    const fls_status dev = gfx950_device(device_id);
    if (dev != FLS_OK) return dev;
    static std::mutex mx;
    static std::map<int, LoopMatcher*>* cache = new std::map<int, LoopMatcher*>();
    std::lock_guard<std::mutex> lk(mx);
    LoopMatcher*& slot = (*cache)[device_id];
    if (!slot) {
        std::unique_ptr<LoopMatcher> fresh(new LoopMatcher());
        fresh->init(device_id);
        slot = fresh.release();
    }
    m = slot;
    return FLS_OK;
}

}  // namespace

extern "C" {

int fls_abi_version(void) { return FLS_ABI_VERSION; }
int fls_abi_revision(void) { return FLS_ABI_REVISION; }

int fls_device_count(void) {
    int n = 0, ok = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    for (int d = 0; d < n; ++d) ok += gfx950_device(d) == FLS_OK;
    return ok;
}

const char* fls_status_string(int s) {
    switch (s) {
        case FLS_OK: return "ok (Match returned true)";
        case FLS_NOT_CONVERGED: return "not converged (Match returned false)";
        case FLS_SKIPPED: return "batch job not run";
        case FLS_ERR_INVALID: return "invalid argument or unset parameter";
        case FLS_ERR_DEVICE: return "HIP error or no gfx950 device";
        case FLS_ERR_RANGE: return "coordinate outside the voxel key range";
        case FLS_ERR_NOMEM: return "out of memory";
        case FLS_ERR_STATE: return "call order violated";
        default: return "unknown status";
    }
}

fls_status fls_create(fls_kind kind, const fls_params* params, int device_id, fls_handle* out) {
    if (!out) return FLS_ERR_INVALID;
    *out = nullptr;
    if (!params) return FLS_ERR_INVALID;
    const fls_status pc = check_common(*params);
    if (pc != FLS_OK) return pc;
    switch (kind) {
        case FLS_P2PLANE_IVOX: return create_matcher<P2PlaneIvoxMatcher>(kind, *params, device_id, out);
        case FLS_ICP_OPTIMIZED: return create_matcher<IcpMatcher>(kind, *params, device_id, out);
        case FLS_INCREMENTAL_NDT: return create_matcher<NdtMatcher>(kind, *params, device_id, out);
        case FLS_LOAM_FULL: return create_matcher<LoamFullMatcher>(kind, *params, device_id, out);
        case FLS_P2PLANE_KDTREE: return create_matcher<P2PlaneKdMatcher>(kind, *params, device_id, out);
        default: return gfx950_device(device_id, true) != FLS_OK ? FLS_ERR_DEVICE : FLS_ERR_INVALID;  // (the device is judged before the kind)
    }
}

void fls_destroy(fls_handle h) {
    destroy_handle(h, [&] { h->lanes.clear(); });  // the batch lanes read this handle's map: they go first
}

fls_status fls_add_cloud_to_local_map(fls_handle h, const float* c0, size_t n0, const float* c1, size_t n1, int stride) {
    if (!h || (!c0 && n0) || stride < 3) return FLS_ERR_INVALID;
    return on_device(h, [&] { return h->add_cloud(c0, n0, c1, n1, stride); });
}

// (the two uploads synchronise the stream: fls_reg.h promises that they return after the upload has completed)
fls_status fls_scan_upload(fls_handle h, const float* s0, size_t n0, const float* s1, size_t n1, int stride) {
    if (!h || (!s0 && n0) || stride < 3) return FLS_ERR_INVALID;
    return on_device(h, [&] {
        const fls_status rc = h->scan_upload(s0, n0, s1, n1, stride);
        FLS_HIP(hipStreamSynchronize(h->stream));
        return rc;
    });
}

fls_status fls_scan_upload_raw(fls_handle h, const float* s0, size_t n0, const float* s1, size_t n1, int stride) {
    if (!h || (!s0 && n0) || stride < 3) return FLS_ERR_INVALID;
    return on_device(h, [&] {
        const fls_status rc = h->scan_upload_raw(s0, n0, s1, n1, stride);
        FLS_HIP(hipStreamSynchronize(h->stream));
        return rc;
    });
}

fls_status fls_match_resident(fls_handle h, double T[16], int update_map, fls_stats* stats) {
    if (!h || !T) return FLS_ERR_INVALID;
    return on_device(h, [&] { return h->match_resident(T, update_map, stats); });
}

fls_status fls_match(fls_handle h, const float* s0, size_t n0, const float* s1, size_t n1, int stride, double T[16], int update_map,
                     fls_stats* stats) {
    if (!h || !T || (!s0 && n0) || stride < 3) return FLS_ERR_INVALID;
    return on_device(h, [&] {
        const fls_status rc = h->scan_upload_for_match(s0, n0, s1, n1, stride);
        return rc != FLS_OK ? rc : h->match_resident(T, update_map, stats);
    });
}

// (the size_t getters have no status to return: a failure is 0, or what was counted before it)
size_t fls_map_image_bytes(fls_handle h) {
    if (!h) return 0;
    size_t n = 0;
    (void)on_device(h, [&] { n = h->map_image_bytes(); return FLS_OK; });
    return n;
}
fls_status fls_map_image_export(fls_handle h, void* dst, size_t cap_bytes, int dst_on_device) {
    if (!h || !dst) return FLS_ERR_INVALID;
    return on_device(h, [&] { return h->map_image_export(dst, cap_bytes, dst_on_device); });
}
fls_status fls_map_image_import(fls_handle h, const void* src, size_t n_bytes, int src_on_device) {
    if (!h || !src) return FLS_ERR_INVALID;
    return on_device(h, [&] { return h->map_image_import(src, n_bytes, src_on_device); });
}

fls_status fls_match_batch(fls_handle h, size_t n_jobs, const float* const* src0, const size_t* n0, const float* const* src1,
                           const size_t* n1, int stride, double* T, fls_stats* stats, int32_t* status, int lanes) {
    return batch_call(h, n_jobs, src0, n0, src1, n1, stride, T, /*check_rows=*/true, /*empty_is_ok=*/false, [&] {
        return on_device(h, [&] { return h->match_batch(n_jobs, src0, n0, src1, n1, stride, T, stats, status, lanes); });
    });
}

// ---- include/fls_batch.h ----
int fls_batch_revision(void) { return FLS_BATCH_REVISION; }

fls_status fls_match_batch_fused(fls_handle h, size_t n_jobs, const float* const* src0, const size_t* n0, const float* const* src1,
                                 const size_t* n1, int stride, double* T, fls_stats* stats, int32_t* status, int n_slots) {
    return batch_call(h, n_jobs, src0, n0, src1, n1, stride, T, /*check_rows=*/true, /*empty_is_ok=*/true, [&] {
        return on_device(h, [&] { return h->match_batch_fused(n_jobs, src0, n0, src1, n1, stride, T, stats, status, n_slots); });
    });
}

size_t fls_batch_stat(fls_handle h, int slot) { return (h && slot >= 0 && slot < 4) ? h->batch_counters[slot] : 0; }

// ---- include/fls_batch_ivox.h ----
int fls_batch_ivox_revision(void) { return FLS_BATCH_IVOX_REVISION; }

fls_status fls_match_batch_shared_ivox(fls_handle h, size_t n_jobs, const float* const* src0, const size_t* n0, const float* const* src1,
                                       const size_t* n1, int stride, double* T, fls_stats* stats, int32_t* status, int n_slots) {
    return batch_call(h, n_jobs, src0, n0, src1, n1, stride, T, /*check_rows=*/true, /*empty_is_ok=*/true, [&] {
        return on_device(h, [&] { return h->match_batch_shared_ivox(n_jobs, src0, n0, src1, n1, stride, T, stats, status, n_slots); });
    });
}

size_t fls_batch_ivox_stat(fls_handle h, int slot) { return (h && slot >= 0 && slot < 5) ? h->batch_ivox_counters[slot] : 0; }

size_t fls_map_export(fls_handle h, void* blob, size_t cap) {
    if (!h) return 0;
    size_t n = 0;
    (void)on_device(h, [&] { n = h->map_export(blob, cap); return FLS_OK; });
    return n;
}

fls_status fls_map_import(fls_handle h, const void* blob, size_t n) {
    if (!h || !blob) return FLS_ERR_INVALID;
    return on_device(h, [&] { return h->map_import(blob, n); });
}

// ---- include/fls_map_ivox.h: the blob of fls_map_export / fls_map_import for an FLS_P2PLANE_IVOX handle, packed and built on the device ----
unsigned fls_ivox_blob_revision(void) { return FLS_IVOX_BLOB_REVISION; }

size_t fls_ivox_map_bytes(fls_handle h) {
    if (!h) return 0;
    size_t n = 0;
    (void)guarded([&]() -> fls_status { n = h->ivox_blob_bytes(); return FLS_OK; });  // no device set: the size is computed from host counts
    return n;
}

fls_status fls_ivox_map_export(fls_handle h, void* dst, size_t cap_bytes, int dst_on_device) {
    if (!h || !dst) return FLS_ERR_INVALID;
    return on_device(h, [&] { return h->ivox_blob_export(dst, cap_bytes, dst_on_device); });
}

fls_status fls_ivox_map_import(fls_handle h, const void* src, size_t n_bytes, int src_on_device) {
    if (!h || !src) return FLS_ERR_INVALID;
    return on_device(h, [&] { return h->ivox_blob_import(src, n_bytes, src_on_device); });
}

// ---- include/fls_map_ndt.h: the format fls_map_export / fls_map_image_export write for an FLS_INCREMENTAL_NDT handle ----
int fls_ndt_image_revision(void) { return FLS_NDT_IMAGE_REVISION; }

// ---- include/fls_map_kd.h: the format fls_map_export / fls_map_image_export write for the kd-tree kinds ----
int fls_kd_image_revision(void) { return FLS_KD_IMAGE_REVISION; }

// ---- replica sets (fls_reg.h; the fused batch over a set: fls_map_kd.h).  A set spans devices: no call here sets one, each member handle's
// own calls do (replicas.hpp) ----
fls_status fls_replicas_create(fls_handle owner, const int* device_ids, int n_devices, fls_replicas_handle* out) {
    if (!out) return FLS_ERR_INVALID;
    *out = nullptr;
    if (!owner || !device_ids || n_devices <= 0 || n_devices > 64) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return FLS_ERR_DEVICE;
        for (int i = 0; i < n_devices; ++i)
            if (device_ids[i] < 0 || device_ids[i] >= n) return FLS_ERR_DEVICE;
        std::unique_ptr<fls_replicas> r(new fls_replicas());
        r->owner = owner;
        bool owner_used = false;
        for (int i = 0; i < n_devices; ++i) {
            r->devices.push_back(device_ids[i]);
            r->import_ms.push_back(0.0);
            if (device_ids[i] == owner->device && !owner_used) {
                owner_used = true;
                r->handles.push_back(owner);
                r->owned.push_back(0);
                continue;
            }
            fls_handle h = nullptr;
            const fls_status rc = fls_create(owner->kind, &owner->p, device_ids[i], &h);
            if (rc < 0) return rc;  // (the set's destructor releases what was created so far)
            r->handles.push_back(h);
            r->owned.push_back(1);
        }
        const fls_status rc = r->refresh();
        if (rc < 0) return rc;
        *out = r.release();
        return FLS_OK;
    });
}

fls_status fls_replicas_refresh(fls_replicas_handle r) {
    if (!r) return FLS_ERR_INVALID;
    return guarded([&]() -> fls_status { return r->refresh(); });
}

fls_status fls_replicas_match_batch(fls_replicas_handle r, size_t n_jobs, const float* const* src0, const size_t* n0, const float* const* src1,
                                    const size_t* n1, int stride, double* T, fls_stats* stats, int32_t* status, int lanes) {
    return batch_call(r, n_jobs, src0, n0, src1, n1, stride, T, /*check_rows=*/false, /*empty_is_ok=*/false, [&] {
        return guarded([&]() -> fls_status { return r->match_batch(n_jobs, src0, n0, src1, n1, stride, T, stats, status, lanes); });
    });
}

fls_status fls_replicas_match_batch_fused(fls_replicas_handle r, size_t n_jobs, const float* const* src0, const size_t* n0, const float* const* src1,
                                          const size_t* n1, int stride, double* T, fls_stats* stats, int32_t* status, int slots) {
    return batch_call(r, n_jobs, src0, n0, src1, n1, stride, T, /*check_rows=*/false, /*empty_is_ok=*/false, [&] {
        return guarded([&]() -> fls_status { return r->match_batch(n_jobs, src0, n0, src1, n1, stride, T, stats, status, slots, true); });
    });
}

int fls_replicas_import_ms(fls_replicas_handle r, double* ms, int cap) {
    if (!r) return 0;
    const int n = int(r->import_ms.size());
    for (int i = 0; i < std::min(n, cap); ++i)
        if (ms) ms[i] = r->import_ms[size_t(i)];
    return n;
}

void fls_replicas_destroy(fls_replicas_handle r) { delete r; }

// ---- getters and profiling ----
fls_status fls_get_fitness_score(fls_handle h, float max_range, float* score) {
    if (!h || !score) return FLS_ERR_INVALID;
    return on_device(h, [&] { return h->fitness(max_range, score); });
}

int fls_get_iteration_log(fls_handle h, double* T_iters, int32_t* n_valid, double* sum_res, int cap) {
    if (!h || !h->h_state.p) return 0;
    if (on_device(h, [&] { h->refresh_log(); return FLS_OK; }) != FLS_OK) return 0;
    const GnState& s = *h->h_state.p;
    const int n = std::min(cap, h->log_n);
    for (int i = 0; i < n; ++i) {
        if (T_iters) std::memcpy(T_iters + 16 * i, s.log_T[i], sizeof(double) * 16);
        if (n_valid) n_valid[i] = s.log_nv[i];
        if (sum_res) sum_res[i] = s.log_res[i];
    }
    return h->log_n;
}

int fls_get_correspondences(fls_handle h, int slot, int32_t* ids, uint8_t* cnt, uint8_t* valid, size_t cap) {
    if (!h || !ids || !cnt || !valid) return -1;
    int n = -1;  // (a count, so an error is -1 and not a status)
    return on_device(h, [&] { n = h->correspondences(slot, ids, cnt, valid, cap); return FLS_OK; }) == FLS_OK ? n : -1;
}

size_t fls_map_size(fls_handle h, int slot) { return h ? h->map_size(slot) : 0; }

fls_status fls_set_profiling(fls_handle h, int enable) {
    if (!h) return FLS_ERR_INVALID;
    h->profiling = (enable & 1) != 0;       // accumulators are only reset by fls_get_kernel_time, so the flag can be
    h->count_traffic = (enable & 2) != 0;   // toggled per Match (e.g. to bracket every n-th step of a timed region)
    return FLS_OK;
}

fls_status fls_get_kernel_time(fls_handle h, double* ms_total, int64_t* launches, uint64_t* point_iters) {
    if (!h) return FLS_ERR_INVALID;
    const fls_status rc = on_device(h, [&] { h->settle_events(); return FLS_OK; });
    if (rc != FLS_OK) return rc;  // (the accumulators are read and reset only once every event has settled into them)
    if (ms_total) *ms_total = h->prof_ms;
    if (launches) *launches = h->prof_launches;
    if (point_iters) *point_iters = h->prof_point_iters;
    h->prof_ms = 0.0;
    h->prof_launches = 0;
    h->prof_point_iters = 0;
    return FLS_OK;
}

fls_status fls_get_debug_stamps(fls_handle h, int64_t out[16]) {
    if (!h || !out || !h->h_state.p) return FLS_ERR_INVALID;
    (void)on_device(h, [&] { h->refresh_log(); return FLS_OK; });  // (a failed refresh leaves the stamps of the last one: still what was asked for)
    for (int i = 0; i < 16; ++i) out[i] = h->h_state.p->dbg[i];
    return FLS_OK;
}

fls_status fls_get_traffic_counters(fls_handle h, uint64_t* probes, uint64_t* hit_voxels, uint64_t* cand_points) {
    if (!h) return FLS_ERR_INVALID;
    if (probes) *probes = h->last_tc.probes;
    if (hit_voxels) *hit_voxels = h->last_tc.hits;
    if (cand_points) *cand_points = h->last_tc.cand;
    return FLS_OK;
}

// ---- the VoxelGrid filter and the loop-closure matcher, without a handle ----
fls_status fls_voxel_grid_cloud(int device_id, fls_voxelgrid_mode mode, const float* pts, size_t n, int stride, float leaf, float* out, size_t cap,
                                size_t* n_out) {
    if (mode == FLS_VOXELGRID_DEVICE) return fls_debug_voxel_grid(device_id, pts, n, stride, leaf, out, cap, n_out);
    if (mode != FLS_VOXELGRID_EXACT || (!pts && n) || !n_out || stride < 3 || !(leaf > 0.f) || (cap && !out)) return FLS_ERR_INVALID;
    *n_out = 0;
    return guarded([&]() -> fls_status {
        const std::vector<PtI> c = voxel_grid_strided(pts, n, stride, leaf);  // host_maps.hpp: the exact filter (pooled introsort order)
        *n_out = c.size();
        if (c.size() > cap) return FLS_ERR_INVALID;
        if (!c.empty()) std::memcpy(out, c.data(), c.size() * sizeof(PtI));
        return FLS_OK;
    });
}

fls_status fls_loop_match(int device_id, const float* source, size_t n_source, const float* target, size_t n_target, int stride, double T[16], float* fitness,
                          fls_loop_stats* stats) {
    if (!T || !fitness || stride < 3 || (!source && n_source) || (!target && n_target)) return FLS_ERR_INVALID;
    *fitness = std::numeric_limits<float>::max();
    if (stats) std::memset(stats, 0, sizeof(*stats));
    return guarded([&]() -> fls_status {
        const bool timing = host_timing_enabled();
        const auto t0 = std::chrono::steady_clock::now();
        LoopMatcher* m = nullptr;
        const fls_status got = loop_matcher_for(device_id, m);
        if (got != FLS_OK) return got;
        std::lock_guard<std::mutex> run_lk(m->run_mx);  // (devices run side by side, calls on one device one after the other)
        if (timing) std::fprintf(stderr, "[fls loop] ms: matcher set-up %.2f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        const fls_status rc = m->run(cloud_from(source, n_source, stride), cloud_from(target, n_target, stride), T, fitness);
        if (stats) *stats = m->st;
        return rc;
    });
}

}  // extern "C"
