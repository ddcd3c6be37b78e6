// abi_stores.hpp -- the device stores: include/fls_keyframes.h and fls_localmap.h.  Host code only.  Their size is the caller's to decide, so
// every call here that may allocate reports a failed device allocation as FLS_ERR_NOMEM (on_device_nomem, abi_common.hpp).
#pragma once
#include "abi_common.hpp"

namespace {
bool kf_leaf_ok(float leaf) { return std::isfinite(leaf) && leaf >= 0.f; }
bool kf_ids_ok(const fls_keyframes& h, const int32_t* ids, size_t n) {
    for (size_t k = 0; k < n; ++k)
        if (!h.valid_id(ids[k])) return false;
    return true;
}
bool lm_grid_ok(double g) { return std::isfinite(g) && g > 0.0; }
bool lm_pose_ok(const double* T) { return T && std::isfinite(T[12]) && std::isfinite(T[13]) && std::isfinite(T[14]); }
}  // namespace

extern "C" {

// ---- the device keyframe store (include/fls_keyframes.h) --------------------------------------------------------------------------
int fls_keyframes_revision(void) { return FLS_KEYFRAMES_REVISION; }

fls_status fls_keyframes_create(int device_id, fls_keyframes_handle* out) {
    if (!out) return FLS_ERR_INVALID;
    *out = nullptr;
    return create_handle<fls_keyframes>(device_id, out, [](fls_keyframes&) {}, Guard::kNomem);
}

void fls_keyframes_destroy(fls_keyframes_handle h) { destroy_handle(h); }

fls_status fls_keyframes_add(fls_keyframes_handle h, const float* pts, size_t n, int stride, int32_t* id) {
    if (!h || !id || (!pts && n) || stride < 3) return FLS_ERR_INVALID;
    return on_device_nomem(h, [&] { return h->add(pts, n, stride, id); });
}

fls_status fls_keyframes_add_preprocessed(fls_keyframes_handle h, fls_preprocess_handle pre, int what, int32_t* id) {
    if (!h || !pre || !id || !pre_cloud_ok(what) || h->device != pre->device) return FLS_ERR_INVALID;
    if (!pre->scan_done) return FLS_ERR_STATE;
    return on_device_nomem(h, [&] { return h->add_preprocessed(*pre, what, id); });
}

size_t fls_keyframes_count(fls_keyframes_handle h) { return h ? h->kf.size() : 0; }

fls_status fls_keyframes_get(fls_keyframes_handle h, int32_t id, float leaf, float* out, size_t cap, size_t* n_out) {
    if (!h || !n_out || (cap && !out) || !kf_leaf_ok(leaf) || !h->valid_id(id)) return FLS_ERR_INVALID;
    *n_out = 0;
    return on_device_nomem(h, [&] { return h->get(id, leaf, out, cap, n_out); });
}

fls_status fls_keyframes_merge(fls_keyframes_handle h, const int32_t* ids, const double* poses, size_t n_ids, float leaf_each, float leaf_final, float* out,
                               size_t cap, size_t* n_out) {
    if (!h || !n_out || (n_ids && (!ids || !poses)) || (cap && !out) || !kf_leaf_ok(leaf_each) || !kf_leaf_ok(leaf_final) || !kf_ids_ok(*h, ids, n_ids))
        return FLS_ERR_INVALID;
    *n_out = 0;
    return on_device_nomem(h, [&] { return h->merge(ids, poses, n_ids, leaf_each, leaf_final, out, cap, n_out); });
}

fls_status fls_keyframes_loop_match(fls_keyframes_handle h, const int32_t* src_ids, const double* src_poses, size_t n_src, const int32_t* tgt_ids,
                                    const double* tgt_poses, size_t n_tgt, double T[16], float* fitness, fls_loop_stats* stats) {
    if (!h || !T || !fitness || (n_src && (!src_ids || !src_poses)) || (n_tgt && (!tgt_ids || !tgt_poses)) || !kf_ids_ok(*h, src_ids, n_src) ||
        !kf_ids_ok(*h, tgt_ids, n_tgt))
        return FLS_ERR_INVALID;
    std::vector<float> src, tgt;
    const fls_status rc = on_device_nomem(h, [&] {
        size_t n = 0;  // GetSubMap's leaf (loop_closure.cpp:219)
        const fls_status a = h->merge(src_ids, src_poses, n_src, 0.2f, 0.f, nullptr, 0, &n, &src);
        return a != FLS_OK ? a : h->merge(tgt_ids, tgt_poses, n_tgt, 0.2f, 0.f, nullptr, 0, &n, &tgt);
    });
    if (rc != FLS_OK) return rc;
    return fls_loop_match(h->device, src.data(), src.size() / 4, tgt.data(), tgt.size() / 4, 4, T, fitness, stats);
}

size_t fls_keyframes_stat(fls_keyframes_handle h, int slot) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);  // outside any guard: stat() reads counters and one event time and does not throw
    return h->stat(slot);
}

// ---- the device local-map source (include/fls_localmap.h) ------------------------------------------------------------------------
int fls_localmap_revision(void) { return FLS_LOCALMAP_REVISION; }

fls_status fls_localmap_create(int device_id, fls_localmap_handle* out) {
    if (!out) return FLS_ERR_INVALID;
    *out = nullptr;
    return create_handle<fls_localmap>(device_id, out, [](fls_localmap&) {}, Guard::kNomem);
}

void fls_localmap_destroy(fls_localmap_handle h) { destroy_handle(h); }

fls_status fls_localmap_set_global(fls_localmap_handle h, const float* pts, size_t n, int stride, float leaf, size_t* n_stored) {
    if (!h || (!pts && n) || stride < 3 || !kf_leaf_ok(leaf) || n > kLmMaxPoints) return FLS_ERR_INVALID;
    return on_device_nomem(h, [&] { return h->set_global(pts, n, stride, leaf, n_stored); });
}

fls_status fls_localmap_crop(fls_localmap_handle h, const double pose[16], int force, int* updated, size_t* n_local) {
    if (!h || !updated || !n_local || !lm_pose_ok(pose)) return FLS_ERR_INVALID;
    if (!h->global) return FLS_ERR_STATE;
    return on_device_nomem(h, [&] { return h->crop(pose, force, updated, n_local); });
}

fls_status fls_localmap_split(fls_localmap_handle h, double grid_size, size_t* n_tiles) {
    if (!h || !n_tiles || !lm_grid_ok(grid_size)) return FLS_ERR_INVALID;
    if (!h->global) return FLS_ERR_STATE;
    return on_device_nomem(h, [&] { return h->split(grid_size, n_tiles); });
}

fls_status fls_localmap_add_tile(fls_localmap_handle h, double grid_size, int32_t gx, int32_t gy, const float* pts, size_t n, int stride) {
    if (!h || (!pts && n) || stride < 3 || !lm_grid_ok(grid_size) || n > kLmMaxPoints || (h->grid_size != 0.0 && h->grid_size != grid_size)) return FLS_ERR_INVALID;
    return on_device_nomem(h, [&] { return h->add_tile(grid_size, gx, gy, pts, n, stride); });
}

// (fls_localmap_tiles and fls_localmap_reset run unguarded and set no device: they touch the host-side tile list and counters only)
fls_status fls_localmap_tiles(fls_localmap_handle h, int32_t* gxgy, uint32_t* counts, size_t cap, size_t* n_tiles) {
    if (!h || !n_tiles || (cap && (!gxgy || !counts))) return FLS_ERR_INVALID;
    return h->list_tiles(gxgy, counts, cap, n_tiles);
}

fls_status fls_localmap_get_tile(fls_localmap_handle h, int32_t gx, int32_t gy, float leaf, float* out, size_t cap, size_t* n_out) {
    if (!h || !n_out || (cap && !out) || !kf_leaf_ok(leaf) || !h->tiles.count(LmTileKey{gx, gy})) return FLS_ERR_INVALID;
    *n_out = 0;
    return on_device_nomem(h, [&] { return h->get_tile(gx, gy, leaf, out, cap, n_out); });
}

fls_status fls_localmap_load_tiles(fls_localmap_handle h, const double pose[16], float leaf, int* updated, size_t* n_local) {
    if (!h || !updated || !n_local || !lm_pose_ok(pose) || !kf_leaf_ok(leaf)) return FLS_ERR_INVALID;
    if (h->tiles.empty()) return FLS_ERR_STATE;
    return on_device_nomem(h, [&] { return h->load_tiles(pose, leaf, updated, n_local); });
}

fls_status fls_localmap_reset(fls_localmap_handle h) {
    if (!h) return FLS_ERR_INVALID;
    h->reset();
    return FLS_OK;
}

fls_status fls_localmap_get_local(fls_localmap_handle h, float* out, size_t cap, size_t* n_out) {
    if (!h || !n_out || (cap && !out)) return FLS_ERR_INVALID;
    *n_out = 0;
    return on_device_nomem(h, [&] { return h->get_local(out, cap, n_out); });
}

fls_status fls_add_localmap_to_local_map(fls_handle m, fls_localmap_handle h) {
    if (!m || !h || m->device != h->device) return FLS_ERR_INVALID;
    if (h->n_local == 0) return FLS_ERR_STATE;
    return on_device_nomem(m, [&] { return h->add_to(*m); });
}

size_t fls_localmap_stat(fls_localmap_handle h, int slot) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);  // outside any guard, as fls_keyframes_stat
    return h->stat(slot);
}

}  // extern "C"
