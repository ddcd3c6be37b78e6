// abi_frontend.hpp -- the front ends that make a matcher's input: include/fls_features.h, fls_features_device.h, fls_preprocess.h,
// fls_ingest.h, and the two calls that attach a front end's device cloud to a matcher.  Host code only.
#pragma once
#include "abi_common.hpp"

extern "C" {

// ---- LOAM feature front-end (include/fls_features.h) ------------------------------------------------------------
fls_status fls_features_create(const fls_feature_params* params, int device_id, fls_features_handle* out) {
    if (!out) return FLS_ERR_INVALID;
    *out = nullptr;
    if (!params) return FLS_ERR_INVALID;
    return create_handle<fls_features>(device_id, out, [&](fls_features& f) { f.p = *params; });
}

void fls_features_destroy(fls_features_handle h) { destroy_handle(h); }

fls_status fls_features_project(fls_features_handle h, const void* raw, size_t n, const fls_point_layout* layout, size_t* n_ordered) {
    if (!h || !layout || (!raw && n)) return FLS_ERR_INVALID;
    return on_device(h, [&] { return h->project(raw, n, *layout, n_ordered); });
}

fls_status fls_features_extract(fls_features_handle h, size_t* n_corner, size_t* n_planar) {
    if (!h) return FLS_ERR_INVALID;
    return on_device(h, [&] { return h->extract(n_corner, n_planar); });
}

size_t fls_features_get(fls_features_handle h, int what, void* out, size_t cap_elems) {
    if (!h) return 0;
    size_t n = 0;  // no device set here: most arrays are on the host already, and each read-back of features_host.hpp sets it itself
    (void)guarded([&]() -> fls_status { n = h->get(what, out, cap_elems); return FLS_OK; });
    return n;
}

fls_status fls_features_get_time(fls_features_handle h, double* project_ms, double* extract_ms) {
    if (!h) return FLS_ERR_INVALID;
    if (project_ms) *project_ms = h->project_ms;
    if (extract_ms) *extract_ms = h->extract_ms;
    return FLS_OK;
}

fls_status fls_features_project_deskew(fls_features_handle h, const void* raw, size_t n, const fls_raw_layout* layout, uint64_t stamp_us,
                                       const uint64_t* imu_t_us, const double* imu_q_xyzw, size_t n_imu, const double T_lidar_to_imu[16], size_t* n_ordered,
                                       int* imu_status) {
    if (!h || !layout || (!raw && n) || !T_lidar_to_imu) return FLS_ERR_INVALID;
    return on_device(h, [&] { return features_project_deskew(*h, raw, n, *layout, stamp_us, imu_t_us, imu_q_xyzw, n_imu, T_lidar_to_imu, n_ordered, imu_status); });
}

// ---- the feature clouds kept on the device and handed to the LoamFull kind (include/fls_features_device.h) ----------------------
int fls_features_device_revision(void) { return FLS_FEATURES_DEVICE_REVISION; }

fls_status fls_features_keep_on_device(fls_features_handle h, int on) {
    if (!h) return FLS_ERR_INVALID;
    const bool want = on != 0;
    if (want != h->resident) {  // (no array of a projection made in the other mode is read in this one)
        h->resident = want;
        h->projected = h->extracted = false;
    }
    return FLS_OK;
}

fls_status fls_features_get_host_bytes(fls_features_handle h, uint64_t* d2h_bytes) {
    if (!h || !d2h_bytes) return FLS_ERR_INVALID;
    *d2h_bytes = h->d2h_bytes;
    return FLS_OK;
}

size_t fls_features_stat(fls_features_handle h, int what) { return (h && what >= 0 && what < 4) ? h->stats[what] : 0; }

fls_status fls_scan_attach_features(fls_handle m, fls_features_handle f, int filtered) {
    if (!m || !f || m->device != f->device) return FLS_ERR_INVALID;
    if (m->kind != FLS_LOAM_FULL || !f->extracted) return FLS_ERR_STATE;
    if (filtered && (!(f->p.corner_voxel_filter_size > 0.f) || !(f->p.planar_voxel_filter_size > 0.f))) return FLS_ERR_STATE;
    return on_device(m, [&]() -> fls_status {
        if (!f->resident) {  // the clouds the default mode left on the host: the ordinary upload
            const std::vector<PtI>& pl = filtered ? f->planar_f : f->planar;
            const std::vector<PtI>& co = filtered ? f->corner_f : f->corner;
            const fls_status rc = m->scan_upload(pl.empty() ? nullptr : &pl[0].x, pl.size(), co.empty() ? nullptr : &co[0].x, co.size(), 4);
            FLS_HIP(hipStreamSynchronize(m->stream));
            return rc;
        }
        const HandoffCloud pl = filtered ? f->rc_planar.filtered() : f->rc_planar.cloud();
        const HandoffCloud co = filtered ? f->rc_corner.filtered() : f->rc_corner.cloud();
        if (pl.n == 0 && co.n == 0) return m->scan_attach_features(pl, co);
        return handoff(*f, m->stream, [&] { return m->scan_attach_features(pl, co); });
    });
}

// ---- per-scan preprocessing: IMU de-skew, range gate, subsample, planar VoxelGrid (include/fls_preprocess.h) --------------------
fls_status fls_preprocess_create(const fls_preprocess_params* params, int device_id, fls_preprocess_handle* out) {
    if (!out) return FLS_ERR_INVALID;
    *out = nullptr;
    if (!params || fls_preprocess::check(*params) != FLS_OK) return FLS_ERR_INVALID;
    return create_handle<fls_preprocess>(device_id, out, [&](fls_preprocess& f) { f.p = *params; });
}

void fls_preprocess_destroy(fls_preprocess_handle h) { destroy_handle(h); }

fls_status fls_preprocess_scan(fls_preprocess_handle h, const void* raw, size_t n, const fls_raw_layout* layout, uint64_t stamp_us, const uint64_t* imu_t_us,
                               const double* imu_q_xyzw, size_t n_imu, fls_preprocess_result* result) {
    if (!h || !layout || (!raw && n) || (result && result->struct_size != sizeof(fls_preprocess_result))) return FLS_ERR_INVALID;
    return on_device(h, [&] { return h->scan(raw, n, *layout, stamp_us, imu_t_us, imu_q_xyzw, n_imu, result); });
}

fls_status fls_preprocess_scan_device(fls_preprocess_handle h, const void* raw, size_t n, const fls_raw_layout* layout, uint64_t stamp_us,
                                      const uint64_t* imu_t_us, const double* imu_q_xyzw, size_t n_imu, fls_preprocess_result* result) {
    if (!h || !layout || (!raw && n) || (result && result->struct_size != sizeof(fls_preprocess_result))) return FLS_ERR_INVALID;
    return on_device(h, [&] { return h->scan(raw, n, *layout, stamp_us, imu_t_us, imu_q_xyzw, n_imu, result, /*on_device=*/true); });
}

size_t fls_preprocess_get(fls_preprocess_handle h, int what, void* out, size_t cap_elems) {
    if (!h) return 0;
    size_t n = 0;
    (void)on_device(h, [&] { n = h->get(what, out, cap_elems); return FLS_OK; });  // (after a device scan the first request of an array downloads it)
    return n;
}

fls_status fls_preprocess_get_host_bytes(fls_preprocess_handle h, uint64_t* d2h_bytes) {
    if (!h || !d2h_bytes) return FLS_ERR_INVALID;
    *d2h_bytes = h->d2h_bytes;
    return FLS_OK;
}

fls_status fls_preprocess_get_time(fls_preprocess_handle h, double* deskew_ms, double* filter_ms) {
    if (!h) return FLS_ERR_INVALID;
    if (deskew_ms) *deskew_ms = h->deskew_ms;
    if (filter_ms) *filter_ms = h->filter_ms;
    return FLS_OK;
}

fls_status fls_scan_attach_preprocessed(fls_handle m, fls_preprocess_handle pre, int what) {
    if (!m || !pre || !pre_cloud_ok(what) || m->device != pre->device) return FLS_ERR_INVALID;
    if (m->kind == FLS_LOAM_FULL || m->is_lane || !pre->scan_done) return FLS_ERR_STATE;
    return on_device(m, [&]() -> fls_status {
        HandoffCloud c;
        const std::vector<PtI>* rows = nullptr;
        if (!pre->device_cloud(what, c, rows))  // the cloud the exact host filter made: the ordinary upload
            return m->scan_upload_raw(rows->empty() ? nullptr : &(*rows)[0].x, rows->size(), nullptr, 0, 4);
        if (c.n == 0) return m->scan_attach_device(c);
        return handoff(*pre, m->stream, [&] { return m->scan_attach_device(c); });
    });
}

// ---- the driver-cloud front end (include/fls_ingest.h) ---------------------------------------------------------------------------
int fls_ingest_revision(void) { return FLS_INGEST_REVISION; }

fls_status fls_ingest_default_layout(int sensor, fls_driver_cloud* out) {
    if (!out || sensor < FLS_SENSOR_VELODYNE || sensor > FLS_SENSOR_NONE) return FLS_ERR_INVALID;
    fls_driver_cloud d{};
    d.struct_size = sizeof(d);
    d.sensor = sensor;
    d.point_step = 32;
    d.is_dense = 1;
    d.x_offset = 0; d.y_offset = 4; d.z_offset = 8; d.intensity_offset = 16;  // PCL_ADD_POINT4D, then the intensity
    switch (sensor) {
        case FLS_SENSOR_VELODYNE: d.ring_offset = 20; d.time_offset = 24; break;
        case FLS_SENSOR_OUSTER: d.time_offset = 20; d.ring_offset = 26; d.point_step = 48; break;  // t, reflectivity, ring, noise, range
        case FLS_SENSOR_LIVOX_AVIA: d.time_offset = 20; d.line_offset = 24; d.tag_offset = 25; break;
        case FLS_SENSOR_ROBOSENSE:
        case FLS_SENSOR_LEISHEN: d.ring_offset = 20; d.time_offset = 24; break;
        case FLS_SENSOR_LIVOX_MID_360: d.tag_offset = 20; d.line_offset = 21; d.time_offset = 24; break;
        default: break;  // pcl::PointXYZI
    }
    *out = d;
    return FLS_OK;
}

fls_status fls_preprocess_scan_driver(fls_preprocess_handle h, const void* msg, size_t n, const fls_driver_cloud* cloud, const fls_ingest_params* ingest,
                                      uint64_t stamp_us, const uint64_t* imu_t_us, const double* imu_q_xyzw, size_t n_imu, int keep_on_device,
                                      fls_preprocess_result* result, uint64_t* stamp_out_us, fls_ingest_info* info) {
    if (!h || !cloud || !ingest || (!msg && n) || (result && result->struct_size != sizeof(fls_preprocess_result)) ||
        (info && info->struct_size != sizeof(fls_ingest_info)))
        return FLS_ERR_INVALID;
    return on_device(h, [&] { return h->scan_driver(msg, n, *cloud, *ingest, stamp_us, imu_t_us, imu_q_xyzw, n_imu, result, keep_on_device != 0, stamp_out_us, info); });
}

fls_status fls_features_project_driver(fls_features_handle h, const void* msg, size_t n, const fls_driver_cloud* cloud, const fls_ingest_params* ingest,
                                       uint64_t stamp_us, const uint64_t* imu_t_us, const double* imu_q_xyzw, size_t n_imu, const double T_lidar_to_imu[16],
                                       size_t* n_ordered, int* imu_status, uint64_t* stamp_out_us, fls_ingest_info* info) {
    if (!h || !cloud || !ingest || (!msg && n) || !T_lidar_to_imu || (info && info->struct_size != sizeof(fls_ingest_info))) return FLS_ERR_INVALID;
    return on_device(h, [&] {
        return features_project_driver(*h, msg, n, *cloud, *ingest, stamp_us, imu_t_us, imu_q_xyzw, n_imu, T_lidar_to_imu, n_ordered, imu_status, stamp_out_us, info);
    });
}

}  // extern "C"
