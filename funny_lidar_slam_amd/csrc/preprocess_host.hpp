// preprocess_host.hpp -- host side of include/fls_preprocess.h: the per-scan IMU segment (GetDataSegment, slerp), SetRefTime, the
// staging of the raw cloud, the launches of kernels_deskew.hpp, the planar VoxelGrid; and fls_features_project_deskew.  Also the host
// side of include/fls_ingest.h: validation of the driver-cloud descriptor, the launches of kernels_ingest.hpp and the summary read-back.
#pragma once
#include "features_host.hpp"
#include "device_voxelgrid.hpp"
#include "kernels_ingest.hpp"
#include "../../include/fls_ingest.h"
#include <cmath>
#include <limits>

namespace fls {

// MotionInterpolator::InterpolateQuaternionSlerp(q0, q1, t0, t1, t) (motion_interpolator.h:108-147), C library acos / sin
inline void deskew_slerp_host(const double* a, const double* b, const uint64_t t0, const uint64_t t1, const uint64_t t, double* q) {
    const double tt = (double)(t - t0) / (double)(t1 - t0);
    const double one = 1.0 - std::numeric_limits<double>::epsilon();
    const double d = (a[0] * b[0] + a[2] * b[2]) + (a[1] * b[1] + a[3] * b[3]);
    const double ad = std::fabs(d);
    double s0, s1;
    if (ad >= one) {
        s0 = 1.0 - tt;
        s1 = tt;
    } else {
        const double th = std::acos(ad), st = std::sin(th);
        s0 = std::sin((1.0 - tt) * th) / st;
        s1 = std::sin(tt * th) / st;
    }
    if (d < 0.0) s1 = -s1;
    for (int c = 0; c < 4; ++c) q[c] = s0 * a[c] + s1 * b[c];
}

// rightmost sample with ts <= t (the reference's backward scan; the caller guarantees ts[0] <= t)
inline size_t deskew_rightmost_le(const uint64_t* ts, const size_t n, const uint64_t t) {
    return size_t(std::upper_bound(ts, ts + n, t) - ts) - 1;
}

// IMUDataSearcher::GetDataSegment(start, end) on t_us[n] (strictly increasing, ts[0] <= start, end <= ts[n-1]).  start >= end: empty.
// Where start and end share one bracket sample the reference's middle loop runs past the deque's end; here the segment is the two ends.
inline void deskew_segment(const uint64_t* ts, const double* qs, const size_t n, const uint64_t start, const uint64_t end, std::vector<uint64_t>& st,
                           std::vector<double>& sq) {
    st.clear();
    sq.clear();
    if (start >= end) return;
    double ql[4], qr[4];
    size_t lb, rb;
    if (ts[0] == start) { lb = 0; std::memcpy(ql, qs, sizeof ql); }
    else { lb = deskew_rightmost_le(ts, n, start); deskew_slerp_host(qs + 4 * lb, qs + 4 * (lb + 1), ts[lb], ts[lb + 1], start, ql); }
    if (ts[n - 1] == end) { rb = n - 1; std::memcpy(qr, qs + 4 * (n - 1), sizeof qr); }
    else { rb = deskew_rightmost_le(ts, n, end); deskew_slerp_host(qs + 4 * rb, qs + 4 * (rb + 1), ts[rb], ts[rb + 1], end, qr); }
    st.push_back(start);
    sq.insert(sq.end(), ql, ql + 4);
    for (size_t k = lb + 1; k < rb; ++k) { st.push_back(ts[k]); sq.insert(sq.end(), qs + 4 * k, qs + 4 * k + 4); }  // strictly between the brackets
    st.push_back(end);
    sq.insert(sq.end(), qr, qr + 4);
}

// one scan's preparation, shared by fls_preprocess_scan and fls_features_project_deskew: validation, time range, IMU status, segment,
// q_ref_inv, and the raw cloud + segment staged in pinned memory for ONE host-to-device copy
struct DeskewScratch {
    PinnedBuf<unsigned char> stage;
    DevBuf<unsigned char> d_in;  // raw bytes | segment t (u64) | segment q (4 doubles)
    DevBuf<float4> d_corr;
    DevBuf<unsigned char> d_flag;
    DevBuf<uint2> d_blk, d_off;
    std::vector<uint64_t> seg_t;
    std::vector<double> seg_q;
    DeskewRawDev L{};
    DeskewParamsDev P{};
    uint64_t start = 0, end = 0;
    int imu_status = FLS_IMU_EMPTY_CLOUD;
    size_t n = 0, raw_bytes = 0, seg_off = 0;

    static bool layout_ok(const fls_raw_layout& l, bool need_ring) {
        if (l.stride_bytes < 16 || (l.stride_bytes & 3u) || (l.xyz_offset & 3u) || (l.intensity_offset & 3u) || (l.time_offset & 3u)) return false;
        if (l.xyz_offset + 12 > l.stride_bytes || l.intensity_offset + 4 > l.stride_bytes || l.time_offset + 4 > l.stride_bytes) return false;
        if (l.ring_bytes > 2 || (need_ring && l.ring_bytes == 0)) return false;
        if (l.ring_bytes && (l.ring_offset + l.ring_bytes > l.stride_bytes || (l.ring_bytes == 2 && (l.ring_offset & 1u)))) return false;
        return true;
    }

    // FLS_OK: imu_status set; with FLS_IMU_OK the stage holds raw + segment and P / L are ready
    fls_status prepare(const void* raw, size_t n_, const fls_raw_layout& l, uint64_t stamp, const uint64_t* it, const double* iq, size_t n_imu,
                       const double* T, bool need_ring) {
        if (!layout_ok(l, need_ring) || (!raw && n_) || !it || !iq || !T || n_imu < 2 || n_ > 0x7FFFFFF0ull) return FLS_ERR_INVALID;
        for (size_t k = 1; k < n_imu; ++k)
            if (!(it[k] > it[k - 1])) return FLS_ERR_INVALID;  // the searcher's deque is in time order (CHECKs of the reference)
        n = n_;
        ingested = false;
        L = DeskewRawDev{l.stride_bytes, l.xyz_offset, l.intensity_offset, l.ring_offset, l.ring_bytes, l.time_offset};
        seg_t.clear();
        seg_q.clear();
        start = end = 0;
        if (n == 0) { imu_status = FLS_IMU_EMPTY_CLOUD; return FLS_OK; }
        raw_bytes = n * l.stride_bytes;
        seg_off = (raw_bytes + 15) & ~size_t(15);
        stage.reserve(seg_off + size_t(kDeskewMaxSeg) * 40);
        std::memcpy(stage.p, raw, raw_bytes);
        // GetLidarPointMinMaxOffsetTime (:554-570)
        const unsigned char* s = stage.p + l.time_offset;
        float mn, mx;
        std::memcpy(&mn, s, 4);
        mx = mn;
        for (size_t k = 0; k < n; ++k) {
            float v;
            std::memcpy(&v, s + k * l.stride_bytes, 4);
            if (!std::isfinite(v)) return FLS_ERR_INVALID;
            if (v < mn) mn = v;
            if (v > mx) mx = v;
        }
        return segment_and_params(mn, mx, stamp, it, iq, n_imu, T);
    }

    // from the time range of the cloud on: IMU status, segment (into the stage at seg_off), q_ref_inv, the extrinsic
    fls_status segment_and_params(const float mn, const float mx, uint64_t stamp, const uint64_t* it, const double* iq, size_t n_imu, const double* T) {
        start = (uint64_t)((int64_t)stamp + deskew_trunc_i64((double)mn * 1.0e6));  // (:89-96)
        end = (uint64_t)((int64_t)stamp + deskew_trunc_i64((double)mx * 1.0e6));
        if (stamp < start) start = stamp;  // (:100-104)
        else if (stamp > end) end = stamp;
        if (it[0] > start) { imu_status = FLS_IMU_DROP; return FLS_OK; }        // (:124-133)
        if (it[n_imu - 1] < end) { imu_status = FLS_IMU_WAIT; return FLS_OK; }  // (:136-141)
        deskew_segment(it, iq, n_imu, start, end, seg_t, seg_q);
        if (seg_t.empty()) { imu_status = FLS_IMU_EMPTY_SEGMENT; return FLS_OK; }
        if (seg_t.size() > size_t(kDeskewMaxSeg)) return FLS_ERR_INVALID;
        imu_status = FLS_IMU_OK;
        std::memcpy(stage.p + seg_off, seg_t.data(), seg_t.size() * 8);
        std::memcpy(stage.p + seg_off + seg_t.size() * 8, seg_q.data(), seg_q.size() * 8);
        // SetRefTime(stamp): the stamp lies inside [start, end], so the bracket exists
        P = DeskewParamsDev{};
        P.n = unsigned(n);
        P.n_seg = int(seg_t.size());
        P.ref_us = stamp;
        const int lr = deskew_bracket((const unsigned long long*)seg_t.data(), P.n_seg, stamp);
        const uint64_t tl = seg_t[size_t(lr)], tr = seg_t[size_t(lr) + 1];
        double qref[4];
        deskew_nlerp(seg_q.data() + 4 * lr, seg_q.data() + 4 * (lr + 1), (double)(stamp - tl) / (double)(tr - tl), qref);
        deskew_inverse(qref, P.qri);
        for (int i = 0; i < 3; ++i) {
            for (int k = 0; k < 3; ++k) P.R[3 * i + k] = T[4 * k + i];
            P.t[i] = T[12 + i];
        }
        return FLS_OK;
    }

    // ---- the driver-cloud front end (include/fls_ingest.h, kernels_ingest.hpp) ---------------------------------------------------
    bool ingested = false;  // the last prepare was prepare_driver: `raw` of the de-skew kernels is d_conv, d_in holds message | segment
    DevBuf<unsigned char> d_conv, d_iflag, d_ring8;  // 32-byte PointXYZIRT rows; keep flags; compact ring array
    DevBuf<int> d_cidx;                              // message index of every converted point
    DevBuf<uint2> d_iblk, d_ioff;
    DevBuf<unsigned> d_ictl;  // tot[2] | first_kept | nonfinite | timeless | pad[3] | first point of ring r, r < 256
    DevBuf<float> d_tb;
    DevBuf<IngestMinMax> d_part;
    DevBuf<IngestMail> d_mail;
    PinnedBuf<IngestMail> h_mail;
    IngestMail mail{};
    size_t n_msg = 0;
    uint64_t stamp_out = 0;

    static bool ingest_check(const fls_driver_cloud& c, const fls_ingest_params& ip, IngestDev& D) {
        if (c.struct_size != sizeof(fls_driver_cloud) || ip.struct_size != sizeof(fls_ingest_params)) return false;
        if (c.sensor < FLS_SENSOR_VELODYNE || c.sensor > FLS_SENSOR_NONE || !std::isfinite(ip.lidar_point_time_scale)) return false;
        const int s = c.sensor;
        const uint64_t step = c.point_step;
        auto fits = [&](uint32_t off, uint32_t bytes) { return uint64_t(off) + bytes <= step; };
        if (step == 0 || !fits(c.x_offset, 4) || !fits(c.y_offset, 4) || !fits(c.z_offset, 4) || !fits(c.intensity_offset, 4)) return false;
        const bool ring16 = s == FLS_SENSOR_VELODYNE || s == FLS_SENSOR_ROBOSENSE || s == FLS_SENSOR_LEISHEN;
        if (ring16 && !fits(c.ring_offset, 2)) return false;
        if (s == FLS_SENSOR_OUSTER && !fits(c.ring_offset, 1)) return false;
        const bool time64 = s == FLS_SENSOR_ROBOSENSE || s == FLS_SENSOR_LEISHEN || s == FLS_SENSOR_LIVOX_MID_360;
        if (s != FLS_SENSOR_NONE && !fits(c.time_offset, time64 ? 8 : 4)) return false;
        if (s == FLS_SENSOR_LIVOX_AVIA && (!fits(c.tag_offset, 1) || !fits(c.line_offset, 1))) return false;
        const bool need_vsn = s == FLS_SENSOR_VELODYNE || s == FLS_SENSOR_NONE;
        if (need_vsn && (ip.vertical_scan_num < 1 || ip.vertical_scan_num > 255)) return false;
        D = IngestDev{};
        D.sensor = s;
        D.drop_nonfinite = c.is_dense ? 0 : 1;
        D.step = c.point_step;
        D.off_x = c.x_offset; D.off_y = c.y_offset; D.off_z = c.z_offset; D.off_i = c.intensity_offset;
        D.off_ring = c.ring_offset; D.off_time = c.time_offset; D.off_tag = c.tag_offset; D.off_line = c.line_offset;
        D.vsn = need_vsn ? ip.vertical_scan_num : 0;
        D.lower_angle = ip.lower_angle;
        D.v_res = ip.v_res;
        D.scale = ip.lidar_point_time_scale;
        return true;
    }

    // static_cast<uint64_t>(double) as x86-64 executes it
    static uint64_t trunc_u64(const double v) {
        if (v >= 9223372036854775808.0) return (uint64_t)deskew_trunc_i64(v - 9223372036854775808.0) ^ 0x8000000000000000ull;
        return (uint64_t)deskew_trunc_i64(v);
    }

    // prepare() for a driver message: the message goes to the device (d_in), the conversion runs there, the summary comes back, and
    // from the time range on everything is prepare()'s.  Afterwards n = the converted count and L = the PointXYZIRT layout.
    fls_status prepare_driver(hipStream_t s, const void* msg, size_t n_, const fls_driver_cloud& c, const fls_ingest_params& ip, uint64_t stamp,
                              const uint64_t* it, const double* iq, size_t n_imu, const double* T) {
        IngestDev D;
        if (!ingest_check(c, ip, D) || (!msg && n_) || !it || !iq || !T || n_imu < 2 || n_ > 0x7FFFFFF0ull ||
            uint64_t(n_) * c.point_step > 0x7FFFFFF0ull)
            return FLS_ERR_INVALID;
        for (size_t k = 1; k < n_imu; ++k)
            if (!(it[k] > it[k - 1])) return FLS_ERR_INVALID;
        n_msg = n_;
        n = 0;
        ingested = true;
        L = DeskewRawDev{32, 0, 16, 20, 1, 24};
        mail = IngestMail{};
        stamp_out = stamp;
        seg_t.clear();
        seg_q.clear();
        start = end = 0;
        imu_status = FLS_IMU_EMPTY_CLOUD;
        if (n_msg == 0) return FLS_OK;
        D.n = unsigned(n_msg);
        raw_bytes = n_msg * c.point_step;
        seg_off = (raw_bytes + 15) & ~size_t(15);
        const size_t all = seg_off + size_t(kDeskewMaxSeg) * 40;
        stage.reserve(all);
        d_in.reserve(all);
        std::memcpy(stage.p, msg, raw_bytes);
        const unsigned nb = unsigned((n_msg + kIngestThreads - 1) / kIngestThreads);
        d_conv.reserve(32 * n_msg); d_iflag.reserve(n_msg); d_ring8.reserve(n_msg); d_cidx.reserve(n_msg); d_tb.reserve(n_msg);
        d_iblk.reserve(nb); d_ioff.reserve(nb); d_part.reserve(nb);
        d_ictl.reserve(8 + 256); d_mail.reserve(1); h_mail.reserve(1);
        unsigned *tot = d_ictl.p, *first_kept = d_ictl.p + 2, *nonfinite = d_ictl.p + 3, *timeless = d_ictl.p + 4, *ring_first = d_ictl.p + 8;
        uint4* rows = (uint4*)d_conv.p;
        FLS_HIP(hipMemcpyAsync(d_in.p, stage.p, raw_bytes, hipMemcpyHostToDevice, s));
        FLS_HIP(hipMemsetAsync(d_ictl.p, 0, 8 * sizeof(unsigned), s));
        FLS_HIP(hipMemsetAsync(first_kept, 0xFF, sizeof(unsigned), s));
        hipLaunchKernelGGL(ingest_count_kernel, dim3(nb), dim3(kIngestThreads), 0, s, d_in.p, D, d_iflag.p, d_iblk.p, first_kept);
        hipLaunchKernelGGL(deskew_scan_kernel, dim3(1), dim3(1024), 0, s, d_iblk.p, nb, d_ioff.p, tot);
        hipLaunchKernelGGL(ingest_write_kernel, dim3(nb), dim3(kIngestThreads), 0, s, d_in.p, D, d_iflag.p, d_ioff.p, first_kept, rows, d_cidx.p, d_ring8.p);
        if (D.vsn) {  // Velodyne / None: ComputePointOffsetTime where the last converted time is <= 0 (decided on the device)
            hipLaunchKernelGGL(ingest_ring_first_kernel, dim3(unsigned(D.vsn)), dim3(kIngestRingThreads), 0, s, D, tot, rows, d_ring8.p, ring_first, timeless);
            hipLaunchKernelGGL(ingest_base_kernel, dim3(nb), dim3(kIngestThreads), 0, s, D, tot, rows, ring_first, timeless, d_tb.p);
            hipLaunchKernelGGL(ingest_ring_scan_kernel, dim3(unsigned(D.vsn)), dim3(kIngestRingThreads), 0, s, D, tot, rows, d_ring8.p, ring_first, timeless,
                               d_tb.p);
        }
        hipLaunchKernelGGL(ingest_minmax_kernel, dim3(nb), dim3(kIngestThreads), 0, s, tot, rows, d_part.p, nonfinite);
        hipLaunchKernelGGL(ingest_summary_kernel, dim3(1), dim3(1024), 0, s, D, d_in.p, tot, rows, d_part.p, nb, first_kept, nonfinite, timeless, d_mail.p);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipMemcpyAsync(h_mail.p, d_mail.p, sizeof(IngestMail), hipMemcpyDeviceToHost, s));
        FLS_HIP(hipStreamSynchronize(s));
        mail = *h_mail.p;
        n = mail.n_conv;
        if (c.sensor == FLS_SENSOR_ROBOSENSE && n) stamp_out = trunc_u64(mail.t0 * 1.0e6);  // (:376)
        if (n == 0) return FLS_OK;  // (the reference reads points.back() / [0] of the empty cloud: undefined there, EMPTY_CLOUD here)
        if (mail.nonfinite) return FLS_ERR_INVALID;
        return segment_and_params(mail.t_min, mail.t_max, stamp_out, it, iq, n_imu, T);
    }
    void fill_info(fls_ingest_info* info) const {
        if (!info) return;
        info->timeless = int32_t(mail.timeless);
        info->n_message = n_msg;
        info->n_converted = n;
        info->time_min = mail.t_min; info->time_max = mail.t_max; info->time_last = mail.t_last;
        info->reserved = 0;
        info->t0 = mail.t0;
    }
    // the cloud the de-skew and projection kernels read (valid after upload_and_deskew)
    const unsigned char* raw_dev() const { return ingested ? d_conv.p : d_in.p; }

    // H2D of the stage (after prepare_driver: of the segment only), pass 1 (gate + de-skew of every point); returns the block count
    unsigned upload_and_deskew(hipStream_t s, bool gate, float min_d, float max_d, unsigned span) {
        P.gate = gate ? 1 : 0;
        P.min_dist = min_d;
        P.max_dist = max_d;
        P.jump_span = span;
        const size_t bytes = seg_off + seg_t.size() * 40;
        const unsigned nb = unsigned((n + kDeskewThreads - 1) / kDeskewThreads);
        d_in.reserve(bytes);
        d_corr.reserve(n);
        d_flag.reserve(n);
        d_blk.reserve(nb);
        d_off.reserve(nb);
        if (ingested) FLS_HIP(hipMemcpyAsync(d_in.p + seg_off, stage.p + seg_off, seg_t.size() * 40, hipMemcpyHostToDevice, s));
        else FLS_HIP(hipMemcpyAsync(d_in.p, stage.p, bytes, hipMemcpyHostToDevice, s));
        const auto* st = (const unsigned long long*)(d_in.p + seg_off);
        const auto* sq = (const double*)(d_in.p + seg_off + seg_t.size() * 8);
        hipLaunchKernelGGL(deskew_point_kernel, dim3(nb), dim3(kDeskewThreads), seg_t.size() * 40, s, raw_dev(), L, P, st, sq, d_corr.p, d_flag.p, d_blk.p);
        FLS_HIP(hipGetLastError());
        return nb;
    }
};

}  // namespace fls

struct fls_preprocess {
    fls_preprocess_params p{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    fls::DeskewScratch ds;
    fls::DeviceVoxelGrid vg;
    fls::DevBuf<float4> d_ordered;
    fls::DevBuf<int> d_ordered_idx;
    fls::DevBuf<float> d_planar;  // x | y | z | i, row stride = capacity
    fls::DevBuf<unsigned> d_tot;
    fls::PinnedBuf<unsigned> h_tot;
    std::vector<fls::PtI> ordered, planar, planar_f;
    std::vector<int> ordered_idx;
    std::vector<float> tmp;
    double deskew_ms = 0.0, filter_ms = 0.0;
    bool filter_on_device = false;
    // the last scan: counts (all the host learns from fls_preprocess_scan_device), the row stride of d_planar, and which host arrays
    // have not been downloaded yet (fls_preprocess_get fetches them on first request)
    size_t n_ordered = 0, n_planar = 0, n_planar_f = 0, planar_cap = 0;
    bool stale_ordered = false, stale_idx = false, stale_planar = false, stale_planar_f = false;
    // fls_preprocess_scan_driver: host copies of the converted cloud / its message indices, downloaded on their first request
    std::vector<unsigned char> converted;
    std::vector<int> converted_idx;
    bool stale_conv = false, stale_cidx = false;
    bool scan_done = false;      // a scan has completed with clouds (not DROP / WAIT, not an invalid call)
    uint64_t d2h_bytes = 0;      // device -> host copies on behalf of the last scan so far
    // hand-off (fls_scan_attach_preprocessed): ready = "everything queued on this stream so far", recorded per attach and waited for
    // by the matcher's stream; consumed[k] = a matcher's copy kernel has read this handle's buffers, waited for by the next scan
    hipEvent_t ev_ready = nullptr;
    std::vector<hipEvent_t> consumed;
    size_t n_consumed = 0;

    ~fls_preprocess() {
        for (size_t k = 0; k < n_consumed; ++k) (void)hipEventSynchronize(consumed[k]);  // (the buffers below are still being read)
        for (auto e : consumed) if (e) (void)hipEventDestroy(e);
        if (ev_ready) (void)hipEventDestroy(ev_ready);
        for (auto e : ev) if (e) (void)hipEventDestroy(e);
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
    }

    static fls_status check(const fls_preprocess_params& q) {
        if (q.struct_size != sizeof(fls_preprocess_params) || q.lidar_point_jump_span < 1 || !(q.planar_voxel_filter_size >= 0.f)) return FLS_ERR_INVALID;
        for (double v : q.T_lidar_to_imu) if (!std::isfinite(v)) return FLS_ERR_INVALID;
        return FLS_OK;
    }

    fls_status init() {
        if (check(p) != FLS_OK) return FLS_ERR_INVALID;
        FLS_HIP(hipSetDevice(device));
        FLS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        for (auto& e : ev) FLS_HIP(hipEventCreate(&e));
        FLS_HIP(hipEventCreateWithFlags(&ev_ready, hipEventDisableTiming));
        d_tot.reserve(2);
        h_tot.reserve(2);
        return FLS_OK;
    }

    void clear() {
        ordered.clear(); planar.clear(); planar_f.clear(); ordered_idx.clear();
        deskew_ms = filter_ms = 0.0;
        filter_on_device = false;
        n_ordered = n_planar = n_planar_f = 0;
        stale_ordered = stale_idx = stale_planar = stale_planar_f = false;
        stale_conv = stale_cidx = false;
        converted.clear(); converted_idx.clear();
        scan_done = false;
        d2h_bytes = 0;
    }

    // the device -> host copies of the clouds: queued by fls_preprocess_scan, or by the first fls_preprocess_get after a device scan
    void enqueue_ordered() {
        ordered.resize(n_ordered);
        if (n_ordered) FLS_HIP(hipMemcpyAsync(ordered.data(), d_ordered.p, n_ordered * sizeof(float4), hipMemcpyDeviceToHost, stream));
        d2h_bytes += n_ordered * sizeof(float4);
        stale_ordered = false;
    }
    void enqueue_ordered_idx() {
        ordered_idx.resize(n_ordered);
        if (n_ordered) FLS_HIP(hipMemcpyAsync(ordered_idx.data(), d_ordered_idx.p, n_ordered * sizeof(int), hipMemcpyDeviceToHost, stream));
        d2h_bytes += n_ordered * sizeof(int);
        stale_idx = false;
    }
    void enqueue_planar() {
        const size_t np = n_planar;
        planar.resize(np);
        if (np) {
            tmp.resize(4 * np);
            for (int a = 0; a < 4; ++a)
                FLS_HIP(hipMemcpyAsync(tmp.data() + size_t(a) * np, d_planar.p + size_t(a) * planar_cap, np * sizeof(float), hipMemcpyDeviceToHost, stream));
        }
        d2h_bytes += 4 * np * sizeof(float);
    }
    void finish_planar() {  // after the stream has drained
        const size_t np = n_planar;
        for (size_t i = 0; i < np; ++i) planar[i] = fls::PtI{tmp[i], tmp[np + i], tmp[2 * np + i], tmp[3 * np + i]};
        stale_planar = false;
    }
    void fetch_planar_f() {
        std::vector<float> t2;
        planar_f = vg.download(stream, t2);
        d2h_bytes += planar_f.size() * sizeof(fls::PtI);
        stale_planar_f = false;
    }

    // on_device: fls_preprocess_scan_device -- the clouds stay in d_ordered / d_ordered_idx / d_planar / the VoxelGrid's output
    fls_status scan(const void* raw, size_t n, const fls_raw_layout& L, uint64_t stamp, const uint64_t* it, const double* iq, size_t n_imu,
                    fls_preprocess_result* r, const bool on_device = false) {
        clear();
        const fls_status rc = ds.prepare(raw, n, L, stamp, it, iq, n_imu, p.T_lidar_to_imu, false);
        if (rc != FLS_OK) return rc;
        return finish_scan(r, on_device);
    }

    // fls_preprocess_scan_driver: the conversion in front, then the same scan on the converted cloud
    fls_status scan_driver(const void* msg, size_t n_msg, const fls_driver_cloud& c, const fls_ingest_params& ip, uint64_t stamp, const uint64_t* it,
                           const double* iq, size_t n_imu, fls_preprocess_result* r, const bool on_device, uint64_t* stamp_out, fls_ingest_info* info) {
        clear();
        const fls_status rc = ds.prepare_driver(stream, msg, n_msg, c, ip, stamp, it, iq, n_imu, p.T_lidar_to_imu);
        if (rc != FLS_OK) return rc;
        d2h_bytes += sizeof(fls::IngestMail);
        if (stamp_out) *stamp_out = ds.stamp_out;
        ds.fill_info(info);
        stale_conv = stale_cidx = true;
        return finish_scan(r, on_device);
    }

    // after ds.prepare / ds.prepare_driver succeeded: the de-skew, the compaction, the planar VoxelGrid, the report
    fls_status finish_scan(fls_preprocess_result* r, const bool on_device) {
        const size_t n = ds.n;
        auto report = [&](fls_status s) {
            if (r) {
                r->imu_status = ds.imu_status;
                r->cloud_start_us = ds.start; r->cloud_end_us = ds.end;
                r->n_raw = n; r->n_ordered = n_ordered; r->n_planar = n_planar; r->n_planar_filtered = n_planar_f;
                r->n_segment = ds.seg_t.size();
                r->filter_on_device = filter_on_device ? 1 : 0;
                r->reserved = 0;
            }
            return s;
        };
        if (ds.imu_status == FLS_IMU_DROP || ds.imu_status == FLS_IMU_WAIT) return report(FLS_ERR_STATE);
        scan_done = true;
        if (ds.imu_status != FLS_IMU_OK) return report(FLS_OK);
        const size_t cap = n;
        d_ordered.reserve(n); d_ordered_idx.reserve(n); d_planar.reserve(4 * cap);
        planar_cap = cap;
        // a matcher may still be copying the previous scan out of these buffers (and out of the VoxelGrid's): this scan's writes wait
        for (size_t k = 0; k < n_consumed; ++k) FLS_HIP(hipStreamWaitEvent(stream, consumed[k], 0));
        n_consumed = 0;
        FLS_HIP(hipEventRecord(ev[0], stream));
        const unsigned nb = ds.upload_and_deskew(stream, true, p.min_distance, p.max_distance, unsigned(p.lidar_point_jump_span));
        hipLaunchKernelGGL(fls::deskew_scan_kernel, dim3(1), dim3(1024), 0, stream, ds.d_blk.p, nb, ds.d_off.p, d_tot.p);
        hipLaunchKernelGGL(fls::deskew_write_kernel, dim3(nb), dim3(fls::kDeskewThreads), 0, stream, ds.d_flag.p, ds.d_corr.p, unsigned(n), ds.d_off.p,
                           d_ordered.p, d_ordered_idx.p, d_planar.p, cap);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipEventRecord(ev[1], stream));
        FLS_HIP(hipMemcpyAsync(h_tot.p, d_tot.p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        d2h_bytes += 2 * sizeof(unsigned);
        n_ordered = h_tot.p[0];
        n_planar = h_tot.p[1];
        const size_t np = n_planar;
        if (on_device) {
            stale_ordered = stale_idx = stale_planar = true;
        } else {
            enqueue_ordered();
            enqueue_ordered_idx();
            enqueue_planar();
        }
        bool vg_ok = false;
        if (np && p.planar_voxel_filter_size > 0.f) {
            FLS_HIP(hipEventRecord(ev[2], stream));
            vg_ok = fls::device_voxelgrid_mode() != 0 &&
                    vg.run(d_planar.p, d_planar.p + cap, d_planar.p + 2 * cap, d_planar.p + 3 * cap, np, p.planar_voxel_filter_size, stream);
            FLS_HIP(hipEventRecord(ev[3], stream));
        }
        FLS_HIP(hipStreamSynchronize(stream));
        if (!on_device) finish_planar();
        float ms = 0.f;
        FLS_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        deskew_ms = ms;
        if (np && p.planar_voxel_filter_size > 0.f) {
            FLS_HIP(hipEventElapsedTime(&ms, ev[2], ev[3]));
            filter_ms = ms;
            if (vg_ok) {
                filter_on_device = true;
                n_planar_f = vg.n_out;
                if (on_device) stale_planar_f = true; else fetch_planar_f();
            } else {
                fetch(FLS_PRE_PLANAR);  // (a device scan the VoxelGrid declined: the exact host filter needs the cloud here)
                planar_f = fls::voxel_grid_strided(&planar[0].x, np, 4, p.planar_voxel_filter_size);  // the exact host filter (SourceFilter's fallback)
                n_planar_f = planar_f.size();
            }
        }
        return report(FLS_OK);
    }

    // make the host copy of one array current (no-op unless the last scan left it on the device)
    void fetch(int what) {
        switch (what) {
            case FLS_PRE_ORDERED: if (stale_ordered) { enqueue_ordered(); FLS_HIP(hipStreamSynchronize(stream)); } break;
            case FLS_PRE_ORDERED_INDEX: if (stale_idx) { enqueue_ordered_idx(); FLS_HIP(hipStreamSynchronize(stream)); } break;
            case FLS_PRE_PLANAR: if (stale_planar) { enqueue_planar(); FLS_HIP(hipStreamSynchronize(stream)); finish_planar(); } break;
            case FLS_PRE_PLANAR_FILTERED: if (stale_planar_f) fetch_planar_f(); break;
            case FLS_PRE_CONVERTED:
                if (stale_conv) {
                    converted.resize(32 * ds.n);
                    if (ds.n) FLS_HIP(hipMemcpyAsync(converted.data(), ds.d_conv.p, 32 * ds.n, hipMemcpyDeviceToHost, stream));
                    FLS_HIP(hipStreamSynchronize(stream));
                    d2h_bytes += 32 * ds.n;
                    stale_conv = false;
                }
                break;
            case FLS_PRE_CONVERTED_INDEX:
                if (stale_cidx) {
                    converted_idx.resize(ds.n);
                    if (ds.n) FLS_HIP(hipMemcpyAsync(converted_idx.data(), ds.d_cidx.p, ds.n * sizeof(int), hipMemcpyDeviceToHost, stream));
                    FLS_HIP(hipStreamSynchronize(stream));
                    d2h_bytes += ds.n * sizeof(int);
                    stale_cidx = false;
                }
                break;
            default: break;
        }
    }

    // where a cloud of the last scan lies on the device (fls_scan_attach_preprocessed); false: only the host has it (the planar
    // cloud the host filter made) -- `host_rows` then
    bool device_cloud(int what, fls::HandoffCloud& c, const std::vector<fls::PtI>*& host_rows) const {
        c = fls::HandoffCloud{};
        host_rows = nullptr;
        if (what == FLS_PRE_ORDERED) { c.rows = d_ordered.p; c.n = n_ordered; return true; }
        if (what == FLS_PRE_PLANAR) {
            c.x = d_planar.p; c.y = d_planar.p + planar_cap; c.z = d_planar.p + 2 * planar_cap; c.in = d_planar.p + 3 * planar_cap; c.n = n_planar;
            return true;
        }
        if (n_planar_f == 0 || filter_on_device) { c.x = vg.ox(); c.y = vg.oy(); c.z = vg.oz(); c.in = vg.oi(); c.n = n_planar_f; return true; }
        host_rows = &planar_f;
        return false;
    }
    hipEvent_t next_consumed_event() {
        if (n_consumed == consumed.size()) {
            hipEvent_t e = nullptr;
            FLS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            consumed.push_back(e);
        }
        return consumed[n_consumed++];
    }

    template <class T>
    static size_t copy_out(const T* v, size_t n, void* out, size_t cap) {
        if (out && n) std::memcpy(out, v, std::min(cap, n) * sizeof(T));
        return n;
    }
    size_t get(int what, void* out, size_t cap) {
        if (out) fetch(what);
        switch (what) {
            case FLS_PRE_ORDERED: return copy_out(ordered.data(), n_ordered, out, cap);
            case FLS_PRE_ORDERED_INDEX: return copy_out(ordered_idx.data(), n_ordered, out, cap);
            case FLS_PRE_PLANAR: return copy_out(planar.data(), n_planar, out, cap);
            case FLS_PRE_PLANAR_FILTERED: return copy_out(planar_f.data(), n_planar_f, out, cap);
            case FLS_PRE_CONVERTED: {
                const size_t m = converted.size() / 32;
                if (out && m) std::memcpy(out, converted.data(), std::min(cap, m) * 32);
                return (stale_conv || !converted.empty()) ? ds.n : 0;
            }
            case FLS_PRE_CONVERTED_INDEX: return (stale_cidx || !converted_idx.empty()) ? copy_out(converted_idx.data(), ds.n, out, cap) : 0;
            case FLS_PRE_SEGMENT_T: return copy_out(ds.seg_t.data(), ds.seg_t.size(), out, cap);
            case FLS_PRE_SEGMENT_Q: {
                const size_t m = ds.seg_t.size();
                if (out && m) std::memcpy(out, ds.seg_q.data(), std::min(cap, m) * 4 * sizeof(double));
                return m;
            }
            default: return 0;
        }
    }
};

// fls_features_project_deskew: pass 1 without the gate (every point's ProcessPoint), then the projection where only points whose
// de-skew succeeded compete for their cell, the usual ring compaction, and the corrected xyz into the ordered cloud
inline fls_status features_project_prepared(fls_features& f, size_t* n_ordered, int* imu_status);

inline fls_status features_project_deskew(fls_features& f, const void* raw, size_t n, const fls_raw_layout& L, uint64_t stamp, const uint64_t* it,
                                          const double* iq, size_t n_imu, const double* T, size_t* n_ordered, int* imu_status) {
    if (!f.deskew) f.deskew = std::make_shared<fls::DeskewScratch>();
    const fls_status rc = f.deskew->prepare(raw, n, L, stamp, it, iq, n_imu, T, true);
    if (rc != FLS_OK) return rc;
    return features_project_prepared(f, n_ordered, imu_status);
}

// fls_features_project_driver: the conversion in front (on the feature handle's stream), then the same projection
inline fls_status features_project_driver(fls_features& f, const void* msg, size_t n, const fls_driver_cloud& c, const fls_ingest_params& ip, uint64_t stamp,
                                          const uint64_t* it, const double* iq, size_t n_imu, const double* T, size_t* n_ordered, int* imu_status,
                                          uint64_t* stamp_out, fls_ingest_info* info) {
    if (!f.deskew) f.deskew = std::make_shared<fls::DeskewScratch>();
    const fls_status rc = f.deskew->prepare_driver(f.stream, msg, n, c, ip, stamp, it, iq, n_imu, T);
    if (rc != FLS_OK) return rc;
    if (stamp_out) *stamp_out = f.deskew->stamp_out;
    f.deskew->fill_info(info);
    const fls_status prc = features_project_prepared(f, n_ordered, imu_status);
    if (n) f.d2h_bytes += sizeof(fls::IngestMail);  // (the conversion's summary, read back before the projection)
    return prc;
}

// after ds.prepare / ds.prepare_driver succeeded
inline fls_status features_project_prepared(fls_features& f, size_t* n_ordered, int* imu_status) {
    fls::DeskewScratch& ds = *f.deskew;
    const size_t n = ds.n;
    const fls::DeskewRawDev L{ds.L};
    if (imu_status) *imu_status = ds.imu_status;
    f.begin_projection();
    f.N = 0;
    f.ordered.clear(); f.depth.clear(); f.col.clear();
    if (n_ordered) *n_ordered = 0;
    if (ds.imu_status == FLS_IMU_DROP || ds.imu_status == FLS_IMU_WAIT) return FLS_ERR_STATE;
    f.n_raw = n;
    const fls::FeatParamsDev& pd = f.pd;
    const size_t cells = size_t(pd.rows) * size_t(pd.cols);
    // feat_compact_kernel reads the ring field as a uint16 it does not use: point it at the xyz (in bounds for any ring width)
    f.layout = fls::RawLayoutDev{L.stride, L.off_xyz, L.off_i, L.off_xyz};
    FLS_HIP(hipEventRecord(f.ev[0], f.stream));
    FLS_HIP(hipMemsetAsync(f.d_owner.p, 0xFF, cells * sizeof(unsigned), f.stream));
    if (ds.imu_status == FLS_IMU_OK) {
        ds.upload_and_deskew(f.stream, false, pd.min_dist, pd.max_dist, 1u);
        hipLaunchKernelGGL(fls::feat_project_deskew_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, f.stream, ds.raw_dev(), unsigned(n), ds.L, pd,
                           ds.d_flag.p, f.d_owner.p);
    }
    // (EMPTY_SEGMENT / EMPTY_CLOUD: every ProcessPoint fails, no cell is claimed; the compaction runs on the empty image)
    const unsigned char* raw_dev = ds.imu_status == FLS_IMU_OK ? ds.raw_dev() : nullptr;
    hipLaunchKernelGGL(fls::feat_count_kernel, dim3(unsigned(pd.rows)), dim3(256), 0, f.stream, f.d_owner.p, pd, f.d_row_count.p);
    hipLaunchKernelGGL(fls::feat_compact_kernel, dim3(unsigned(pd.rows)), dim3(256), 0, f.stream, raw_dev, f.layout, f.d_owner.p, pd, f.d_row_count.p,
                       f.d_ordered.p, f.d_depth.p, f.d_col.p, f.d_raw_index.p, f.d_valid.p, f.d_row_start.p, f.d_row_end.p, f.d_n.p);
    if (ds.imu_status == FLS_IMU_OK)
        hipLaunchKernelGGL(fls::deskew_apply_kernel, dim3(unsigned((cells + 255) / 256)), dim3(256), 0, f.stream, f.d_n.p, f.d_raw_index.p, ds.d_corr.p,
                           f.d_ordered.p);
    FLS_HIP(hipGetLastError());
    return f.finish_projection(n_ordered);  // (the read-back every projection shares)
}
