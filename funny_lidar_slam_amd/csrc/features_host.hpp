// features_host.hpp -- host side of the LOAM feature front-end (include/fls_features.h): owns the device buffers,
// launches kernels_features.hpp, keeps the PointcloudCluster fields the reference's classes fill.
#pragma once
#include "host_maps.hpp"
#include "kernels_features.hpp"
#include "kernels_features_gather.hpp"
#include "device_voxelgrid.hpp"
#include "../../include/fls_features.h"
#include "../../include/fls_features_device.h"
#include <limits>
#include <memory>

namespace fls { struct DeskewScratch; }  // preprocess_host.hpp: the buffers of fls_features_project_deskew

struct fls_features {
    fls_feature_params p{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    fls::FeatParamsDev pd{};
    fls::RawLayoutDev layout{};
    size_t n_raw = 0;
    int N = 0;
    bool projected = false, extracted = false;
    double project_ms = 0.0, extract_ms = 0.0;

    fls::DevBuf<unsigned char> d_raw, d_valid, d_valid_pre, d_is_corner;
    // introspection arrays (raw_index, roughness, the three flag arrays) come down only when somebody asks for them
    bool have_raw_index = false, have_intro = false;
    fls::DevBuf<unsigned> d_owner;
    fls::DevBuf<int> d_row_count, d_row_start, d_row_end, d_n, d_col, d_raw_index, d_corner_idx, d_corner_cnt, d_planar_idx, d_planar_cnt;
    fls::DevBuf<float4> d_ordered;
    fls::DevBuf<float> d_depth, d_rough;

    std::vector<fls::Pt4> ordered;  // 16-byte xyzi rows (Pt4 reused as a container: the int member holds the intensity bits)
    std::vector<float> depth, rough;
    std::vector<int> col, raw_index, row_start, row_end, corner_idx, planar_idx;
    std::vector<unsigned char> valid_pre, valid_post, is_corner;
    std::vector<fls::PtI> corner, planar, corner_f, planar_f;
    std::vector<int> h_cidx, h_ccnt, h_pidx, h_pcnt;
    std::shared_ptr<fls::DeskewScratch> deskew;  // created by the first fls_features_project_deskew

    // ---- include/fls_features_device.h: the arrays stay on the device, fls_features_get fetches what it is asked for ----
    bool resident = false;       // fls_features_keep_on_device
    uint64_t d2h_bytes = 0;      // device -> host copies on behalf of the last frame so far
    size_t stats[4] = {0, 0, 0, 0};  // FLS_FEAT_STAT_*
    // One class's clouds on the device: the gathered planes (row stride cap), the compacted indices, and the filtered cloud -- the
    // VoxelGrid's own output planes, or `up` where the device declined and the host filter's result went up again.
    struct ResidentCloud {
        fls::DevBuf<float> planes;  // x | y | z | intensity, row stride cap
        fls::DevBuf<int> idx;
        fls::DevBuf<float> up;      // x | y | z | intensity of the host-filtered cloud, row stride n_f
        fls::DeviceVoxelGrid vg;
        size_t cap = 0, n = 0, n_f = 0;
        bool filter_on_device = false;
        bool stale = false, stale_idx = false, stale_f = false;  // the host copy has not been downloaded yet
        fls::HandoffCloud cloud() const {
            fls::HandoffCloud c;
            c.x = planes.p; c.y = planes.p + cap; c.z = planes.p + 2 * cap; c.in = planes.p + 3 * cap; c.n = n;
            return c;
        }
        fls::HandoffCloud filtered() const {
            fls::HandoffCloud c;
            if (filter_on_device) { c.x = vg.ox(); c.y = vg.oy(); c.z = vg.oz(); c.in = vg.oi(); }
            else { c.x = up.p; c.y = up.p + n_f; c.z = up.p + 2 * n_f; c.in = up.p + 3 * n_f; }
            c.n = n_f;
            return c;
        }
    };
    ResidentCloud rc_corner, rc_planar;
    fls::DevBuf<int> d_tot;
    int h_tot[2] = {0, 0};
    bool stale_ordered = false, stale_depth = false, stale_col = false, stale_rows = false;
    std::vector<float> tmp;
    // hand-off (fls_scan_attach_features): ready = "everything queued on this stream so far", recorded per attach and waited for by the
    // matcher's stream; consumed[k] = a matcher's copy kernels have read this handle's buffers, waited for by the next projection
    hipEvent_t ev_ready = nullptr;
    std::vector<hipEvent_t> consumed;
    size_t n_consumed = 0;

    ~fls_features() {
        for (size_t k = 0; k < n_consumed; ++k) (void)hipEventSynchronize(consumed[k]);  // (the buffers below are still being read)
        for (auto e : consumed) if (e) (void)hipEventDestroy(e);
        if (ev_ready) (void)hipEventDestroy(ev_ready);
        for (auto e : ev) if (e) (void)hipEventDestroy(e);
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
    }

    fls_status init() {
        const float fmax = std::numeric_limits<float>::max();
        const int imax = std::numeric_limits<int>::max();
        if (p.struct_size != sizeof(fls_feature_params)) return FLS_ERR_INVALID;
        if (p.lidar_vertical_scan == imax || p.lidar_horizontal_scan == imax || p.lidar_horizontal_resolution == fmax || p.min_distance == fmax ||
            p.max_distance == fmax || p.corner_thres == fmax || p.planar_thres == fmax)
            return FLS_ERR_INVALID;  // CHECK_NE(..., NaN) of both constructors
        if (p.lidar_vertical_scan <= 0 || p.lidar_horizontal_scan <= 0 || p.lidar_horizontal_scan > fls::kFeatMaxCols ||
            (p.lidar_horizontal_scan - 11) / 6 > fls::kFeatMaxSector || !(p.lidar_horizontal_resolution > 0.f))
            return FLS_ERR_INVALID;
        pd = fls::FeatParamsDev{p.lidar_vertical_scan, p.lidar_horizontal_scan, p.lidar_horizontal_resolution, p.min_distance, p.max_distance,
                                p.corner_thres, p.planar_thres};
        FLS_HIP(hipSetDevice(device));
        FLS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        for (auto& e : ev) FLS_HIP(hipEventCreate(&e));
        FLS_HIP(hipEventCreateWithFlags(&ev_ready, hipEventDisableTiming));
        d_tot.reserve(2);
        const size_t cells = size_t(pd.rows) * size_t(pd.cols);
        d_owner.reserve(cells);
        d_row_count.reserve(size_t(pd.rows)); d_row_start.reserve(size_t(pd.rows)); d_row_end.reserve(size_t(pd.rows));
        d_n.reserve(1);
        d_ordered.reserve(cells); d_depth.reserve(cells); d_rough.reserve(cells); d_col.reserve(cells); d_raw_index.reserve(cells);
        d_valid.reserve(cells); d_valid_pre.reserve(cells); d_is_corner.reserve(cells);
        d_corner_idx.reserve(size_t(pd.rows) * 120); d_corner_cnt.reserve(size_t(pd.rows));
        d_planar_idx.reserve(size_t(pd.rows) * size_t(pd.cols + 6)); d_planar_cnt.reserve(size_t(pd.rows));
        return FLS_OK;
    }

    fls_status project(const void* raw, size_t n, const fls_point_layout& L, size_t* n_ordered) {
        if (L.stride_bytes < 16 || (L.stride_bytes & 3u) || (L.xyz_offset & 3u) || (L.intensity_offset & 3u) || (L.ring_offset & 1u) ||
            L.xyz_offset + 12 > L.stride_bytes || L.intensity_offset + 4 > L.stride_bytes || L.ring_offset + 2 > L.stride_bytes ||
            n > 0xFFFFFFF0ull)
            return FLS_ERR_INVALID;
        layout = fls::RawLayoutDev{L.stride_bytes, L.xyz_offset, L.intensity_offset, L.ring_offset};
        n_raw = n;
        begin_projection();
        const size_t cells = size_t(pd.rows) * size_t(pd.cols);
        d_raw.reserve(std::max<size_t>(n * L.stride_bytes, 16));
        FLS_HIP(hipEventRecord(ev[0], stream));
        if (n) FLS_HIP(hipMemcpyAsync(d_raw.p, raw, n * L.stride_bytes, hipMemcpyHostToDevice, stream));
        FLS_HIP(hipMemsetAsync(d_owner.p, 0xFF, cells * sizeof(unsigned), stream));
        if (n)
            hipLaunchKernelGGL(fls::feat_project_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, stream, d_raw.p, unsigned(n), layout, pd,
                               d_owner.p);
        hipLaunchKernelGGL(fls::feat_count_kernel, dim3(unsigned(pd.rows)), dim3(256), 0, stream, d_owner.p, pd, d_row_count.p);
        hipLaunchKernelGGL(fls::feat_compact_kernel, dim3(unsigned(pd.rows)), dim3(256), 0, stream, d_raw.p, layout, d_owner.p, pd, d_row_count.p,
                           d_ordered.p, d_depth.p, d_col.p, d_raw_index.p, d_valid.p, d_row_start.p, d_row_end.p, d_n.p);
        FLS_HIP(hipGetLastError());
        return finish_projection(n_ordered);
    }

    // a matcher may still be copying the previous frame's clouds out of this handle's buffers: whatever is queued next waits for that
    void wait_consumers() {
        for (size_t k = 0; k < n_consumed; ++k) FLS_HIP(hipStreamWaitEvent(stream, consumed[k], 0));
        n_consumed = 0;
    }
    hipEvent_t next_consumed_event() {
        if (n_consumed == consumed.size()) {
            hipEvent_t e = nullptr;
            FLS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            consumed.push_back(e);
        }
        return consumed[n_consumed++];
    }
    // the start of every projection: no array of the previous frame is current any more
    void begin_projection() {
        projected = extracted = false;
        have_raw_index = have_intro = false;
        stale_ordered = stale_depth = stale_col = stale_rows = false;
        d2h_bytes = 0;
        wait_consumers();
    }

    // behind the launches of a projection (all three forms): the read-back.  Default: N and the ring indices, then the ordered cloud,
    // depths and columns.  Resident: N alone.
    fls_status finish_projection(size_t* n_ordered) {
        FLS_HIP(hipEventRecord(ev[1], stream));
        FLS_HIP(hipMemcpyAsync(&N, d_n.p, sizeof(int), hipMemcpyDeviceToHost, stream));
        d2h_bytes += sizeof(int);
        const size_t rows = size_t(pd.rows);
        if (!resident) {
            row_start.resize(rows); row_end.resize(rows);
            FLS_HIP(hipMemcpyAsync(row_start.data(), d_row_start.p, rows * sizeof(int), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipMemcpyAsync(row_end.data(), d_row_end.p, rows * sizeof(int), hipMemcpyDeviceToHost, stream));
            d2h_bytes += 2 * rows * sizeof(int);
        }
        FLS_HIP(hipStreamSynchronize(stream));
        const size_t m = size_t(N);
        if (resident) {
            stale_ordered = stale_depth = stale_col = stale_rows = true;
        } else {
            ordered.resize(m); depth.resize(m); col.resize(m);
            if (m) {
                FLS_HIP(hipMemcpyAsync(ordered.data(), d_ordered.p, m * sizeof(float4), hipMemcpyDeviceToHost, stream));
                FLS_HIP(hipMemcpyAsync(depth.data(), d_depth.p, m * sizeof(float), hipMemcpyDeviceToHost, stream));
                FLS_HIP(hipMemcpyAsync(col.data(), d_col.p, m * sizeof(int), hipMemcpyDeviceToHost, stream));
                FLS_HIP(hipStreamSynchronize(stream));
                d2h_bytes += m * (sizeof(float4) + sizeof(float) + sizeof(int));
            }
        }
        float ms = 0.f;
        FLS_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        project_ms = ms;
        projected = true;
        if (n_ordered) *n_ordered = m;
        return FLS_OK;
    }

    fls_status extract(size_t* n_corner, size_t* n_planar) {
        if (!projected) return FLS_ERR_STATE;
        const size_t m = size_t(N);
        have_intro = false;
        corner_idx.clear(); planar_idx.clear(); corner.clear(); planar.clear(); corner_f.clear(); planar_f.clear();
        // no cloud of an earlier extraction is pending on the device any more, whichever mode made it (a handle switched back to the default
        // must not fetch the resident frame's clouds over the ones computed below)
        for (ResidentCloud* c : {&rc_corner, &rc_planar}) {
            c->n = c->n_f = 0;
            c->filter_on_device = false;
            c->stale = c->stale_idx = c->stale_f = false;
        }
        if (resident) return extract_resident(n_corner, n_planar);
        if (N >= 12) {
            const size_t rows = size_t(pd.rows);
            h_cidx.resize(rows * 120); h_ccnt.resize(rows); h_pidx.resize(rows * size_t(pd.cols + 6)); h_pcnt.resize(rows);
            FLS_HIP(hipEventRecord(ev[2], stream));
            hipLaunchKernelGGL(fls::feat_valid_rough_kernel, dim3(unsigned((m + 255) / 256)), dim3(256), 0, stream, d_n.p, d_depth.p, d_col.p, d_rough.p,
                               d_valid.p);
            FLS_HIP(hipMemcpyAsync(d_valid_pre.p, d_valid.p, m, hipMemcpyDeviceToDevice, stream));  // snapshot before SelectFeatures edits the flags
            hipLaunchKernelGGL(fls::feat_select_kernel, dim3(unsigned(pd.rows)), dim3(fls::kFeatSelectThreads), 0, stream, d_n.p, pd, d_row_start.p, d_row_end.p, d_rough.p,
                               d_col.p, d_valid.p, d_is_corner.p, d_corner_idx.p, d_corner_cnt.p, d_planar_idx.p, d_planar_cnt.p);
            FLS_HIP(hipGetLastError());
            FLS_HIP(hipEventRecord(ev[3], stream));
            FLS_HIP(hipMemcpyAsync(h_ccnt.data(), d_corner_cnt.p, rows * sizeof(int), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipMemcpyAsync(h_pcnt.data(), d_planar_cnt.p, rows * sizeof(int), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipMemcpyAsync(h_cidx.data(), d_corner_idx.p, h_cidx.size() * sizeof(int), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipMemcpyAsync(h_pidx.data(), d_planar_idx.p, h_pidx.size() * sizeof(int), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            d2h_bytes += (2 * rows + h_cidx.size() + h_pidx.size()) * sizeof(int);
            float ms = 0.f;
            FLS_HIP(hipEventElapsedTime(&ms, ev[2], ev[3]));
            extract_ms = ms;
            // corner_cloud_ grows ring by ring, sector by sector (:158-160); planar_cloud_ += per-ring cloud (:220)
            for (size_t r = 0; r < rows; ++r) {
                corner_idx.insert(corner_idx.end(), h_cidx.begin() + r * 120, h_cidx.begin() + r * 120 + h_ccnt[r]);
                planar_idx.insert(planar_idx.end(), h_pidx.begin() + r * size_t(pd.cols + 6), h_pidx.begin() + r * size_t(pd.cols + 6) + h_pcnt[r]);
            }
            auto gather = [&](const std::vector<int>& idx, std::vector<fls::PtI>& out) {
                out.resize(idx.size());
                for (size_t k = 0; k < idx.size(); ++k) std::memcpy(&out[k], &ordered[size_t(idx[k])], sizeof(fls::PtI));
            };
            gather(corner_idx, corner);
            gather(planar_idx, planar);
            if (p.corner_voxel_filter_size > 0.f) corner_f = fls::voxel_grid(corner, p.corner_voxel_filter_size);  // preprocessing.cpp:234-235
            if (p.planar_voxel_filter_size > 0.f) planar_f = fls::voxel_grid(planar, p.planar_voxel_filter_size);  // :236-237
        }
        extracted = true;
        if (n_corner) *n_corner = corner.size();
        if (n_planar) *n_planar = planar.size();
        return FLS_OK;
    }

    // fls_features_extract with the arrays kept on the device: the same two launches, then the gather (kernels_features_gather.hpp), ONE
    // wait for the two sizes, then the two VoxelGrid filters on the gathered planes
    fls_status extract_resident(size_t* n_corner, size_t* n_planar) {
        const size_t m = size_t(N), rows = size_t(pd.rows);
        wait_consumers();  // (an extraction repeated without a projection writes the same buffers)
        if (N >= 12) {
            rc_corner.cap = rows * size_t(fls::kFeatCornerStride);
            rc_planar.cap = rows * size_t(pd.cols + 6);
            for (ResidentCloud* c : {&rc_corner, &rc_planar}) { c->planes.reserve(4 * c->cap); c->idx.reserve(c->cap); }
            FLS_HIP(hipEventRecord(ev[2], stream));
            hipLaunchKernelGGL(fls::feat_valid_rough_kernel, dim3(unsigned((m + 255) / 256)), dim3(256), 0, stream, d_n.p, d_depth.p, d_col.p, d_rough.p,
                               d_valid.p);
            FLS_HIP(hipMemcpyAsync(d_valid_pre.p, d_valid.p, m, hipMemcpyDeviceToDevice, stream));  // snapshot before SelectFeatures edits the flags
            hipLaunchKernelGGL(fls::feat_select_kernel, dim3(unsigned(pd.rows)), dim3(fls::kFeatSelectThreads), 0, stream, d_n.p, pd, d_row_start.p, d_row_end.p, d_rough.p,
                               d_col.p, d_valid.p, d_is_corner.p, d_corner_idx.p, d_corner_cnt.p, d_planar_idx.p, d_planar_cnt.p);
            const auto side = [](const fls::DevBuf<int>& idx, const fls::DevBuf<int>& cnt, int stride, ResidentCloud& c) {
                return fls::FeatGatherSide{idx.p, cnt.p, stride, c.planes.p, c.planes.p + c.cap, c.planes.p + 2 * c.cap, c.planes.p + 3 * c.cap, c.idx.p};
            };
            hipLaunchKernelGGL(fls::feat_gather_kernel, dim3(unsigned(pd.rows)), dim3(fls::kFeatGatherThreads), 0, stream, d_n.p, d_ordered.p, pd.rows,
                               side(d_corner_idx, d_corner_cnt, fls::kFeatCornerStride, rc_corner), side(d_planar_idx, d_planar_cnt, pd.cols + 6, rc_planar),
                               d_tot.p);
            FLS_HIP(hipGetLastError());
            FLS_HIP(hipEventRecord(ev[3], stream));
            FLS_HIP(hipMemcpyAsync(h_tot, d_tot.p, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            d2h_bytes += 2 * sizeof(int);
            float ms = 0.f;
            FLS_HIP(hipEventElapsedTime(&ms, ev[2], ev[3]));
            extract_ms = ms;
            ++stats[FLS_FEAT_STAT_DEVICE_GATHERS];
            rc_corner.n = std::min(size_t(std::max(h_tot[0], 0)), rc_corner.cap);
            rc_planar.n = std::min(size_t(std::max(h_tot[1], 0)), rc_planar.cap);
            for (ResidentCloud* c : {&rc_corner, &rc_planar}) c->stale = c->stale_idx = c->n != 0;
            filter_resident(rc_corner, corner, corner_f, p.corner_voxel_filter_size);  // preprocessing.cpp:234-235
            filter_resident(rc_planar, planar, planar_f, p.planar_voxel_filter_size);  // :236-237
        }
        extracted = true;
        if (n_corner) *n_corner = rc_corner.n;
        if (n_planar) *n_planar = rc_planar.n;
        return FLS_OK;
    }
    // VoxelGrid of one gathered cloud: on the device; where the device declines, the exact host filter on the downloaded cloud, its
    // result uploaded again (x | y | z | intensity) so that fls_scan_attach_features still finds it in device memory
    void filter_resident(ResidentCloud& c, std::vector<fls::PtI>& full, std::vector<fls::PtI>& filtered, const float leaf) {
        if (!(leaf > 0.f) || c.n == 0) return;
        if (fls::device_voxelgrid_mode() != 0 && c.vg.run(c.planes.p, c.planes.p + c.cap, c.planes.p + 2 * c.cap, c.planes.p + 3 * c.cap, c.n, leaf, stream)) {
            c.filter_on_device = true;
            c.n_f = c.vg.n_out;
            c.stale_f = c.n_f != 0;
            ++stats[FLS_FEAT_STAT_DEVICE_FILTERS];
            return;
        }
        ++stats[FLS_FEAT_STAT_FILTER_DECLINES];
        fetch_cloud(c, full);
        filtered = fls::voxel_grid(full, leaf);
        const size_t nf = c.n_f = filtered.size();
        if (!nf) return;
        tmp.resize(4 * nf);
        for (size_t i = 0; i < nf; ++i) { tmp[i] = filtered[i].x; tmp[nf + i] = filtered[i].y; tmp[2 * nf + i] = filtered[i].z; tmp[3 * nf + i] = filtered[i].i; }
        c.up.reserve(4 * nf);
        FLS_HIP(hipMemcpyAsync(c.up.p, tmp.data(), 4 * nf * sizeof(float), hipMemcpyHostToDevice, stream));
        FLS_HIP(hipStreamSynchronize(stream));  // (`tmp` is reused)
    }

    // ---- the lazy read-back of the resident mode: the host copy of one array made current ----
    template <class T>
    bool download(bool& stale, std::vector<T>& v, const T* dev, const size_t n) {
        if (!stale) return false;
        v.resize(n);
        if (n) {
            FLS_HIP(hipMemcpyAsync(v.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
        }
        d2h_bytes += n * sizeof(T);
        stale = false;
        return true;
    }
    bool fetch_cloud(ResidentCloud& c, std::vector<fls::PtI>& out) {
        if (!c.stale) return false;
        const size_t n = c.n;
        out.resize(n);
        tmp.resize(4 * n);
        for (int a = 0; a < 4; ++a)
            FLS_HIP(hipMemcpyAsync(tmp.data() + size_t(a) * n, c.planes.p + size_t(a) * c.cap, n * sizeof(float), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        for (size_t i = 0; i < n; ++i) out[i] = fls::PtI{tmp[i], tmp[n + i], tmp[2 * n + i], tmp[3 * n + i]};
        d2h_bytes += 4 * n * sizeof(float);
        c.stale = false;
        return true;
    }
    bool fetch_filtered(ResidentCloud& c, std::vector<fls::PtI>& out) {
        if (!c.stale_f) return false;
        out = c.vg.download(stream, tmp);
        d2h_bytes += out.size() * sizeof(fls::PtI);
        c.stale_f = false;
        return true;
    }
    void fetch_resident(int what) {
        FLS_HIP(hipSetDevice(device));
        const size_t m = size_t(N), rows = size_t(pd.rows);
        bool did = false;
        switch (what) {
            case FLS_FEAT_ORDERED: did = download(stale_ordered, ordered, reinterpret_cast<const fls::Pt4*>(d_ordered.p), m); break;
            case FLS_FEAT_DEPTH: did = download(stale_depth, depth, d_depth.p, m); break;
            case FLS_FEAT_COL: did = download(stale_col, col, d_col.p, m); break;
            case FLS_FEAT_ROW_START:
            case FLS_FEAT_ROW_END: {
                bool again = stale_rows;
                did = download(stale_rows, row_start, d_row_start.p, rows);
                download(again, row_end, d_row_end.p, rows);
                break;
            }
            case FLS_FEAT_CORNER: did = fetch_cloud(rc_corner, corner); break;
            case FLS_FEAT_PLANAR: did = fetch_cloud(rc_planar, planar); break;
            case FLS_FEAT_CORNER_IDX: did = download(rc_corner.stale_idx, corner_idx, rc_corner.idx.p, rc_corner.n); break;
            case FLS_FEAT_PLANAR_IDX: did = download(rc_planar.stale_idx, planar_idx, rc_planar.idx.p, rc_planar.n); break;
            case FLS_FEAT_CORNER_FILTERED: did = fetch_filtered(rc_corner, corner_f); break;
            case FLS_FEAT_PLANAR_FILTERED: did = fetch_filtered(rc_planar, planar_f); break;
            default: break;
        }
        if (did) ++stats[FLS_FEAT_STAT_LAZY_DOWNLOADS];
    }
    // the element count of an array whose host copy is not current (a size query downloads nothing); false: the host copy is current
    bool pending_size(int what, size_t& n) const {
        switch (what) {
            case FLS_FEAT_ORDERED: n = size_t(N); return stale_ordered;
            case FLS_FEAT_DEPTH: n = size_t(N); return stale_depth;
            case FLS_FEAT_COL: n = size_t(N); return stale_col;
            case FLS_FEAT_ROW_START:
            case FLS_FEAT_ROW_END: n = size_t(pd.rows); return stale_rows;
            case FLS_FEAT_CORNER: n = rc_corner.n; return rc_corner.stale;
            case FLS_FEAT_PLANAR: n = rc_planar.n; return rc_planar.stale;
            case FLS_FEAT_CORNER_IDX: n = rc_corner.n; return rc_corner.stale_idx;
            case FLS_FEAT_PLANAR_IDX: n = rc_planar.n; return rc_planar.stale_idx;
            case FLS_FEAT_CORNER_FILTERED: n = rc_corner.n_f; return rc_corner.stale_f;
            case FLS_FEAT_PLANAR_FILTERED: n = rc_planar.n_f; return rc_planar.stale_f;
            default: return false;
        }
    }

    void fetch_raw_index() {
        if (have_raw_index) return;
        const size_t m = size_t(N);
        raw_index.resize(m);
        if (m && projected) {
            FLS_HIP(hipSetDevice(device));
            FLS_HIP(hipMemcpyAsync(raw_index.data(), d_raw_index.p, m * sizeof(int), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            d2h_bytes += m * sizeof(int);
        }
        have_raw_index = true;
    }
    void fetch_intro() {
        if (have_intro) return;
        const size_t m = size_t(N);
        rough.assign(m, 0.f); valid_pre.assign(m, 1); valid_post.assign(m, 1); is_corner.assign(m, 0);
        if (m && extracted && N >= 12) {
            FLS_HIP(hipSetDevice(device));
            FLS_HIP(hipMemcpyAsync(rough.data(), d_rough.p, m * sizeof(float), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipMemcpyAsync(valid_pre.data(), d_valid_pre.p, m, hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipMemcpyAsync(valid_post.data(), d_valid.p, m, hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipMemcpyAsync(is_corner.data(), d_is_corner.p, m, hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            d2h_bytes += m * (sizeof(float) + 3);
        }
        have_intro = true;
    }
    template <class T>
    static size_t copy_out(const std::vector<T>& v, void* out, size_t cap) {
        if (out && !v.empty()) std::memcpy(out, v.data(), std::min(cap, v.size()) * sizeof(T));
        return v.size();
    }
    size_t get(int what, void* out, size_t cap) {
        if (what == FLS_FEAT_RAW_INDEX) fetch_raw_index();
        if (what == FLS_FEAT_IS_CORNER || what == FLS_FEAT_ROUGHNESS || what == FLS_FEAT_VALID_PRE || what == FLS_FEAT_VALID_POST) fetch_intro();
        size_t pending = 0;
        if (pending_size(what, pending)) {  // (resident mode: the array still lies on the device alone)
            if (!out) return pending;
            fetch_resident(what);
        }
        switch (what) {
            case FLS_FEAT_ORDERED: return copy_out(ordered, out, cap);
            case FLS_FEAT_DEPTH: return copy_out(depth, out, cap);
            case FLS_FEAT_COL: return copy_out(col, out, cap);
            case FLS_FEAT_ROW_START: return copy_out(row_start, out, cap);
            case FLS_FEAT_ROW_END: return copy_out(row_end, out, cap);
            case FLS_FEAT_CORNER: return copy_out(corner, out, cap);
            case FLS_FEAT_PLANAR: return copy_out(planar, out, cap);
            case FLS_FEAT_IS_CORNER: return copy_out(is_corner, out, cap);
            case FLS_FEAT_ROUGHNESS: return copy_out(rough, out, cap);
            case FLS_FEAT_VALID_PRE: return copy_out(valid_pre, out, cap);
            case FLS_FEAT_VALID_POST: return copy_out(valid_post, out, cap);
            case FLS_FEAT_CORNER_IDX: return copy_out(corner_idx, out, cap);
            case FLS_FEAT_PLANAR_IDX: return copy_out(planar_idx, out, cap);
            case FLS_FEAT_RAW_INDEX: return copy_out(raw_index, out, cap);
            case FLS_FEAT_CORNER_FILTERED: return copy_out(corner_f, out, cap);
            case FLS_FEAT_PLANAR_FILTERED: return copy_out(planar_f, out, cap);
            default: return 0;
        }
    }
};
