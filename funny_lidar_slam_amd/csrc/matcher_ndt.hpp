// matcher_ndt.hpp -- host side of FLS_INCREMENTAL_NDT, the replacement of IncrementalNDT
// (include/registration/incremental_ndt.h:16-383).
//   AddCloudToLocalMap :182-227  voxel insert with LRU eviction + UpdateVoxel (:130-179): on the device (kernels_ndt_update.hpp) -- a whole
//                                cloud through add_cloud_build (first-scan rule), later scans as incremental batches -- and on the host
//                                for whatever the device declines: there the estimated voxels are flattened into a device hash table
//                                {key -> slot} with mu[slot], info[slot] in FP64.
//   Match              :229-337  device-resident loop: ndt_lanes_kernel (7-voxel Mahalanobis scoring,
//                                FP64, the Gauss-Newton tail in its last workgroup; mode 1).
//   the map as it travels        one flat image (include/fls_map_ndt.h): map_export / map_import, map_image_*, replicate_from -- packed from the device
//                                rows or from the mirror (ndt_image.hpp, which also holds the mirror itself: NdtMirror), the same bytes either way.
#pragma once
#include "matcher_base.hpp"
#include "host_math.hpp"
#include "device_voxelgrid.hpp"
#include "kernels_ndt_update.hpp"
#include "kernels_ndt_image.hpp"
#include "kernels_knn.hpp"
#include "fitness_host.hpp"
#include <chrono>
#include <list>

namespace fls {

struct NdtMatcher final : fls_matcher, NdtMirror {
    // the host mirror of the map (Voxel, pool, LRU list, key map): ndt_image.hpp's NdtMirror
    unsigned epoch = 0;
    bool flag_first_scan = true;
    int next_vid = 0;
    double inv_voxel = 1.0;

    // device image
    std::vector<HashEntry> h_table;
    std::vector<double> h_mu, h_info;
    std::vector<int> h_vid;
    DevBuf<HashEntry> d_table;
    DevBuf<double> d_mu, d_info;
    DevBuf<int> d_vid;
    unsigned mask = 0;

    DevScan scan;
    std::vector<PtI> source;
    SourceFilter src_filter;
    bool host_timing = false;  // FLS_HOST_TIMING=1: print the host-side split of every map update
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
        host_timing = host_timing_enabled();
        init_tickets(d_ticket);
        if (const char* e = std::getenv("FLS_NDT_DEVICE_UPDATE")) allow_device_update = std::atoi(e) != 0;
        if (const char* e = std::getenv("FLS_NDT_DEVICE_SLACK")) { const long c = std::atol(e); if (c >= 0) device_slack = size_t(c); }
        if (const char* e = std::getenv("FLS_NDT_DEVICE_BUILD")) allow_device_build = std::atoi(e) != 0;
        if (!allow_device_update) allow_device_build = false;  // a handle told to stay on the host stays there
        inv_voxel = 1.0 / p.ndt_voxel_size;
        return FLS_OK;
    }

    static void mean_cov(const std::vector<double>& pts, double* mean, double* cov) {  // ComputeMeanAndCov :91-110
        const double* P = pts.data();
        hm::ndt_mean_cov(int(pts.size() / 3), [P](int k, double* q) { q[0] = P[3 * k]; q[1] = P[3 * k + 1]; q[2] = P[3 * k + 2]; }, mean, cov);
    }
    void update_voxel(Voxel& v) const {  // UpdateVoxel :130-179
        if (flag_first_scan) {
            if (v.pts.size() / 3 > 1u) { mean_cov(v.pts, v.mu, v.sigma); hm::ndt_regularised_info(v.sigma, v.info); }
            else {
                v.mu[0] = v.pts[0]; v.mu[1] = v.pts[1]; v.mu[2] = v.pts[2];
                for (int k = 0; k < 9; ++k) v.info[k] = ((k % 4 == 0) ? 1.0 : 0.0) * 1.0e2;
            }
            v.estimated = true;
            v.dirty = true;
            v.pts.clear();
            return;
        }
        if (v.estimated && v.num_points > p.ndt_max_points_in_voxel) return;
        const int npts = int(v.pts.size() / 3);
        if (!v.estimated && npts > p.ndt_min_points_in_voxel) {
            mean_cov(v.pts, v.mu, v.sigma);
            hm::ndt_regularised_info(v.sigma, v.info);
            v.estimated = true;
            v.dirty = true;
            v.pts.clear();
        } else if (v.estimated && npts > p.ndt_min_points_in_voxel) {
            double cmu[3], cvar[9];
            mean_cov(v.pts, cmu, cvar);
            hm::ndt_merge(v.mu, v.sigma, v.info, v.num_points, cmu, cvar, npts);
            v.num_points += npts;
            v.dirty = true;
            v.pts.clear();
        }
    }

    // ---- device image: table {key -> row}, rows {mu, info, vid}.  Rows are stable per voxel (free list), evicted keys leave a
    // tombstone in the table (never equal to a packed key, never "empty": probing walks over it); one map update ships only
    // the rows and table entries it changed -- a full rebuild when the table must grow, when tombstones pile up, or when
    // most of the image changed anyway (first scan).
    static constexpr unsigned long long kTombKey = ~0ull - 1ull;
    std::vector<int> free_rows;
    unsigned n_rows = 0, n_in_table = 0, n_tomb = 0;
    size_t row_cap = 0;
    std::vector<unsigned> changed_idx;
    std::vector<NdtTableEdit> edit_table;
    std::vector<NdtRowEdit> edit_rows;
    std::vector<unsigned long long> evicted_image_keys;
    PinnedBuf<unsigned char> edit_stage;
    DevBuf<unsigned char> d_edit;
    unsigned long long full_rebuilds = 0, incremental_updates = 0;

    void rebuild_image() {
        size_t n_est = 0;
        for (int v = lru_head; v >= 0; v = pool[v].next) n_est += pool[v].estimated ? 1 : 0;
        const unsigned ts = GridImage::table_size_for(n_est + n_est / 4 + 1024);  // room for the voxels the next scans estimate
        mask = ts - 1;
        h_table.assign(ts, HashEntry{kEmptyKey, 0u, 0u});
        h_mu.clear(); h_info.clear(); h_vid.clear();
        free_rows.clear();
        unsigned slot = 0;
        for (int vi = lru_head; vi >= 0; vi = pool[vi].next) {
            Voxel& v = pool[vi];
            v.dirty = false;
            v.slot = -1;
            if (!v.estimated) continue;
            const unsigned long long key = pack_key(v.kx, v.ky, v.kz);
            unsigned h = hash_key(key) & mask;
            while (h_table[h].key != kEmptyKey) h = (h + 1) & mask;
            h_table[h] = HashEntry{key, slot, 1u};
            h_mu.insert(h_mu.end(), v.mu, v.mu + 3);
            h_info.insert(h_info.end(), v.info, v.info + 9);
            h_vid.push_back(v.vid);
            v.slot = int(slot);
            ++slot;
        }
        n_rows = slot;
        n_in_table = slot;
        n_tomb = 0;
        row_cap = size_t(slot) + slot / 4 + 1024;
        d_table.reserve(ts);
        d_mu.reserve(3 * row_cap);
        d_info.reserve(9 * row_cap);
        d_vid.reserve(row_cap);
        FLS_HIP(hipMemcpyAsync(d_table.p, h_table.data(), ts * sizeof(HashEntry), hipMemcpyHostToDevice, stream));
        if (slot) {
            FLS_HIP(hipMemcpyAsync(d_mu.p, h_mu.data(), h_mu.size() * sizeof(double), hipMemcpyHostToDevice, stream));
            FLS_HIP(hipMemcpyAsync(d_info.p, h_info.data(), h_info.size() * sizeof(double), hipMemcpyHostToDevice, stream));
            FLS_HIP(hipMemcpyAsync(d_vid.p, h_vid.data(), h_vid.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        }
        FLS_HIP(hipStreamSynchronize(stream));
        edit_table.clear(); edit_rows.clear(); evicted_image_keys.clear();
        have_map = true;
        ++full_rebuilds;
    }

    // ships what this call changed; `touched` = pool indices whose UpdateVoxel ran
    void sync_image(const std::vector<int>& touched) {
        if (!have_map) { rebuild_image(); return; }
        edit_table.clear();
        edit_rows.clear();
        changed_idx.clear();
        size_t n_new = 0;
        for (int vi : touched) n_new += (pool[vi].dirty && pool[vi].slot < 0) ? 1 : 0;
        const size_t ts = size_t(mask) + 1;
        if ((size_t(n_in_table) + n_tomb + n_new) * 2 + 2 > ts || size_t(n_rows) + n_new > row_cap || touched.size() * 4 > size_t(n_in_table) + 4096) {
            rebuild_image();
            return;
        }
        for (const unsigned long long key : evicted_image_keys) {  // evictions first: their rows are reused below
            unsigned h = hash_key(key) & mask;
            while (h_table[h].key != key) h = (h + 1) & mask;
            free_rows.push_back(int(h_table[h].begin));
            h_table[h] = HashEntry{kTombKey, 0u, 0u};
            changed_idx.push_back(h);
            --n_in_table;
            ++n_tomb;
        }
        evicted_image_keys.clear();
        for (int vi : touched) {
            Voxel& v = pool[vi];
            if (!v.dirty) continue;
            v.dirty = false;
            if (v.slot < 0) {
                if (!free_rows.empty()) { v.slot = free_rows.back(); free_rows.pop_back(); }
                else v.slot = int(n_rows++);
                const unsigned long long key = pack_key(v.kx, v.ky, v.kz);
                unsigned h = hash_key(key) & mask;
                while (h_table[h].key != kEmptyKey && h_table[h].key != kTombKey) h = (h + 1) & mask;
                if (h_table[h].key == kTombKey) --n_tomb;
                h_table[h] = HashEntry{key, unsigned(v.slot), 1u};
                changed_idx.push_back(h);
                ++n_in_table;
            }
            NdtRowEdit r;
            r.row = unsigned(v.slot);
            r.vid = v.vid;
            std::memcpy(r.mu, v.mu, sizeof(r.mu));
            std::memcpy(r.info, v.info, sizeof(r.info));
            edit_rows.push_back(r);
        }
        ++incremental_updates;
        // one edit per table index, carrying its FINAL entry (a tombstone written and re-used within this call is one edit)
        std::sort(changed_idx.begin(), changed_idx.end());
        changed_idx.erase(std::unique(changed_idx.begin(), changed_idx.end()), changed_idx.end());
        for (const unsigned h : changed_idx) edit_table.push_back(NdtTableEdit{h, 0u, h_table[h]});
        changed_idx.clear();
        if (edit_table.empty() && edit_rows.empty()) return;
        const size_t bt = edit_table.size() * sizeof(NdtTableEdit), br = edit_rows.size() * sizeof(NdtRowEdit);
        edit_stage.reserve(bt + br);
        d_edit.reserve(bt + br);
        if (bt) std::memcpy(edit_stage.p, edit_table.data(), bt);
        if (br) std::memcpy(edit_stage.p + bt, edit_rows.data(), br);
        FLS_HIP(hipMemcpyAsync(d_edit.p, edit_stage.p, bt + br, hipMemcpyHostToDevice, stream));
        const int nt = int(edit_table.size()), nr = int(edit_rows.size());
        hipLaunchKernelGGL(ndt_apply_edits_kernel, dim3(unsigned((std::max(nt, nr * 4) + 255) / 256)), dim3(256), 0, stream,
                           (const NdtTableEdit*)d_edit.p, nt, (const NdtRowEdit*)(d_edit.p + bt), nr, d_table.p, d_mu.p, d_info.p, d_vid.p);
        FLS_HIP(hipStreamSynchronize(stream));  // the staging buffer is reused by the next call
    }

    // ---- device map update (kernels_ndt_update.hpp): the image holds EVERY alive voxel (table count = "estimated"), the
    // per-voxel bookkeeping lives in device rows, the host mirror (pool / LRU list / key map) is stale until
    // sync_host_from_device().  Entered by the first cloud of a handle, from nothing (add_cloud_build: no mirror is uploaded), or from the
    // mirror after a host-path update (enter_device_mode); left by a refused batch or build and entered again eight host-path updates later.
    // A localization handle stays in it across its reloads.
    bool allow_device_update = true;  // FLS_NDT_DEVICE_UPDATE
    bool allow_device_build = true;   // FLS_NDT_DEVICE_BUILD (off with FLS_NDT_DEVICE_UPDATE=0 as well)
    size_t device_slack = 65536;      // FLS_NDT_DEVICE_SLACK: spare table entries / rows allocated ahead (test hook: small values force growth)
    bool device_mode = false, device_left = false;
    unsigned host_updates_since_left = 0;  // device mode is re-entered after a refusal once eight host-path updates went by (hysteresis)
    unsigned upd_seq = 0;
    size_t dev_entries = 0;           // table entries in use (alive voxels + tombstones since the last re-hash)
    unsigned long long device_evictions = 0, device_compactions = 0;
    DevBuf<unsigned long long> r_key, r_stamp;
    DevBuf<unsigned> r_hslot;
    DevBuf<unsigned long long> r_touch;
    DevBuf<unsigned> u_crank, u_evict, u_sidx, u_srow;  // eviction selection: creation indices, rows in eviction order, the re-created voxels
    unsigned long long device_recreated = 0;            // voxels evicted and re-created inside one device batch
    DevicePairSort ev_sort;
    DevBuf<int> r_np;
    DevBuf<unsigned char> r_est, r_cc;
    DevBuf<double> r_carry, d_sigma;
    DevBuf<NdtUpdState> d_upd;
    PinnedBuf<NdtUpdState> h_upd;
    DevBuf<unsigned> u_slot, u_lx, u_bt;
    DevBuf<float> u_cloud;
    PinnedBuf<float> u_stage;
    DevicePairSort u_sort;
    size_t dev_rows = 0, dev_alive = 0, dev_table = 0;
    int dev_next_vid = 0;
    unsigned long long dev_epoch = 0, device_batches = 0, refused_batches = 0;
    size_t alive() const { return device_mode ? dev_alive : n_alive; }
    NdtRows rows_dev() { return NdtRows{r_key.p, r_hslot.p, r_np.p, r_est.p, r_cc.p, r_carry.p, d_mu.p, d_sigma.p, d_info.p, d_vid.p, r_stamp.p, r_touch.p}; }
    void reserve_rows(size_t cap, bool keep) {
        r_key.reserve(cap, keep, stream); r_stamp.reserve(cap, keep, stream); r_hslot.reserve(cap, keep, stream); r_np.reserve(cap, keep, stream);
        r_touch.reserve(cap, keep, stream, /*zero_new=*/true);
        r_est.reserve(cap, keep, stream); r_cc.reserve(cap, keep, stream); r_carry.reserve(cap * kNdtCarry * 3, keep, stream);
        d_sigma.reserve(cap * 9, keep, stream); d_mu.reserve(cap * 3, keep, stream); d_info.reserve(cap * 9, keep, stream); d_vid.reserve(cap, keep, stream);
        row_cap = cap;
    }
    bool can_enter_device_mode() const {
        // after a refusal (device_left) the handle comes back once eight host-path updates went by: a scan that left the key range or
        // an eviction the device could not order exactly is an episode, not a reason to stay on the 2 ms host path for good
        // (a localization handle keeps flag_first_scan: every reload of it is a build, so it comes back only where builds run)
        const bool kind_ok = p.is_localization_mode ? allow_device_build && build_filter_ok() : !flag_first_scan;
        return allow_device_update && !staying_on_host() && !device_mode && !owner && kind_ok && device_rows_fit();
    }
    bool staying_on_host() const { return device_left && host_updates_since_left < 8; }
    bool device_rows_fit() const { return p.ndt_min_points_in_voxel <= kNdtCarry && p.ndt_min_points_in_voxel >= 0 && p.ndt_capacity > 2; }
    // the build filters on the device and needs the host filter's bits: the exact-order form of the device VoxelGrid
    static bool build_filter_ok() { return device_voxelgrid_mode() == 1; }
    // an empty image: the table seeded on the device, rows for a first cloud of n filtered points, nothing uploaded
    void enter_device_empty(const size_t n) {
        const size_t ahead = device_slack ? n / 2 + device_slack : 0;  // slack 0 (test hook): nothing ahead
        const unsigned ts = GridImage::table_size_for(n + ahead);
        mask = ts - 1;
        d_table.reserve(ts);
        hipLaunchKernelGGL(ndt_table_fill_kernel, dim3((ts + 255) / 256), dim3(256), 0, stream, d_table.p, ts);
        reserve_rows(n + ahead, false);
        FLS_HIP(hipMemsetAsync(r_touch.p, 0, r_touch.cap * sizeof(unsigned long long), stream));
        dev_rows = dev_alive = dev_entries = 0;
        dev_table = ts;
        dev_next_vid = next_vid;
        dev_epoch = 1;
        d_upd.reserve(1);
        h_upd.reserve(2);
        edit_table.clear(); edit_rows.clear(); evicted_image_keys.clear(); changed_idx.clear(); free_rows.clear();
        device_mode = true;
    }
    // a first cloud the device refused: the empty image is dropped, the (empty) mirror is what it was
    void leave_device_empty() {
        device_mode = false;
        have_map = false;
    }
    // uploads the whole host mirror as rows (LRU order: row 0 = least recently touched) + a table holding every alive voxel
    void enter_device_mode(size_t batch_hint) {
        const size_t na = n_alive;
        const size_t ahead = device_slack ? na / 2 + 2 * batch_hint + device_slack : 1;  // slack 0 (test hook): nothing ahead, every batch grows
        const unsigned ts = GridImage::table_size_for(na + ahead);
        mask = ts - 1;
        h_table.assign(ts, HashEntry{kEmptyKey, kNdtNewBit, 0u});
        std::vector<unsigned long long> k(na), st(na);
        std::vector<unsigned> hs(na);
        std::vector<int> np(na), vid(na);
        std::vector<unsigned char> est(na), cc(na);
        std::vector<double> carry(na * kNdtCarry * 3, 0.0), mu(na * 3), sg(na * 9), inf(na * 9);
        size_t r = 0;
        for (int vi = lru_tail; vi >= 0; vi = pool[vi].prev, ++r) {
            Voxel& v = pool[vi];
            const unsigned long long key = pack_key(v.kx, v.ky, v.kz);
            unsigned h = hash_key(key) & mask;
            while (h_table[h].key != kEmptyKey) h = (h + 1) & mask;
            h_table[h] = HashEntry{key, unsigned(r), v.estimated ? 1u : 0u};
            k[r] = key; hs[r] = h; st[r] = r + 1; np[r] = v.num_points; vid[r] = v.vid; est[r] = v.estimated ? 1 : 0;
            // unconsumed points: at most min_points of them matter (a saturated voxel's list is never read again)
            const size_t keep = (v.estimated && v.num_points > p.ndt_max_points_in_voxel) ? 0 : v.pts.size() / 3;
            cc[r] = (unsigned char)std::min<size_t>(keep, kNdtCarry);
            for (size_t q = 0; q < size_t(cc[r]) * 3; ++q) carry[r * kNdtCarry * 3 + q] = v.pts[q];
            std::memcpy(&mu[3 * r], v.mu, sizeof(v.mu)); std::memcpy(&sg[9 * r], v.sigma, sizeof(v.sigma)); std::memcpy(&inf[9 * r], v.info, sizeof(v.info));
            v.slot = -1;
            v.dirty = false;
        }
        reserve_rows(na + ahead, false);
        d_table.reserve(ts);
        auto up = [&](void* d, const void* h, size_t bytes) { if (bytes) FLS_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, stream)); };
        up(d_table.p, h_table.data(), ts * sizeof(HashEntry));
        up(r_key.p, k.data(), na * 8); up(r_stamp.p, st.data(), na * 8); up(r_hslot.p, hs.data(), na * 4); up(r_np.p, np.data(), na * 4);
        up(d_vid.p, vid.data(), na * 4); up(r_est.p, est.data(), na); up(r_cc.p, cc.data(), na); up(r_carry.p, carry.data(), carry.size() * 8);
        up(d_mu.p, mu.data(), mu.size() * 8); up(d_sigma.p, sg.data(), sg.size() * 8); up(d_info.p, inf.data(), inf.size() * 8);
        FLS_HIP(hipStreamSynchronize(stream));
        FLS_HIP(hipMemsetAsync(r_touch.p, 0, r_touch.cap * sizeof(unsigned long long), stream));
        dev_rows = dev_alive = dev_entries = na;
        device_left = false;
        dev_table = ts;
        dev_next_vid = next_vid;
        dev_epoch = na + 1;
        d_upd.reserve(1);
        h_upd.reserve(2);
        edit_table.clear(); edit_rows.clear(); evicted_image_keys.clear(); changed_idx.clear(); free_rows.clear();
        have_map = true;
        device_mode = true;
        ++full_rebuilds;
    }
    // the table of a device-mode image is rebuilt on the device when the next batch might fill it past one half
    unsigned long long table_growths = 0, row_growths = 0;
    void grow_table_device(size_t need_entries) {
        ++table_growths;
        const unsigned ts = GridImage::table_size_for(device_slack ? need_entries + need_entries / 2 + device_slack : need_entries);
        DevBuf<HashEntry> nt;
        nt.reserve(ts);
        hipLaunchKernelGGL(ndt_table_fill_kernel, dim3((ts + 255) / 256), dim3(256), 0, stream, nt.p, ts);
        if (dev_rows)  // (an image that is still empty has nothing to re-hash)
            hipLaunchKernelGGL(ndt_table_rehash_kernel, dim3(unsigned((dev_rows + 255) / 256)), dim3(256), 0, stream, nt.p, ts - 1, rows_dev(), unsigned(dev_rows));
        FLS_HIP(hipStreamSynchronize(stream));
        std::swap(d_table.p, nt.p);
        std::swap(d_table.cap, nt.cap);
        mask = ts - 1;
        dev_table = ts;
        dev_entries = dev_alive;  // the re-hash dropped the tombstones
    }
    // one map update on the device; false = refused (nothing changed): the caller syncs the host mirror and replays on the host
    bool device_add_cloud(const std::vector<PtI>& cloud) {
        const size_t n = cloud.size();
        if (n == 0) return true;
        u_stage.reserve(3 * n);
        u_cloud.reserve(3 * n);
        for (size_t i = 0; i < n; ++i) { u_stage.p[i] = cloud[i].x; u_stage.p[n + i] = cloud[i].y; u_stage.p[2 * n + i] = cloud[i].z; }
        FLS_HIP(hipMemcpyAsync(u_cloud.p, u_stage.p, 3 * n * sizeof(float), hipMemcpyHostToDevice, stream));
        return device_add_cloud_dev(u_cloud.p, u_cloud.p + n, u_cloud.p + 2 * n, n);
    }
    // the filtered world cloud already on the device (x, y, z of n points, cloud order).  first_rule: UpdateVoxel with flag_first_scan set
    // (a build: counted in slots 150 and 107, never in 109 / 110); refused_status says why a refused call was refused.
    unsigned refused_status = 0;
    bool device_add_cloud_dev(const float* x, const float* y, const float* z, const size_t n, const bool first_rule = false) {
        if (n == 0) return true;
        refused_status = 0;
        if (n > size_t(kVgMaxBlocks) * kVgTile) return false;
        if ((dev_entries + n) * 2 + 2 > dev_table) grow_table_device(dev_alive + n);
        if (dev_rows + n > row_cap) { reserve_rows(device_slack ? dev_rows + dev_rows / 2 + 2 * n : dev_rows + n, true); ++row_growths; }
        upd_seq = upd_seq + 1u;
        if (upd_seq == 0u) {  // the touch words order batches by their sequence number: start over after 2^32 of them
            upd_seq = 1u;
            FLS_HIP(hipMemsetAsync(r_touch.p, 0, r_touch.cap * sizeof(unsigned long long), stream));
        }
        const bool may_evict = dev_alive + n >= size_t(p.ndt_capacity);  // every point a new voxel: the worst case
        NdtUpdState& hs = h_upd.p[0];
        hs = NdtUpdState{};
        hs.n_rows = unsigned(dev_rows); hs.n_alive = unsigned(dev_alive); hs.next_vid = dev_next_vid; hs.epoch = dev_epoch;
        hs.capacity = unsigned(p.ndt_capacity); hs.row_cap = unsigned(std::min<size_t>(row_cap, 0x7fffffffu));
        hs.seq = upd_seq; hs.evict_ready = may_evict ? 1u : 0u; hs.dead_hi = unsigned((dev_epoch + n + 2) >> 32) + 1u;
        FLS_HIP(hipMemcpyAsync(d_upd.p, &hs, sizeof(NdtUpdState), hipMemcpyHostToDevice, stream));
        const int ni = int(n), nb1 = (ni + 255) / 256, nb2 = (ni + kVgScanBlock - 1) / kVgScanBlock;
        u_slot.reserve(n); u_lx.reserve(n); u_bt.reserve(size_t(2 * nb2));
        const NdtRows R = rows_dev();
        hipLaunchKernelGGL(ndt_upd_locate, dim3(unsigned(nb1)), dim3(256), 0, stream, x, y, z, ni, inv_voxel, d_table.p, mask, u_slot.p, d_upd.p, r_touch.p, upd_seq);
        hipLaunchKernelGGL(ndt_upd_creators, dim3(unsigned(nb2)), dim3(kVgScanBlock), 0, stream, ni, (const HashEntry*)d_table.p, (const unsigned*)u_slot.p, u_lx.p, u_bt.p);
        hipLaunchKernelGGL(vg_scan, dim3(1), dim3(kVgScanBlock), 0, stream, (const unsigned*)u_bt.p, u_bt.p + nb2, nb2, &d_upd.p->n_new);
        hipLaunchKernelGGL(ndt_upd_predecide, dim3(1), dim3(1), 0, stream, d_upd.p);
        if (may_evict && dev_rows > 0) {
            // rows in LRU order: stable radix sort by the low, then by the high word of the 64-bit stamps (dead rows last)
            const unsigned nr = unsigned(dev_rows), nbr = (nr + 255u) / 256u;
            ev_sort.prepare(dev_rows);
            hipLaunchKernelGGL(ndt_evict_keys, dim3(nbr), dim3(256), 0, stream, R, nr, hs.dead_hi, 0, (const unsigned*)nullptr, ev_sort.k0, ev_sort.v0);
            ev_sort.run(4, stream);
            hipLaunchKernelGGL(ndt_evict_keys, dim3(nbr), dim3(256), 0, stream, R, nr, hs.dead_hi, 1, (const unsigned*)ev_sort.v0, ev_sort.k0, ev_sort.v0);
            ev_sort.run(DevicePairSort::passes_for((unsigned long long)hs.dead_hi), stream);
            // the walk over the LRU order (ndt_evict_select): skips what the batch touched in time, re-creates what it touched too late
            u_crank.reserve(n); u_evict.reserve(std::max<size_t>(dev_rows, n)); u_sidx.reserve(size_t(kNdtMaxRecreate)); u_srow.reserve(size_t(kNdtMaxRecreate));
            hipLaunchKernelGGL(ndt_upd_cranks, dim3(unsigned(nb1)), dim3(256), 0, stream, ni, (const unsigned*)u_lx.p, (const unsigned*)(u_bt.p + nb2), u_crank.p);
            hipLaunchKernelGGL(ndt_evict_select, dim3(1), dim3(kNdtEvBlock), 0, stream, R, (const unsigned*)ev_sort.v0, nr, d_upd.p, (const unsigned*)u_crank.p, u_evict.p,
                               u_sidx.p, u_srow.p);
        }
        hipLaunchKernelGGL(ndt_upd_decide, dim3(1), dim3(1), 0, stream, d_upd.p);
        if (may_evict && dev_rows > 0)
            hipLaunchKernelGGL(ndt_evict_apply, dim3(unsigned(nb1)), dim3(256), 0, stream, R, (const unsigned*)u_evict.p, d_table.p, (const NdtUpdState*)d_upd.p);
        hipLaunchKernelGGL(ndt_upd_create, dim3(unsigned(nb1)), dim3(256), 0, stream, x, y, z, ni, inv_voxel, d_table.p, (const unsigned*)u_slot.p,
                           (const unsigned*)u_lx.p, (const unsigned*)(u_bt.p + nb2), R, (const NdtUpdState*)d_upd.p, (const unsigned*)u_crank.p, (const unsigned*)u_sidx.p);
        u_sort.prepare(n);
        hipLaunchKernelGGL(ndt_upd_rowkeys, dim3(unsigned(nb1)), dim3(256), 0, stream, ni, (const HashEntry*)d_table.p, (const unsigned*)u_slot.p, u_sort.k0, u_sort.v0,
                           (const NdtUpdState*)d_upd.p);
        u_sort.run(DevicePairSort::passes_for((unsigned long long)(dev_rows + n)), stream);
        if (first_rule)
            hipLaunchKernelGGL(ndt_upd_voxel_first, dim3(unsigned((ni + 63) / 64)), dim3(64), 0, stream, (const unsigned*)u_sort.k0, (const unsigned*)u_sort.v0, ni, x, y, z,
                               R, d_table.p, d_upd.p);
        else
            hipLaunchKernelGGL(ndt_upd_voxel, dim3(unsigned((ni + 63) / 64)), dim3(64), 0, stream, (const unsigned*)u_sort.k0, (const unsigned*)u_sort.v0, ni, x, y, z, R,
                               d_table.p, d_upd.p, int(p.ndt_min_points_in_voxel), int(p.ndt_max_points_in_voxel));
        hipLaunchKernelGGL(ndt_upd_commit, dim3(1), dim3(1), 0, stream, d_upd.p, unsigned(n));
        FLS_HIP(hipMemcpyAsync(&h_upd.p[1], d_upd.p, sizeof(NdtUpdState), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        FLS_HIP(hipGetLastError());
        const NdtUpdState& o = h_upd.p[1];
        if (!o.apply) {
            refused_status = o.status;
            if (!first_rule) ++refused_batches;
            return false;
        }
        dev_entries += size_t(o.n_rows) - dev_rows - o.recreated;  // one table entry per created voxel (an evicted voxel's entry stays as a tombstone, a re-created voxel reuses its own)
        dev_rows = o.n_rows; dev_alive = o.n_alive; dev_next_vid = o.next_vid; dev_epoch = o.epoch;
        last_touched = o.touched;
        device_evictions += o.evict;
        device_recreated += o.recreated;
        if (first_rule) { ++device_builds; ++full_rebuilds; } else ++device_batches;
        // retired rows pile up at the capacity (hundreds per scan): drop them through the host mirror now and then
        if (dev_rows - dev_alive > std::max<size_t>(2 * dev_alive, 262144)) compact_device_rows(n);
        return true;
    }
    unsigned last_touched = 0;
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
        if (!device_add_cloud_dev(map_vg.ox(), map_vg.oy(), map_vg.oz(), map_vg.n_out)) {
            sync_host_from_device();
            return false;
        }
        ++resident_updates;
        if (host_timing) {
            const auto t1 = std::chrono::steady_clock::now();
            std::fprintf(stderr, "[fls_reg] ndt map update (device, resident source): %zu -> %zu pts | transform + VoxelGrid + UpdateVoxel x%u %.3f ms (%zu voxels)\n", n,
                         map_vg.n_out, last_touched, std::chrono::duration<double, std::milli>(t1 - t0).count(), dev_alive);
        }
        return true;
    }
    // device rows -> host mirror (pool, LRU list in stamp order, key map); the image is rebuilt by the next host-path update
    void sync_host_from_device() {
        const size_t nr = dev_rows;
        std::vector<unsigned long long> k(nr), st(nr);
        std::vector<int> np(nr), vid(nr);
        std::vector<unsigned char> est(nr), cc(nr);
        std::vector<double> carry(nr * kNdtCarry * 3), mu(nr * 3), sg(nr * 9), inf(nr * 9);
        auto dn = [&](void* h, const void* d, size_t bytes) { if (bytes) FLS_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, stream)); };
        dn(k.data(), r_key.p, nr * 8); dn(st.data(), r_stamp.p, nr * 8); dn(np.data(), r_np.p, nr * 4); dn(vid.data(), d_vid.p, nr * 4);
        dn(est.data(), r_est.p, nr); dn(cc.data(), r_cc.p, nr); dn(carry.data(), r_carry.p, carry.size() * 8);
        dn(mu.data(), d_mu.p, mu.size() * 8); dn(sg.data(), d_sigma.p, sg.size() * 8); dn(inf.data(), d_info.p, inf.size() * 8);
        FLS_HIP(hipStreamSynchronize(stream));
        std::vector<size_t> order(nr);
        for (size_t i = 0; i < nr; ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return st[a] < st[b]; });  // stamps are unique
        clear_mirror();
        pool.reserve(nr);
        for (const size_t r : order) {  // oldest first: every push_front leaves the most recent at the head
            if (k[r] == kNdtDeadKey) continue;  // evicted on the device
            push_row(k[r], np[r], vid[r], est[r] != 0, cc[r], &carry[r * kNdtCarry * 3], &mu[3 * r], &sg[9 * r], &inf[9 * r]);
        }
        next_vid = dev_next_vid;
        device_mode = false;
        device_left = true;
        host_updates_since_left = 0;
        have_map = false;  // the host-path image (estimated voxels only, host-assigned rows) is rebuilt from the mirror
        rebuild_image();
    }
    void compact_device_rows(size_t batch_hint) {
        sync_host_from_device();
        device_left = false;
        ++device_compactions;
        if (can_enter_device_mode()) enter_device_mode(batch_hint);
    }

    // ---- the map as one flat image (include/fls_map_ndt.h, ndt_image.hpp): fls_map_export / _import, fls_map_image_*, replica sets.  The bytes are
    // a function of the map's logical state: the mirror walked from its LRU tail and the device rows sorted by their stamps give the same image.
    // A device-mode export runs on the device and changes nothing (the stamp sort uses the eviction selection's scratch buffers); an import
    // builds new rows and a new table beside the old ones, checks them, and swaps them in only then.  Slots 156-159.
    unsigned long long image_exports_device = 0, image_exports_mirror = 0, image_imports_device = 0, image_imports_mirror = 0;
    DevBuf<unsigned char> img_stage;      // the image on the device, where the caller's buffer is not device memory the kernels can use directly
    PinnedBuf<unsigned char> img_pinned;  // the image (or its header) on its way between the mirror and device memory
    DevBuf<unsigned> img_status;
    PinnedBuf<unsigned> img_status_h;
    NdtImageParams image_params() const { return NdtImageParams{p.ndt_voxel_size, p.ndt_min_points_in_voxel, p.ndt_max_points_in_voxel, p.ndt_capacity}; }
    // a voxel may hold as many pending points as ndt_min_points_in_voxel: an image entry carries kNdtCarry of them, like a device row
    bool image_fits() const { return !owner && p.ndt_min_points_in_voxel <= kNdtCarry; }
    static bool kernel_aligned(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }
    size_t map_image_bytes() override {
        NdtImageLayout L;
        return image_fits() && ndt_image_layout(alive(), L) ? L.total : 0;
    }
    fls_status map_image_export(void* dst, size_t cap, int dst_on_device) override {
        NdtImageLayout L;
        if (!image_fits() || !dst || !ndt_image_layout(alive(), L)) return FLS_ERR_STATE;
        if (cap < L.total) return FLS_ERR_RANGE;
        unsigned char* const out = static_cast<unsigned char*>(dst);
        if (!device_mode) {  // from the mirror: lru_tail -> prev, as enter_device_mode walks it
            unsigned char* const host = dst_on_device ? (img_pinned.reserve(L.total), img_pinned.p) : out;
            ndt_image_from_mirror(*this, image_params(), next_vid, flag_first_scan, L, host);
            if (dst_on_device) {
                FLS_HIP(hipMemcpyAsync(out, host, L.total, hipMemcpyHostToDevice, stream));
                FLS_HIP(hipStreamSynchronize(stream));
            }
            ++image_exports_mirror;
            return FLS_OK;
        }
        const bool direct = dst_on_device && kernel_aligned(dst);
        unsigned char* img = out;
        if (!direct) { img_stage.reserve(L.total); img = img_stage.p; }
        img_pinned.reserve(sizeof(fls_ndt_image_header));
        const fls_ndt_image_header h = ndt_image_make_header(image_params(), L, dev_next_vid, flag_first_scan);
        std::memcpy(img_pinned.p, &h, sizeof(h));
        FLS_HIP(hipMemsetAsync(img, 0, L.total, stream));  // the padding between the arrays
        FLS_HIP(hipMemcpyAsync(img, img_pinned.p, sizeof(h), hipMemcpyHostToDevice, stream));
        if (L.n) {
            // rows in LRU order, as the eviction selection orders them: stable radix sort by the low, then by the high word of the stamps, dead rows last
            const unsigned nr = unsigned(dev_rows), nbr = (nr + 255u) / 256u;
            const unsigned dead_hi = unsigned((dev_epoch + 2) >> 32) + 1u;
            const NdtRows R = rows_dev();
            ev_sort.prepare(dev_rows);
            hipLaunchKernelGGL(ndt_evict_keys, dim3(nbr), dim3(256), 0, stream, R, nr, dead_hi, 0, (const unsigned*)nullptr, ev_sort.k0, ev_sort.v0);
            ev_sort.run(4, stream);
            hipLaunchKernelGGL(ndt_evict_keys, dim3(nbr), dim3(256), 0, stream, R, nr, dead_hi, 1, (const unsigned*)ev_sort.v0, ev_sort.k0, ev_sort.v0);
            ev_sort.run(DevicePairSort::passes_for((unsigned long long)dead_hi), stream);
            const unsigned long long lanes = (unsigned long long)L.n * kNdtImageLanesPerVoxel;
            hipLaunchKernelGGL(ndt_image_pack_kernel, dim3(unsigned((lanes + 255ull) / 256ull)), dim3(256), 0, stream, R, (const unsigned*)ev_sort.v0,
                               (unsigned long long)L.n, int(p.ndt_max_points_in_voxel), img, ndt_image_offsets(L));
        }
        if (!direct) FLS_HIP(hipMemcpyAsync(out, img, L.total, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        FLS_HIP(hipGetLastError());
        ++image_exports_device;
        return FLS_OK;
    }
    size_t map_export(void* blob, size_t cap) override {
        const size_t need = map_image_bytes();
        if (need && blob && cap >= need && map_image_export(blob, cap, 0) != FLS_OK) return 0;
        return need;
    }
    // what an import leaves of the Match before it (as a replaced iVox map does)
    void map_replaced() {
        have_final = false;
        log_n = 0;
        log_stale = false;
        have_fitness_grid = false;  // not in the image: the next AddCloudToLocalMap of a localization handle builds it
    }
    struct RowBufs {
        DevBuf<unsigned long long> key, stamp, touch;
        DevBuf<unsigned> hslot;
        DevBuf<int> np, vid;
        DevBuf<unsigned char> est, cc;
        DevBuf<double> carry, mu, sigma, info;
        DevBuf<HashEntry> table;
        void reserve(const size_t rows, const size_t ts) {
            key.reserve(rows); stamp.reserve(rows); touch.reserve(rows); hslot.reserve(rows); np.reserve(rows); vid.reserve(rows); est.reserve(rows); cc.reserve(rows);
            carry.reserve(rows * kNdtCarry * 3); mu.reserve(rows * 3); sigma.reserve(rows * 9); info.reserve(rows * 9);
            table.reserve(ts);
        }
        NdtRows rows() { return NdtRows{key.p, hslot.p, np.p, est.p, cc.p, carry.p, mu.p, sigma.p, info.p, vid.p, stamp.p, touch.p}; }
    };
    // the rows and the table an import fills and checks before the handle takes them; what it takes them for stays here for the next import
    // (a replica-set refresh, a periodic re-broadcast): after the first one no import allocates
    RowBufs img_rows;
    template <class T> static void swap_buf(DevBuf<T>& a, DevBuf<T>& b) { std::swap(a.p, b.p); std::swap(a.cap, b.cap); }
    fls_status map_image_import(const void* src, size_t n_bytes, int src_on_device) override {
        if (owner || !src) return FLS_ERR_INVALID;  // a batch lane has no map of its own
        if (!image_fits()) return FLS_ERR_STATE;
        // (1) the header, on the host
        unsigned char head[sizeof(fls_ndt_image_header)];
        if (n_bytes < sizeof(head)) return FLS_ERR_INVALID;
        if (src_on_device) FLS_HIP(hipMemcpy(head, src, sizeof(head), hipMemcpyDeviceToHost));
        else std::memcpy(head, src, sizeof(head));
        fls_ndt_image_header h;
        NdtImageLayout L;
        const fls_status hrc = ndt_image_check_header(head, n_bytes, image_params(), h, L);
        if (hrc != FLS_OK) return hrc;
        FLS_HIP(hipStreamSynchronize(stream));
        const bool to_device = allow_device_update && device_rows_fit() && !staying_on_host();
        const size_t n = L.n;
        RowBufs& nb = img_rows;
        unsigned ts = 0;
        size_t cap_rows = 0;
        const unsigned char* host_bytes = src_on_device ? nullptr : static_cast<const unsigned char*>(src);
        if (n) {
            // (2) the voxels, on the device: into rows and a table of their own
            const unsigned char* img = static_cast<const unsigned char*>(src);
            if (!(src_on_device && kernel_aligned(src))) {
                img_stage.reserve(L.total);
                FLS_HIP(hipMemcpyAsync(img_stage.p, src, L.total, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
                img = img_stage.p;
            }
            const size_t ahead = to_device ? (device_slack ? n / 2 + device_slack : 1) : 0;  // as enter_device_mode sizes them (no batch in sight)
            ts = GridImage::table_size_for(n + ahead);
            cap_rows = n + ahead;
            nb.reserve(cap_rows, ts);
            img_status.reserve(1);
            img_status_h.reserve(1);
            FLS_HIP(hipMemsetAsync(img_status.p, 0, sizeof(unsigned), stream));
            FLS_HIP(hipMemsetAsync(nb.touch.p, 0, nb.touch.cap * sizeof(unsigned long long), stream));
            const NdtRows R = nb.rows();
            const unsigned long long lanes = (unsigned long long)n * kNdtImageLanesPerVoxel;
            hipLaunchKernelGGL(ndt_table_fill_kernel, dim3((ts + 255) / 256), dim3(256), 0, stream, nb.table.p, ts);
            hipLaunchKernelGGL(ndt_image_check_unpack_kernel, dim3(unsigned((lanes + 255ull) / 256ull)), dim3(256), 0, stream, img, ndt_image_offsets(L),
                               (unsigned long long)n, int(p.ndt_max_points_in_voxel), int(h.next_vid), R, img_status.p);
            hipLaunchKernelGGL(ndt_table_rehash_check_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, stream, nb.table.p, ts - 1, R, unsigned(n), img_status.p);
            FLS_HIP(hipMemcpyAsync(img_status_h.p, img_status.p, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
            if (!to_device && src_on_device) {  // the mirror is built from host memory
                img_pinned.reserve(L.total);
                FLS_HIP(hipMemcpyAsync(img_pinned.p, img, L.total, hipMemcpyDeviceToHost, stream));
                host_bytes = img_pinned.p;
            }
            FLS_HIP(hipStreamSynchronize(stream));
            FLS_HIP(hipGetLastError());
            if (img_status_h.p[0] != 0u) return FLS_ERR_INVALID;  // (the handle is as it was)
        }
        // (3) the handle takes the image
        FLS_HIP(hipDeviceSynchronize());  // launches of the batch lanes may still hold the old buffers
        clear_mirror();
        next_vid = h.next_vid;
        flag_first_scan = h.flag_first_scan != 0u;
        edit_table.clear(); edit_rows.clear(); evicted_image_keys.clear(); changed_idx.clear(); free_rows.clear();
        map_replaced();
        if (n == 0) {  // an empty handle: what it was before its first cloud
            device_mode = false;
            have_map = false;
            ++(to_device ? image_imports_device : image_imports_mirror);
            return FLS_OK;
        }
        if (to_device) {
            swap_buf(r_key, nb.key); swap_buf(r_stamp, nb.stamp); swap_buf(r_touch, nb.touch); swap_buf(r_hslot, nb.hslot); swap_buf(r_np, nb.np);
            swap_buf(d_vid, nb.vid); swap_buf(r_est, nb.est); swap_buf(r_cc, nb.cc); swap_buf(r_carry, nb.carry); swap_buf(d_mu, nb.mu);
            swap_buf(d_sigma, nb.sigma); swap_buf(d_info, nb.info); swap_buf(d_table, nb.table);
            row_cap = cap_rows;
            mask = ts - 1;
            dev_table = ts;
            dev_rows = dev_alive = dev_entries = n;
            dev_next_vid = h.next_vid;
            dev_epoch = n + 1;
            device_left = false;
            d_upd.reserve(1);
            h_upd.reserve(2);
            have_map = true;
            device_mode = true;
            ++image_imports_device;
            return FLS_OK;
        }
        ndt_mirror_from_image(*this, host_bytes, L);
        device_mode = false;
        have_map = false;
        rebuild_image();  // the host-path image: estimated voxels only, rows in the mirror's order
        ++image_imports_mirror;
        return FLS_OK;
    }
    fls_status map_import(const void* blob, size_t n) override { return map_image_import(blob, n, 0); }
    // replica sets: the owner's image, exported on its device, copied device to device and imported on this handle's device.  The replica is an
    // ordinary handle holding the owner's map.
    bool can_replicate() const override { return image_fits(); }
    fls_status replicate_from(fls_matcher& o) override {
        if (o.kind != kind || owner) return FLS_ERR_STATE;
        NdtMatcher& src = static_cast<NdtMatcher&>(o);
        FLS_HIP(hipSetDevice(src.device));
        const fls_status prc = src.prepare_batch();  // image current, stream idle
        if (prc != FLS_OK) return prc;
        const size_t nbytes = src.map_image_bytes();
        if (!nbytes) return FLS_ERR_STATE;
        DevBuf<unsigned char>& out = src.replica_out;  // (kept by the owner: a refresh allocates nothing)
        out.reserve(nbytes);
        const fls_status erc = src.map_image_export(out.p, nbytes, 1);
        if (erc != FLS_OK) return erc;
        FLS_HIP(hipSetDevice(device));
        if (src.device == device) return map_image_import(out.p, nbytes, 1);
        replica_in.reserve(nbytes);
        FLS_HIP(hipMemcpyPeer(replica_in.p, device, out.p, src.device, nbytes));
        return map_image_import(replica_in.p, nbytes, 1);
    }
    DevBuf<unsigned char> replica_out, replica_in;  // the image of a replication on the owner's device / on the replica's

    // ---- the map built from a whole cloud on the device: the first cloud of a handle (flag_first_scan still set, nothing in the map) and
    // every reload of a localization handle, which keeps the flag (:222-223).  The raw cloud goes up once, the device VoxelGrid filters it
    // (bit-identical to the host filter), the update chain runs on the filter's output with the first-scan rule (ndt_upd_voxel_first) and,
    // in localization mode, the fitness grid is built from the same device cloud -- after the batch has been applied.  A decline leaves the
    // handle as it was and the host path runs the call (it also answers FLS_ERR_RANGE).  Slots 150-155.
    unsigned long long device_builds = 0, builds_declined = 0;
    enum { kWhyPoints = 0, kWhyEvictions, kWhyRange, kWhyParams, kWhyCount };
    unsigned long long declined_why[kWhyCount] = {0, 0, 0, 0};
    int left_why = kWhyEvictions;  // why the handle left device mode: what the declines of the eight host-path calls behind it count as
    DevScan build_raw;
    DeviceGridBuilder fitness_builder;
    std::vector<float> build_tmp;
    bool is_build_call() const { return !owner && (p.is_localization_mode || (flag_first_scan && !device_mode && n_alive == 0)); }
    bool decline_build(const int why) {
        ++builds_declined;
        if (why >= 0) ++declined_why[why];
        if (why >= 0 && device_mode) left_why = why;  // (the host path is about to take the image back to the mirror)
        return false;
    }
    // true: applied (FLS_OK); false: declined, nothing changed
    bool add_cloud_build(const float* c0, const size_t n0, const int stride) {
        if (n0 == 0 || c0 == nullptr) return false;  // (counted nowhere)
        if (!build_admits(n0)) return false;
        const auto t0 = std::chrono::steady_clock::now();
        build_raw.upload_raw(c0, n0, stride, stream, true);
        return build_core(build_raw.x.p, build_raw.y.p, build_raw.z.p, build_raw.xyz.p + 3 * n0, n0, [&] { return cloud_from(c0, n0, stride); }, t0);
    }
    // what add_cloud_build can say before the cloud is touched (a decline is counted)
    bool build_admits(const size_t n0) {
        if (!allow_device_build) return decline_build(-1);
        if (!device_rows_fit() || !build_filter_ok()) return decline_build(kWhyParams);
        if (n0 > size_t(kVgMaxBlocks) * kVgTile) return decline_build(kWhyPoints);
        if (staying_on_host()) return decline_build(left_why);
        return true;
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
            if (vs == kVgNoFinitePoint || vs == kVgNonFinitePoints) return decline_build(kWhyRange);
            if (vs != kVgLeafTooSmall) return decline_build(kWhyPoints);  // (the exact sort gave up)
            // PCL's "leaf size too small" (an extent of more than INT_MAX leaves, every point finite): the filter hands the cloud on as it came
            fx = rx; fy = ry; fz = rz;
            n = n0;
        }
        if (n == 0) return decline_build(kWhyPoints);
        const auto t1 = std::chrono::steady_clock::now();
        const bool from_nothing = !device_mode && n_alive == 0;
        if (from_nothing) enter_device_empty(n);
        else if (!device_mode) enter_device_mode(n);  // (a populated mirror: a localization handle back from the host path)
        if (!device_add_cloud_dev(fx, fy, fz, n, /*first_rule=*/true)) {
            // (a populated image goes back to the mirror in add_cloud_impl, like a refused batch)
            if (from_nothing) leave_device_empty();
            return decline_build((refused_status & kNdtOutOfRange) ? kWhyRange : kWhyEvictions);
        }
        flag_first_scan = p.is_localization_mode ? true : false;  // :222-226
        have_map = true;
        const auto t2 = std::chrono::steady_clock::now();
        if (p.is_localization_mode) {  // :188-190 kd-tree for GetFitnessScore, from the filtered cloud already on the device
            if (fitness_builder.run(fitness_grid, fx, fy, fz, n, 1.0f, 1, false, stream)) have_fitness_grid = true;
            else have_fitness_grid = fitness_grid.build(fx == rx ? host_cloud() : map_vg.download(stream, build_tmp), 1.0f, stream) == FLS_OK;
            FLS_HIP(hipStreamSynchronize(stream));
        }
        if (host_timing) {
            const auto t3 = std::chrono::steady_clock::now();
            auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            std::fprintf(stderr, "[fls_reg] ndt map build (device): %zu -> %zu pts | upload + VoxelGrid %.3f ms | first-scan UpdateVoxel x%u %.3f ms | fitness grid %.3f ms (%zu voxels)\n",
                         n0, n, ms(t0, t1), last_touched, ms(t1, t2), ms(t2, t3), dev_alive);
        }
        return true;
    }

    fls_status add_cloud_impl(const std::vector<PtI>& cloud_world_full) {  // :182-227
        const auto t0 = std::chrono::steady_clock::now();
        const std::vector<PtI> cloud_world = voxel_grid(cloud_world_full, p.source_cloud_filter_size);
        const auto t1 = std::chrono::steady_clock::now();
        // range check first (all-or-nothing)
        for (const PtI& pt : cloud_world) {
            const double f[3] = {double(pt.x) * inv_voxel, double(pt.y) * inv_voxel, double(pt.z) * inv_voxel};
            for (int a = 0; a < 3; ++a)
                if (!(std::fabs(f[a]) < double(kKeyLimit))) return FLS_ERR_RANGE;
        }
        if (p.is_localization_mode) { have_fitness_grid = fitness_grid.build(cloud_world, 1.0f, stream) == FLS_OK; }
        if (device_mode) {
            if (!flag_first_scan && device_add_cloud(cloud_world)) {
                if (host_timing) {
                    const auto t4 = std::chrono::steady_clock::now();
                    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
                    std::fprintf(stderr, "[fls_reg] ndt map update (device): %zu -> %zu pts | VoxelGrid %.3f ms | upload + device UpdateVoxel x%u %.3f ms (%zu voxels)\n",
                                 cloud_world_full.size(), cloud_world.size(), ms(t0, t1), last_touched, ms(t1, t4), dev_alive);
                }
                return FLS_OK;
            }
            sync_host_from_device();  // refused (evictions that would reach voxels of the batch itself): exact sequential replay below
        }
        ++epoch;
        std::vector<int> touched;
        touched.reserve(4096);
        for (const PtI& pt : cloud_world) {
            const double pe[3] = {double(pt.x), double(pt.y), double(pt.z)};
            const int kx = int(pe[0] * inv_voxel), ky = int(pe[1] * inv_voxel), kz = int(pe[2] * inv_voxel);  // cast<int>: truncation (:195)
            const unsigned long long key = pack_key(kx, ky, kz);
            int vi = grids.find(key);
            if (vi < 0) {
                if (!free_ix.empty()) { vi = free_ix.back(); free_ix.pop_back(); }
                else { vi = int(pool.size()); pool.emplace_back(); }
                Voxel& v = pool[vi];
                v.kx = kx; v.ky = ky; v.kz = kz;
                v.pts.clear();
                v.pts.push_back(pe[0]); v.pts.push_back(pe[1]); v.pts.push_back(pe[2]);
                v.estimated = false;
                v.num_points = 1;
                for (int a = 0; a < 3; ++a) v.mu[a] = 0.0;  // VoxelData's initialisers (:79-81): a recycled pool entry is a new voxel
                for (int a = 0; a < 9; ++a) v.sigma[a] = v.info[a] = 0.0;
                v.vid = next_vid++;
                v.slot = -1;
                v.dirty = false;
                v.epoch = 0;
                lru_push_front(vi);
                grids.insert(key, vi);
                ++n_alive;
                if (n_alive >= size_t(p.ndt_capacity)) {  // :202-205
                    const int b = lru_tail;
                    Voxel& e = pool[b];
                    const unsigned long long ek = pack_key(e.kx, e.ky, e.kz);
                    grids.erase(ek);
                    if (e.slot >= 0) evicted_image_keys.push_back(ek);
                    e.slot = -1;
                    e.epoch = 0;  // a voxel evicted within the call that touched it gets no UpdateVoxel (the reference would dereference a null entry)
                    lru_unlink(b);
                    free_ix.push_back(b);
                    --n_alive;
                    if (b == vi) continue;  // capacity 1: the new voxel itself
                }
            } else {
                Voxel& v = pool[vi];
                v.pts.push_back(pe[0]); v.pts.push_back(pe[1]); v.pts.push_back(pe[2]);
                if (!v.estimated) v.num_points++;
                if (lru_head != vi) { lru_unlink(vi); lru_push_front(vi); }
            }
            Voxel& v = pool[vi];
            if (v.epoch != epoch) { v.epoch = epoch; touched.push_back(vi); }
        }
        const auto t2 = std::chrono::steady_clock::now();
        size_t w = 0;
        for (size_t k = 0; k < touched.size(); ++k) {
            const int vi = touched[k];
            if (pool[vi].epoch != epoch) continue;  // evicted after its touch
            pool[vi].epoch = epoch + 0x40000000u;   // a pool entry re-created after an eviction appears twice: processed once
            update_voxel(pool[vi]);
            touched[w++] = vi;
        }
        touched.resize(w);
        for (int vi : touched) pool[vi].epoch = epoch;
        flag_first_scan = p.is_localization_mode ? true : false;  // :222-226
        const auto t3 = std::chrono::steady_clock::now();
        sync_image(touched);
        if (device_left) ++host_updates_since_left;
        if (can_enter_device_mode()) enter_device_mode(cloud_world.size());
        if (host_timing) {
            const auto t4 = std::chrono::steady_clock::now();
            auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            std::fprintf(stderr, "[fls_reg] ndt map update: %zu -> %zu pts | VoxelGrid %.3f ms | insert + LRU %.3f ms | UpdateVoxel x%zu %.3f ms | image sync %.3f ms (%zu voxels)\n",
                         cloud_world_full.size(), cloud_world.size(), ms(t0, t1), ms(t1, t2), touched.size(), ms(t2, t3), ms(t3, t4), n_alive);
        }
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
        if (is_build_call() && c.n != 0 && build_admits(c.n) && build_core(c.x, c.y, c.z, c.in, c.n, rows, std::chrono::steady_clock::now())) {
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
        const NdtMatcher& M = owner ? *owner : *this;  // a batch lane reads its owner's voxel tables
        if (M.alive() == 0 || !M.have_map) return FLS_ERR_STATE;  // CHECK(!grids_.empty()) :230
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
        const NdtGridDev ng{M.d_table.p, M.mask, M.d_mu.p, M.d_info.p, M.d_vid.p, M.inv_voxel};
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
            if (device_mode && !flag_first_scan && src_filter.resident && device_update_from_resident_source(T_in)) {
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
    const NdtMatcher* owner = nullptr;
    std::unique_ptr<fls_matcher> clone_for_lane() override { return make_owned_lane(*this); }
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
    size_t map_size(int slot) const override {
        if (slot == 105) return size_t(src_filter.device_runs);
        if (slot == 106) return size_t(src_filter.host_runs);
        if (slot == 107) return size_t(full_rebuilds);  // image: full rebuilds / incremental updates
        if (slot == 108) return size_t(incremental_updates);
        if (slot == 109) return size_t(device_batches);  // map updates applied on the device / refused (replayed on the host)
        if (slot == 110) return size_t(refused_batches);
        if (slot == 111) return size_t(resident_updates);  // map updates fed by the device-resident filtered scan
        if (slot == 112) return size_t(table_growths);     // device-side table rebuilds / row-array growths
        if (slot == 113) return size_t(row_growths);
        if (slot == 126) return size_t(device_recreated);    // ... of which re-created by a later point of the same batch
        if (slot == 117) return size_t(device_evictions);    // voxels evicted by device batches / row compactions through the host mirror
        if (slot == 118) return size_t(device_compactions);
        if (slot == 150) return size_t(device_builds);    // maps built from a whole cloud on the device / declined (host path), then why:
        if (slot == 151) return size_t(builds_declined);  // too many points, evictions the device cannot order, range or non-finite, parameters
        if (slot >= 152 && slot <= 155) return size_t(declined_why[slot - 152]);
        if (slot == 156) return size_t(image_exports_device);  // flat images (fls_map_ndt.h) exported on the device / from the mirror,
        if (slot == 157) return size_t(image_exports_mirror);  // imported into device mode / through the mirror
        if (slot == 158) return size_t(image_imports_device);
        if (slot == 159) return size_t(image_imports_mirror);
        return alive();
    }
    // fls_debug_ndt_voxels (include/fls_debug_ndt.h): every alive voxel, most recently touched first -- the mirror's LRU list, or the device
    // rows ordered by their stamps while the device holds the map.  Reads only: no counter, no state, device mode is not left.
    // pending = the unconsumed points a device row would carry (a saturated voxel's list is never read again: 0).
    struct VoxelDump { int32_t *keys, *vid, *num_points; uint8_t *estimated, *pending; double *mu, *sigma, *info; };
    size_t dump_voxels(const size_t cap, const VoxelDump& o) {
        const size_t na = alive();
        if (cap < na || na == 0) return na;
        size_t w = 0;
        auto put = [&](const int kx, const int ky, const int kz, const int vid, const int np, const bool est, const size_t pend, const double* mu, const double* sg,
                       const double* inf) {
            o.keys[3 * w] = kx; o.keys[3 * w + 1] = ky; o.keys[3 * w + 2] = kz;
            o.vid[w] = vid; o.num_points[w] = np; o.estimated[w] = est ? 1 : 0; o.pending[w] = uint8_t(pend);
            std::memcpy(o.mu + 3 * w, mu, 3 * sizeof(double)); std::memcpy(o.sigma + 9 * w, sg, 9 * sizeof(double)); std::memcpy(o.info + 9 * w, inf, 9 * sizeof(double));
            ++w;
        };
        if (!device_mode) {
            for (int vi = lru_head; vi >= 0 && w < na; vi = pool[vi].next) {
                const Voxel& v = pool[vi];
                const size_t keep = (v.estimated && v.num_points > p.ndt_max_points_in_voxel) ? 0 : v.pts.size() / 3;
                put(v.kx, v.ky, v.kz, v.vid, v.num_points, v.estimated, std::min<size_t>(keep, kNdtCarry), v.mu, v.sigma, v.info);
            }
            return w;
        }
        const size_t nr = dev_rows;
        std::vector<unsigned long long> k(nr), st(nr);
        std::vector<int> np(nr), vid(nr);
        std::vector<unsigned char> est(nr), cc(nr);
        std::vector<double> mu(nr * 3), sg(nr * 9), inf(nr * 9);
        auto dn = [&](void* h, const void* d, size_t bytes) { if (bytes) FLS_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, stream)); };
        dn(k.data(), r_key.p, nr * 8); dn(st.data(), r_stamp.p, nr * 8); dn(np.data(), r_np.p, nr * 4); dn(vid.data(), d_vid.p, nr * 4);
        dn(est.data(), r_est.p, nr); dn(cc.data(), r_cc.p, nr);
        dn(mu.data(), d_mu.p, mu.size() * 8); dn(sg.data(), d_sigma.p, sg.size() * 8); dn(inf.data(), d_info.p, inf.size() * 8);
        FLS_HIP(hipStreamSynchronize(stream));
        std::vector<size_t> order;
        order.reserve(na);
        for (size_t r = 0; r < nr; ++r) if (k[r] != kNdtDeadKey) order.push_back(r);
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return st[a] > st[b]; });  // stamps are unique
        for (const size_t r : order) {
            if (w == na) break;
            int kx, ky, kz;
            unpack_key(k[r], kx, ky, kz);
            const bool saturated = est[r] && np[r] > p.ndt_max_points_in_voxel;
            put(kx, ky, kz, vid[r], np[r], est[r] != 0, saturated ? 0 : cc[r], &mu[3 * r], &sg[9 * r], &inf[9 * r]);
        }
        return w;
    }
};

}  // namespace fls
