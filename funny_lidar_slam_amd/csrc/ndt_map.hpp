// ndt_map.hpp -- the voxel map of FLS_INCREMENTAL_NDT without a matcher around it: the replacement of IncrementalNDT's grids_ / data_
// (incremental_ndt.h:352-353) and of AddCloudToLocalMap's voxel side (:192-226).  Host mirror (NdtMirror, ndt_image.hpp) + device image
// (a table {key -> row} and rows) + the rule which of the two is the map (State): the host-path image shipped as edit lists (sync_image), the
// device rows with their update chain (kernels_ndt_update.hpp) for batches and for whole clouds (build), the moves between the two with their
// hysteresis, and the ways the map travels -- one flat image (include/fls_map_ndt.h) packed from the rows or from the mirror, the same bytes
// either way -- plus the voxel dump.  Everything is queued on the one stream given to init().  The matcher decides what goes into it.
#pragma once
#include "host_math.hpp"
#include "device_voxelgrid.hpp"
#include "kernels_ndt_update.hpp"
#include "kernels_ndt_image.hpp"
#include "kernels_knn.hpp"

namespace fls {

using NdtTime = std::chrono::steady_clock::time_point;
inline double ndt_ms(const NdtTime a, const NdtTime b) { return std::chrono::duration<double, std::milli>(b - a).count(); }  // FLS_HOST_TIMING lines

// the rows and the table of a device image.  `cap`: the rows asked for last (every row array holds at least as many)
struct NdtRowBufs {
    DevBuf<unsigned long long> key, stamp, touch;
    DevBuf<unsigned> hslot;
    DevBuf<int> np, vid;
    DevBuf<unsigned char> est, cc;
    DevBuf<double> carry, mu, sigma, info;
    DevBuf<HashEntry> table;
    size_t cap = 0;
    NdtRows rows() { return NdtRows{key.p, hslot.p, np.p, est.p, cc.p, carry.p, mu.p, sigma.p, info.p, vid.p, stamp.p, touch.p}; }
    void reserve(const size_t n, const bool keep, hipStream_t s) {
        key.reserve(n, keep, s); stamp.reserve(n, keep, s); hslot.reserve(n, keep, s); np.reserve(n, keep, s);
        touch.reserve(n, keep, s, /*zero_new=*/true);
        est.reserve(n, keep, s); cc.reserve(n, keep, s); carry.reserve(n * kNdtCarry * 3, keep, s);
        sigma.reserve(n * 9, keep, s); mu.reserve(n * 3, keep, s); info.reserve(n * 9, keep, s); vid.reserve(n, keep, s);
        cap = n;
    }
    void clear_touch(hipStream_t s) { FLS_HIP(hipMemsetAsync(touch.p, 0, touch.cap * sizeof(unsigned long long), s)); }
};
// rows on the host; copy(): the first n of them up to the device or down from it, the stream idle afterwards (hslot only on its way up:
// nothing on the host reads a row's table index)
struct NdtHostRows {
    std::vector<unsigned long long> key, stamp;
    std::vector<unsigned> hslot;
    std::vector<int> np, vid;
    std::vector<unsigned char> est, cc;
    std::vector<double> carry, mu, sigma, info;
    explicit NdtHostRows(const size_t n)
        : key(n), stamp(n), hslot(n), np(n), vid(n), est(n), cc(n), carry(n * kNdtCarry * 3, 0.0), mu(n * 3), sigma(n * 9), info(n * 9) {}
    void copy(NdtRowBufs& B, const size_t n, hipStream_t s, const bool up) {
        auto mv = [&](auto& h, auto& d, const size_t per) {
            const size_t bytes = n * per * sizeof(*d.p);
            if (bytes && up) FLS_HIP(hipMemcpyAsync(d.p, h.data(), bytes, hipMemcpyHostToDevice, s));
            if (bytes && !up) FLS_HIP(hipMemcpyAsync(h.data(), d.p, bytes, hipMemcpyDeviceToHost, s));
        };
        mv(key, B.key, 1); mv(stamp, B.stamp, 1); if (up) mv(hslot, B.hslot, 1);
        mv(np, B.np, 1); mv(vid, B.vid, 1); mv(est, B.est, 1); mv(cc, B.cc, 1); mv(carry, B.carry, kNdtCarry * 3);
        mv(mu, B.mu, 3); mv(sigma, B.sigma, 9); mv(info, B.info, 9);
        FLS_HIP(hipStreamSynchronize(s));
    }
    // the rows no eviction retired, least recently touched first
    std::vector<size_t> alive_oldest_first() const {
        std::vector<size_t> order;
        for (size_t r = 0; r < key.size(); ++r) if (key[r] != kNdtDeadKey) order.push_back(r);
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return stamp[a] < stamp[b]; });  // stamps are unique
        return order;
    }
};

struct NdtMap {
    NdtMirror mirror;  // pool, LRU list, key map, flag_first_scan, next_vid (ndt_image.hpp)
    // Who holds the map.  Transitions: rebuild_image (-> HostImage), become_device (-> Device), become_empty; nothing else assigns `state`.
    enum class State {
        Empty,      // no image on the device; the mirror is the map and is empty (a new handle, an imported empty image) -- or about to be flattened
        HostImage,  // the mirror is the map; the device holds its ESTIMATED voxels only, in rows the host assigns, kept current by sync_image
        Device,     // the device rows are the map (every alive voxel, bookkeeping included); the mirror is stale until sync_host_from_device().
                    // Inside build() also with no row yet: an empty image a first cloud is about to fill, dropped again if the device refuses
    };
    State state = State::Empty;
    bool has_image() const { return state != State::Empty; }
    bool on_device() const { return state == State::Device; }
    size_t alive() const { return on_device() ? dev_alive : mirror.n_alive; }

    hipStream_t stream = nullptr;
    NdtImageParams q{};
    bool localization = false;  // is_localization_mode: every cloud is a build and flag_first_scan stays set (:222-226)
    double inv_voxel = 1.0;
    bool host_timing = false;   // FLS_HOST_TIMING=1: print the host-side split of every map update
    bool allow_device_update = true;  // FLS_NDT_DEVICE_UPDATE
    bool allow_device_build = true;   // FLS_NDT_DEVICE_BUILD (off with FLS_NDT_DEVICE_UPDATE=0 as well)
    size_t device_slack = 65536;      // FLS_NDT_DEVICE_SLACK: spare table entries / rows allocated ahead (test hook: small values force growth)
    void init(hipStream_t s, const NdtImageParams& params, const bool localization_mode) {
        stream = s; q = params; localization = localization_mode;
        inv_voxel = 1.0 / q.voxel_size;
        host_timing = host_timing_enabled();
        if (const char* e = std::getenv("FLS_NDT_DEVICE_UPDATE")) allow_device_update = std::atoi(e) != 0;
        if (const char* e = std::getenv("FLS_NDT_DEVICE_SLACK")) { const long c = std::atol(e); if (c >= 0) device_slack = size_t(c); }
        if (const char* e = std::getenv("FLS_NDT_DEVICE_BUILD")) allow_device_build = std::atoi(e) != 0;
        if (!allow_device_update) allow_device_build = false;  // a handle told to stay on the host stays there
    }

    // the live rows and table, and the pair an import fills and checks before the map takes them (a successful import swaps the two); what the
    // map took them for stays for the next import (a replica-set refresh, a periodic re-broadcast): after the first one no import allocates
    NdtRowBufs bufs[2];
    int live_ix = 0;
    NdtRowBufs& live() { return bufs[live_ix]; }
    unsigned mask = 0;
    NdtGridDev grid() const {  // what Match reads
        const NdtRowBufs& B = bufs[live_ix];
        return NdtGridDev{B.table.p, mask, B.mu.p, B.info.p, B.vid.p, inv_voxel};
    }

    // ---- host-path image: table {key -> row}, rows {mu, info, vid}.  Rows are stable per voxel (free list), evicted keys leave a
    // tombstone in the table (never equal to a packed key, never "empty": probing walks over it); one map update ships only
    // the rows and table entries it changed -- a full rebuild when the table must grow, when tombstones pile up, or when
    // most of the image changed anyway (first scan).
    std::vector<HashEntry> h_table;
    std::vector<double> h_mu, h_info;
    std::vector<int> h_vid;
    std::vector<int> free_rows;
    unsigned n_rows = 0, n_in_table = 0, n_tomb = 0;
    std::vector<unsigned> changed_idx;
    std::vector<NdtTableEdit> edit_table;
    std::vector<NdtRowEdit> edit_rows;
    PinnedBuf<unsigned char> edit_stage;
    DevBuf<unsigned char> d_edit;
    unsigned long long full_rebuilds = 0, incremental_updates = 0;
    void clear_edits() { edit_table.clear(); edit_rows.clear(); mirror.evicted_image_keys.clear(); changed_idx.clear(); free_rows.clear(); }
    // -> Empty.  The mirror is the caller's: empty, or about to be flattened by rebuild_image
    void become_empty() { clear_edits(); state = State::Empty; }

    // -> HostImage
    void rebuild_image() {
        NdtMirror& m = mirror;
        NdtRowBufs& B = live();
        size_t n_est = 0;
        for (int v = m.lru_head; v >= 0; v = m.pool[v].next) n_est += m.pool[v].estimated ? 1 : 0;
        const unsigned ts = GridImage::table_size_for(n_est + n_est / 4 + 1024);  // room for the voxels the next scans estimate
        mask = ts - 1;
        h_table.assign(ts, HashEntry{kEmptyKey, 0u, 0u});
        h_mu.clear(); h_info.clear(); h_vid.clear();
        free_rows.clear();
        unsigned slot = 0;
        for (int vi = m.lru_head; vi >= 0; vi = m.pool[vi].next) {
            NdtMirror::Voxel& v = m.pool[vi];
            v.dirty = false; v.slot = -1;
            if (!v.estimated) continue;
            const unsigned long long key = pack_key(v.kx, v.ky, v.kz);
            unsigned h = hash_key(key) & mask;
            while (h_table[h].key != kEmptyKey) h = (h + 1) & mask;
            h_table[h] = HashEntry{key, slot, 1u};
            h_mu.insert(h_mu.end(), v.mu, v.mu + 3); h_info.insert(h_info.end(), v.info, v.info + 9); h_vid.push_back(v.vid);
            v.slot = int(slot++);
        }
        n_rows = n_in_table = slot;
        n_tomb = 0;
        B.cap = size_t(slot) + slot / 4 + 1024;
        B.table.reserve(ts); B.mu.reserve(3 * B.cap); B.info.reserve(9 * B.cap); B.vid.reserve(B.cap);
        FLS_HIP(hipMemcpyAsync(B.table.p, h_table.data(), ts * sizeof(HashEntry), hipMemcpyHostToDevice, stream));
        if (slot) {
            FLS_HIP(hipMemcpyAsync(B.mu.p, h_mu.data(), h_mu.size() * sizeof(double), hipMemcpyHostToDevice, stream));
            FLS_HIP(hipMemcpyAsync(B.info.p, h_info.data(), h_info.size() * sizeof(double), hipMemcpyHostToDevice, stream));
            FLS_HIP(hipMemcpyAsync(B.vid.p, h_vid.data(), h_vid.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        }
        FLS_HIP(hipStreamSynchronize(stream));
        edit_table.clear(); edit_rows.clear(); m.evicted_image_keys.clear();
        state = State::HostImage;
        ++full_rebuilds;
    }

    // ships what this call changed; `touched` = pool indices whose UpdateVoxel ran
    void sync_image(const std::vector<int>& touched) {
        if (state != State::HostImage) { rebuild_image(); return; }
        NdtMirror& m = mirror;
        NdtRowBufs& B = live();
        edit_table.clear(); edit_rows.clear(); changed_idx.clear();
        size_t n_new = 0;
        for (int vi : touched) n_new += (m.pool[vi].dirty && m.pool[vi].slot < 0) ? 1 : 0;
        const size_t ts = size_t(mask) + 1;
        if ((size_t(n_in_table) + n_tomb + n_new) * 2 + 2 > ts || size_t(n_rows) + n_new > B.cap || touched.size() * 4 > size_t(n_in_table) + 4096) {
            rebuild_image();
            return;
        }
        for (const unsigned long long key : m.evicted_image_keys) {  // evictions first: their rows are reused below
            unsigned h = hash_key(key) & mask;
            while (h_table[h].key != key) h = (h + 1) & mask;
            free_rows.push_back(int(h_table[h].begin));
            h_table[h] = HashEntry{kNdtTombKey, 0u, 0u};
            changed_idx.push_back(h);
            --n_in_table; ++n_tomb;
        }
        m.evicted_image_keys.clear();
        for (int vi : touched) {
            NdtMirror::Voxel& v = m.pool[vi];
            if (!v.dirty) continue;
            v.dirty = false;
            if (v.slot < 0) {
                if (!free_rows.empty()) { v.slot = free_rows.back(); free_rows.pop_back(); }
                else v.slot = int(n_rows++);
                const unsigned long long key = pack_key(v.kx, v.ky, v.kz);
                unsigned h = hash_key(key) & mask;
                while (h_table[h].key != kEmptyKey && h_table[h].key != kNdtTombKey) h = (h + 1) & mask;
                if (h_table[h].key == kNdtTombKey) --n_tomb;
                h_table[h] = HashEntry{key, unsigned(v.slot), 1u};
                changed_idx.push_back(h);
                ++n_in_table;
            }
            NdtRowEdit r;
            r.row = unsigned(v.slot); r.vid = v.vid;
            std::memcpy(r.mu, v.mu, sizeof(r.mu)); std::memcpy(r.info, v.info, sizeof(r.info));
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
        edit_stage.reserve(bt + br); d_edit.reserve(bt + br);
        if (bt) std::memcpy(edit_stage.p, edit_table.data(), bt);
        if (br) std::memcpy(edit_stage.p + bt, edit_rows.data(), br);
        FLS_HIP(hipMemcpyAsync(d_edit.p, edit_stage.p, bt + br, hipMemcpyHostToDevice, stream));
        const int nt = int(edit_table.size()), nr = int(edit_rows.size());
        hipLaunchKernelGGL(ndt_apply_edits_kernel, dim3(unsigned((std::max(nt, nr * 4) + 255) / 256)), dim3(256), 0, stream,
                           (const NdtTableEdit*)d_edit.p, nt, (const NdtRowEdit*)(d_edit.p + bt), nr, B.table.p, B.mu.p, B.info.p, B.vid.p);
        FLS_HIP(hipStreamSynchronize(stream));  // the staging buffer is reused by the next call
    }

    // ---- device map update (kernels_ndt_update.hpp): the image holds EVERY alive voxel (table count = "estimated"), the
    // per-voxel bookkeeping lives in device rows, the host mirror (pool / LRU list / key map) is stale until
    // sync_host_from_device().  Entered by the first cloud of a handle, from nothing (build: no mirror is uploaded), or from the
    // mirror after a host-path update (enter_device_mode); left by a refused batch or build and entered again eight host-path updates later.
    // A localization handle stays in it across its reloads.
    // The hysteresis: after a refusal (device_left) the handle comes back once eight host-path updates went by -- a scan that left the key
    // range or an eviction the device could not order exactly is an episode, not a reason to stay on the 2 ms host path for good.
    // sync_host_from_device sets device_left, a compaction clears it again, a dropped empty image (leave_device_empty) never sets it.
    bool device_left = false;
    unsigned host_updates_since_left = 0;
    bool staying_on_host() const { return device_left && host_updates_since_left < 8; }
    unsigned upd_seq = 0;
    size_t dev_entries = 0;  // table entries in use (alive voxels + tombstones since the last re-hash)
    unsigned long long device_evictions = 0, device_compactions = 0;
    DevBuf<unsigned> u_crank, u_evict, u_sidx, u_srow;  // eviction selection: creation indices, rows in eviction order, the re-created voxels
    unsigned long long device_recreated = 0;            // voxels evicted and re-created inside one device batch
    DevicePairSort ev_sort;
    DevBuf<NdtUpdState> d_upd;
    PinnedBuf<NdtUpdState> h_upd;
    DevBuf<unsigned> u_slot, u_lx, u_bt;
    DevBuf<float> u_cloud;
    PinnedBuf<float> u_stage;
    DevicePairSort u_sort;
    size_t dev_rows = 0, dev_alive = 0, dev_table = 0;
    int dev_next_vid = 0;
    unsigned long long dev_epoch = 0, device_batches = 0, refused_batches = 0;
    unsigned long long table_growths = 0, row_growths = 0;
    unsigned last_touched = 0;
    unsigned refused_status = 0;  // why a refused device_add_cloud_dev was refused
    bool can_enter_device_mode() const {
        // (a localization handle keeps flag_first_scan: every reload of it is a build, so it comes back only where builds run)
        const bool kind_ok = localization ? allow_device_build && build_filter_ok() : !mirror.flag_first_scan;
        return allow_device_update && !staying_on_host() && !on_device() && kind_ok && device_rows_fit();
    }
    bool device_rows_fit() const { return q.min_points <= kNdtCarry && q.min_points >= 0 && q.capacity > 2; }
    // the build filters on the device and needs the host filter's bits: the exact-order form of the device VoxelGrid
    static bool build_filter_ok() { return device_voxelgrid_mode() == 1; }
    // -> Device: n rows, all alive, in a table of ts entries
    void become_device(const size_t n, const unsigned ts) {
        dev_rows = dev_alive = dev_entries = n;
        mask = ts - 1; dev_table = ts;
        dev_next_vid = mirror.next_vid;
        dev_epoch = n + 1;
        d_upd.reserve(1); h_upd.reserve(2);
        clear_edits();
        state = State::Device;
    }
    // an empty image: the table seeded on the device, rows for a first cloud of n filtered points, nothing uploaded
    void enter_device_empty(const size_t n) {
        NdtRowBufs& B = live();
        const size_t ahead = device_slack ? n / 2 + device_slack : 0;  // slack 0 (test hook): nothing ahead
        const unsigned ts = GridImage::table_size_for(n + ahead);
        B.table.reserve(ts);
        hipLaunchKernelGGL(ndt_table_fill_kernel, dim3((ts + 255) / 256), dim3(256), 0, stream, B.table.p, ts);
        B.reserve(n + ahead, false, stream);
        B.clear_touch(stream);
        become_device(0, ts);
    }
    // a first cloud the device refused: the empty image is dropped, the (empty) mirror is what it was
    void leave_device_empty() { become_empty(); }
    // uploads the whole host mirror as rows (LRU order: row 0 = least recently touched) + a table holding every alive voxel
    void enter_device_mode(const size_t batch_hint) {
        NdtMirror& m = mirror;
        NdtRowBufs& B = live();
        const size_t na = m.n_alive;
        const size_t ahead = device_slack ? na / 2 + 2 * batch_hint + device_slack : 1;  // slack 0 (test hook): nothing ahead, every batch grows
        const unsigned ts = GridImage::table_size_for(na + ahead), tm = ts - 1;
        h_table.assign(ts, HashEntry{kEmptyKey, kNdtNewBit, 0u});
        NdtHostRows H(na);
        size_t r = 0;
        for (int vi = m.lru_tail; vi >= 0; vi = m.pool[vi].prev, ++r) {
            NdtMirror::Voxel& v = m.pool[vi];
            const unsigned long long key = pack_key(v.kx, v.ky, v.kz);
            unsigned h = hash_key(key) & tm;
            while (h_table[h].key != kEmptyKey) h = (h + 1) & tm;
            h_table[h] = HashEntry{key, unsigned(r), v.estimated ? 1u : 0u};
            H.key[r] = key; H.hslot[r] = h; H.stamp[r] = r + 1; H.np[r] = v.num_points; H.vid[r] = v.vid; H.est[r] = v.estimated ? 1 : 0;
            // unconsumed points: at most min_points of them matter (a saturated voxel's list is never read again)
            H.cc[r] = (unsigned char)NdtMirror::pending_of(v, q.max_points);
            for (size_t k = 0; k < size_t(H.cc[r]) * 3; ++k) H.carry[r * kNdtCarry * 3 + k] = v.pts[k];
            std::memcpy(&H.mu[3 * r], v.mu, sizeof(v.mu)); std::memcpy(&H.sigma[9 * r], v.sigma, sizeof(v.sigma)); std::memcpy(&H.info[9 * r], v.info, sizeof(v.info));
            v.slot = -1; v.dirty = false;
        }
        B.reserve(na + ahead, false, stream);
        B.table.reserve(ts);
        FLS_HIP(hipMemcpyAsync(B.table.p, h_table.data(), ts * sizeof(HashEntry), hipMemcpyHostToDevice, stream));
        H.copy(B, na, stream, /*up=*/true);
        B.clear_touch(stream);
        device_left = false;
        become_device(na, ts);
        ++full_rebuilds;
    }
    // the table of a device-mode image is rebuilt on the device when the next batch might fill it past one half
    void grow_table_device(const size_t need_entries) {
        NdtRowBufs& B = live();
        ++table_growths;
        const unsigned ts = GridImage::table_size_for(device_slack ? need_entries + need_entries / 2 + device_slack : need_entries);
        DevBuf<HashEntry> nt;
        nt.reserve(ts);
        hipLaunchKernelGGL(ndt_table_fill_kernel, dim3((ts + 255) / 256), dim3(256), 0, stream, nt.p, ts);
        if (dev_rows)  // (an image that is still empty has nothing to re-hash)
            hipLaunchKernelGGL(ndt_table_rehash_kernel, dim3(unsigned((dev_rows + 255) / 256)), dim3(256), 0, stream, nt.p, ts - 1, B.rows(), unsigned(dev_rows));
        FLS_HIP(hipStreamSynchronize(stream));
        std::swap(B.table.p, nt.p); std::swap(B.table.cap, nt.cap);
        mask = ts - 1; dev_table = ts;
        dev_entries = dev_alive;  // the re-hash dropped the tombstones
    }
    // rows in LRU order into ev_sort.v0: stable radix sort by the low, then by the high word of the 64-bit stamps (dead rows last: dead_hi is
    // above every stamp's high word)
    void sort_rows_by_stamp(const NdtRows& R, const unsigned dead_hi) {
        const unsigned nr = unsigned(dev_rows), nbr = (nr + 255u) / 256u;
        ev_sort.prepare(dev_rows);
        hipLaunchKernelGGL(ndt_evict_keys, dim3(nbr), dim3(256), 0, stream, R, nr, dead_hi, 0, (const unsigned*)nullptr, ev_sort.k0, ev_sort.v0);
        ev_sort.run(4, stream);
        hipLaunchKernelGGL(ndt_evict_keys, dim3(nbr), dim3(256), 0, stream, R, nr, dead_hi, 1, (const unsigned*)ev_sort.v0, ev_sort.k0, ev_sort.v0);
        ev_sort.run(DevicePairSort::passes_for((unsigned long long)dead_hi), stream);
    }
    // one map update on the device; false = refused (nothing changed): the caller syncs the host mirror and replays on the host
    bool device_add_cloud(const std::vector<PtI>& cloud) {
        const size_t n = cloud.size();
        if (n == 0) return true;
        u_stage.reserve(3 * n); u_cloud.reserve(3 * n);
        for (size_t i = 0; i < n; ++i) { u_stage.p[i] = cloud[i].x; u_stage.p[n + i] = cloud[i].y; u_stage.p[2 * n + i] = cloud[i].z; }
        FLS_HIP(hipMemcpyAsync(u_cloud.p, u_stage.p, 3 * n * sizeof(float), hipMemcpyHostToDevice, stream));
        return device_add_cloud_dev(u_cloud.p, u_cloud.p + n, u_cloud.p + 2 * n, n);
    }
    // the filtered world cloud already on the device (x, y, z of n points, cloud order).  first_rule: UpdateVoxel with flag_first_scan set
    // (a build: counted in slots 150 and 107, never in 109 / 110); refused_status says why a refused call was refused.
    bool device_add_cloud_dev(const float* x, const float* y, const float* z, const size_t n, const bool first_rule = false) {
        if (n == 0) return true;
        NdtRowBufs& B = live();
        refused_status = 0;
        if (n > size_t(kVgMaxBlocks) * kVgTile) return false;
        if ((dev_entries + n) * 2 + 2 > dev_table) grow_table_device(dev_alive + n);
        if (dev_rows + n > B.cap) { B.reserve(device_slack ? dev_rows + dev_rows / 2 + 2 * n : dev_rows + n, true, stream); ++row_growths; }
        upd_seq = upd_seq + 1u;
        if (upd_seq == 0u) {  // the touch words order batches by their sequence number: start over after 2^32 of them
            upd_seq = 1u;
            B.clear_touch(stream);
        }
        const bool may_evict = dev_alive + n >= size_t(q.capacity);  // every point a new voxel: the worst case
        NdtUpdState& hs = h_upd.p[0];
        hs = NdtUpdState{};
        hs.n_rows = unsigned(dev_rows); hs.n_alive = unsigned(dev_alive); hs.next_vid = dev_next_vid; hs.epoch = dev_epoch;
        hs.capacity = unsigned(q.capacity); hs.row_cap = unsigned(std::min<size_t>(B.cap, 0x7fffffffu));
        hs.seq = upd_seq; hs.evict_ready = may_evict ? 1u : 0u; hs.dead_hi = unsigned((dev_epoch + n + 2) >> 32) + 1u;
        FLS_HIP(hipMemcpyAsync(d_upd.p, &hs, sizeof(NdtUpdState), hipMemcpyHostToDevice, stream));
        const int ni = int(n), nb1 = (ni + 255) / 256, nb2 = (ni + kVgScanBlock - 1) / kVgScanBlock;
        u_slot.reserve(n); u_lx.reserve(n); u_bt.reserve(size_t(2 * nb2));
        const NdtRows R = B.rows();
        hipLaunchKernelGGL(ndt_upd_locate, dim3(unsigned(nb1)), dim3(256), 0, stream, x, y, z, ni, inv_voxel, B.table.p, mask, u_slot.p, d_upd.p, B.touch.p, upd_seq);
        hipLaunchKernelGGL(ndt_upd_creators, dim3(unsigned(nb2)), dim3(kVgScanBlock), 0, stream, ni, (const HashEntry*)B.table.p, (const unsigned*)u_slot.p, u_lx.p, u_bt.p);
        hipLaunchKernelGGL(vg_scan, dim3(1), dim3(kVgScanBlock), 0, stream, (const unsigned*)u_bt.p, u_bt.p + nb2, nb2, &d_upd.p->n_new);
        hipLaunchKernelGGL(ndt_upd_predecide, dim3(1), dim3(1), 0, stream, d_upd.p);
        if (may_evict && dev_rows > 0) {
            sort_rows_by_stamp(R, hs.dead_hi);
            // the walk over the LRU order (ndt_evict_select): skips what the batch touched in time, re-creates what it touched too late
            u_crank.reserve(n); u_evict.reserve(std::max<size_t>(dev_rows, n)); u_sidx.reserve(size_t(kNdtMaxRecreate)); u_srow.reserve(size_t(kNdtMaxRecreate));
            hipLaunchKernelGGL(ndt_upd_cranks, dim3(unsigned(nb1)), dim3(256), 0, stream, ni, (const unsigned*)u_lx.p, (const unsigned*)(u_bt.p + nb2), u_crank.p);
            hipLaunchKernelGGL(ndt_evict_select, dim3(1), dim3(kNdtEvBlock), 0, stream, R, (const unsigned*)ev_sort.v0, unsigned(dev_rows), d_upd.p, (const unsigned*)u_crank.p, u_evict.p,
                               u_sidx.p, u_srow.p);
        }
        hipLaunchKernelGGL(ndt_upd_decide, dim3(1), dim3(1), 0, stream, d_upd.p);
        if (may_evict && dev_rows > 0)
            hipLaunchKernelGGL(ndt_evict_apply, dim3(unsigned(nb1)), dim3(256), 0, stream, R, (const unsigned*)u_evict.p, B.table.p, (const NdtUpdState*)d_upd.p);
        hipLaunchKernelGGL(ndt_upd_create, dim3(unsigned(nb1)), dim3(256), 0, stream, x, y, z, ni, inv_voxel, B.table.p, (const unsigned*)u_slot.p,
                           (const unsigned*)u_lx.p, (const unsigned*)(u_bt.p + nb2), R, (const NdtUpdState*)d_upd.p, (const unsigned*)u_crank.p, (const unsigned*)u_sidx.p);
        u_sort.prepare(n);
        hipLaunchKernelGGL(ndt_upd_rowkeys, dim3(unsigned(nb1)), dim3(256), 0, stream, ni, (const HashEntry*)B.table.p, (const unsigned*)u_slot.p, u_sort.k0, u_sort.v0,
                           (const NdtUpdState*)d_upd.p);
        u_sort.run(DevicePairSort::passes_for((unsigned long long)(dev_rows + n)), stream);
        if (first_rule)
            hipLaunchKernelGGL(ndt_upd_voxel_first, dim3(unsigned((ni + 63) / 64)), dim3(64), 0, stream, (const unsigned*)u_sort.k0, (const unsigned*)u_sort.v0, ni, x, y, z,
                               R, B.table.p, d_upd.p);
        else
            hipLaunchKernelGGL(ndt_upd_voxel, dim3(unsigned((ni + 63) / 64)), dim3(64), 0, stream, (const unsigned*)u_sort.k0, (const unsigned*)u_sort.v0, ni, x, y, z, R,
                               B.table.p, d_upd.p, int(q.min_points), int(q.max_points));
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
    // device rows -> host mirror (pool, LRU list in stamp order, key map), then -> HostImage: the host-path image (estimated voxels only,
    // host-assigned rows) rebuilt from the mirror
    void sync_host_from_device() {
        NdtHostRows H(dev_rows);
        H.copy(live(), dev_rows, stream, /*up=*/false);
        mirror.clear_mirror();
        mirror.pool.reserve(dev_rows);
        for (const size_t r : H.alive_oldest_first())  // every push_front leaves the most recent at the head
            mirror.push_row(H.key[r], H.np[r], H.vid[r], H.est[r] != 0, H.cc[r], &H.carry[r * kNdtCarry * 3], &H.mu[3 * r], &H.sigma[9 * r], &H.info[9 * r]);
        mirror.next_vid = dev_next_vid;
        device_left = true; host_updates_since_left = 0;
        rebuild_image();
    }
    void compact_device_rows(const size_t batch_hint) {
        sync_host_from_device();
        device_left = false;
        ++device_compactions;
        if (can_enter_device_mode()) enter_device_mode(batch_hint);
    }

    // ---- AddCloudToLocalMap :192-226 for the filtered world cloud on the host, every key in range (in_key_range): as a device batch where
    // the device holds the map and takes it, else on the mirror.  n_raw, t0, t1: the caller's VoxelGrid, for the FLS_HOST_TIMING line
    bool in_key_range(const std::vector<PtI>& cloud_world) const {
        for (const PtI& pt : cloud_world)
            for (const float c : {pt.x, pt.y, pt.z})
                if (!(std::fabs(double(c) * inv_voxel) < double(kKeyLimit))) return false;
        return true;
    }
    void add_cloud(const std::vector<PtI>& cloud_world, const size_t n_raw, const NdtTime t0, const NdtTime t1) {
        if (on_device()) {
            if (!mirror.flag_first_scan && device_add_cloud(cloud_world)) {
                if (host_timing)
                    std::fprintf(stderr, "[fls_reg] ndt map update (device): %zu -> %zu pts | VoxelGrid %.3f ms | upload + device UpdateVoxel x%u %.3f ms (%zu voxels)\n",
                                 n_raw, cloud_world.size(), ndt_ms(t0, t1), last_touched, ndt_ms(t1, std::chrono::steady_clock::now()), dev_alive);
                return;
            }
            sync_host_from_device();  // refused (evictions that would reach voxels of the batch itself): exact sequential replay below
        }
        NdtTime t2;
        const std::vector<int> touched = mirror.insert(cloud_world, q, &t2);
        mirror.flag_first_scan = localization;  // :222-226
        const NdtTime t3 = std::chrono::steady_clock::now();
        sync_image(touched);
        if (device_left) ++host_updates_since_left;
        if (can_enter_device_mode()) enter_device_mode(cloud_world.size());
        if (host_timing)
            std::fprintf(stderr, "[fls_reg] ndt map update: %zu -> %zu pts | VoxelGrid %.3f ms | insert + LRU %.3f ms | UpdateVoxel x%zu %.3f ms | image sync %.3f ms (%zu voxels)\n",
                         n_raw, cloud_world.size(), ndt_ms(t0, t1), ndt_ms(t1, t2), touched.size(), ndt_ms(t2, t3), ndt_ms(t3, std::chrono::steady_clock::now()), mirror.n_alive);
    }

    // ---- the map built from a whole cloud on the device: the first cloud of a handle (flag_first_scan still set, nothing in the map) and every reload
    // of a localization handle, which keeps the flag (:222-223): the update chain with the first-scan rule (ndt_upd_voxel_first).  Slots 150-155.
    unsigned long long device_builds = 0, builds_declined = 0;
    enum { kWhyPoints = 0, kWhyEvictions, kWhyRange, kWhyParams, kWhyCount };
    unsigned long long declined_why[kWhyCount] = {0, 0, 0, 0};
    int left_why = kWhyEvictions;  // why the handle left device mode: what the declines of the eight host-path calls behind it count as
    bool wants_build() const { return localization || (mirror.flag_first_scan && !on_device() && mirror.n_alive == 0); }
    bool decline_build(const int why) {
        ++builds_declined;
        if (why >= 0) ++declined_why[why];
        if (why >= 0 && on_device()) left_why = why;  // (the host path is about to take the image back to the mirror)
        return false;
    }
    // what a build can say before the cloud is touched (a decline is counted)
    bool build_admits(const size_t n0) {
        if (!allow_device_build) return decline_build(-1);
        if (!device_rows_fit() || !build_filter_ok()) return decline_build(kWhyParams);
        if (n0 > size_t(kVgMaxBlocks) * kVgTile) return decline_build(kWhyPoints);
        if (staying_on_host()) return decline_build(left_why);
        return true;
    }
    // the filtered cloud on the device (n > 0 points) into the map.  true: applied; false: declined (counted), nothing changed
    bool build(const float* x, const float* y, const float* z, const size_t n) {
        const bool from_nothing = !on_device() && mirror.n_alive == 0;
        if (from_nothing) enter_device_empty(n);
        else if (!on_device()) enter_device_mode(n);  // (a populated mirror: a localization handle back from the host path)
        if (!device_add_cloud_dev(x, y, z, n, /*first_rule=*/true)) {
            // (a populated image goes back to the mirror in add_cloud, like a refused batch)
            if (from_nothing) leave_device_empty();
            return decline_build((refused_status & kNdtOutOfRange) ? kWhyRange : kWhyEvictions);
        }
        mirror.flag_first_scan = localization;  // :222-226
        return true;
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
    DevBuf<unsigned char> replica_out, replica_in;  // the image of a replication on the owner's device / on the replica's
    // a voxel may hold as many pending points as ndt_min_points_in_voxel: an image entry carries kNdtCarry of them, like a device row
    bool image_fits() const { return q.min_points <= kNdtCarry; }
    static bool kernel_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
    size_t image_bytes() const { NdtImageLayout L; return image_fits() && ndt_image_layout(alive(), L) ? L.total : 0; }
    fls_status image_export(void* dst, size_t cap, int dst_on_device) {
        NdtImageLayout L;
        if (!image_fits() || !dst || !ndt_image_layout(alive(), L)) return FLS_ERR_STATE;
        if (cap < L.total) return FLS_ERR_RANGE;
        unsigned char* const out = static_cast<unsigned char*>(dst);
        if (!on_device()) {  // from the mirror: lru_tail -> prev, as enter_device_mode walks it
            unsigned char* const host = dst_on_device ? (img_pinned.reserve(L.total), img_pinned.p) : out;
            ndt_image_from_mirror(mirror, q, mirror.next_vid, mirror.flag_first_scan, L, host);
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
        const fls_ndt_image_header h = ndt_image_make_header(q, L, dev_next_vid, mirror.flag_first_scan);
        std::memcpy(img_pinned.p, &h, sizeof(h));
        FLS_HIP(hipMemsetAsync(img, 0, L.total, stream));  // the padding between the arrays
        FLS_HIP(hipMemcpyAsync(img, img_pinned.p, sizeof(h), hipMemcpyHostToDevice, stream));
        if (L.n) {
            const NdtRows R = live().rows();
            sort_rows_by_stamp(R, unsigned((dev_epoch + 2) >> 32) + 1u);  // as the eviction selection orders them
            const unsigned long long lanes = (unsigned long long)L.n * kNdtImageLanesPerVoxel;
            hipLaunchKernelGGL(ndt_image_pack_kernel, dim3(unsigned((lanes + 255ull) / 256ull)), dim3(256), 0, stream, R, (const unsigned*)ev_sort.v0,
                               (unsigned long long)L.n, int(q.max_points), img, ndt_image_offsets(L));
        }
        if (!direct) FLS_HIP(hipMemcpyAsync(out, img, L.total, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        FLS_HIP(hipGetLastError());
        ++image_exports_device;
        return FLS_OK;
    }
    // Everything is checked in the spare buffers; a refusal leaves the map untouched.  replaced(): the owner's part of taking a new map, called
    // once the checks have passed
    template <class Replaced>
    fls_status image_import(const void* src, size_t n_bytes, int src_on_device, Replaced&& replaced) {
        if (!image_fits()) return FLS_ERR_STATE;
        // (1) the header, on the host
        unsigned char head[sizeof(fls_ndt_image_header)];
        if (n_bytes < sizeof(head)) return FLS_ERR_INVALID;
        if (src_on_device) FLS_HIP(hipMemcpy(head, src, sizeof(head), hipMemcpyDeviceToHost));
        else std::memcpy(head, src, sizeof(head));
        fls_ndt_image_header h;
        NdtImageLayout L;
        const fls_status hrc = ndt_image_check_header(head, n_bytes, q, h, L);
        if (hrc != FLS_OK) return hrc;
        FLS_HIP(hipStreamSynchronize(stream));
        const bool to_device = allow_device_update && device_rows_fit() && !staying_on_host();
        const size_t n = L.n;
        NdtRowBufs& nb = bufs[live_ix ^ 1];
        unsigned ts = 0;
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
            nb.reserve(n + ahead, false, stream);
            nb.table.reserve(ts);
            img_status.reserve(1); img_status_h.reserve(1);
            FLS_HIP(hipMemsetAsync(img_status.p, 0, sizeof(unsigned), stream));
            nb.clear_touch(stream);
            const NdtRows R = nb.rows();
            const unsigned long long lanes = (unsigned long long)n * kNdtImageLanesPerVoxel;
            hipLaunchKernelGGL(ndt_table_fill_kernel, dim3((ts + 255) / 256), dim3(256), 0, stream, nb.table.p, ts);
            hipLaunchKernelGGL(ndt_image_check_unpack_kernel, dim3(unsigned((lanes + 255ull) / 256ull)), dim3(256), 0, stream, img, ndt_image_offsets(L),
                               (unsigned long long)n, int(q.max_points), int(h.next_vid), R, img_status.p);
            hipLaunchKernelGGL(ndt_table_rehash_check_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, stream, nb.table.p, ts - 1, R, unsigned(n), img_status.p);
            FLS_HIP(hipMemcpyAsync(img_status_h.p, img_status.p, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
            if (!to_device && src_on_device) {  // the mirror is built from host memory
                img_pinned.reserve(L.total);
                FLS_HIP(hipMemcpyAsync(img_pinned.p, img, L.total, hipMemcpyDeviceToHost, stream));
                host_bytes = img_pinned.p;
            }
            FLS_HIP(hipStreamSynchronize(stream));
            FLS_HIP(hipGetLastError());
            if (img_status_h.p[0] != 0u) return FLS_ERR_INVALID;  // (the map is as it was)
        }
        // (3) the map takes the image
        FLS_HIP(hipDeviceSynchronize());  // launches of the batch lanes may still hold the old buffers
        mirror.clear_mirror();
        mirror.next_vid = h.next_vid; mirror.flag_first_scan = h.flag_first_scan != 0u;
        replaced();
        ++(to_device ? image_imports_device : image_imports_mirror);
        if (n == 0) {  // an empty handle: what it was before its first cloud
            become_empty();
        } else if (to_device) {
            live_ix ^= 1;
            device_left = false;
            become_device(n, ts);
        } else {
            ndt_mirror_from_image(mirror, host_bytes, L);
            become_empty();
            rebuild_image();  // the host-path image: estimated voxels only, rows in the mirror's order
        }
        return FLS_OK;
    }

    // map_size slots (the matcher's own: 105, 106, 111)
    size_t counter(const int slot) const {
        switch (slot) {
            case 107: return size_t(full_rebuilds);  // image: full rebuilds / incremental updates
            case 108: return size_t(incremental_updates);
            case 109: return size_t(device_batches);  // map updates applied on the device / refused (replayed on the host)
            case 110: return size_t(refused_batches);
            case 112: return size_t(table_growths);  // device-side table rebuilds / row-array growths
            case 113: return size_t(row_growths);
            case 117: return size_t(device_evictions);  // voxels evicted by device batches / row compactions through the host mirror
            case 118: return size_t(device_compactions);
            case 126: return size_t(device_recreated);  // ... of which re-created by a later point of the same batch
            case 150: return size_t(device_builds);    // maps built from a whole cloud on the device / declined (host path), then why:
            case 151: return size_t(builds_declined);  // too many points, evictions the device cannot order, range or non-finite, parameters
            case 152: case 153: case 154: case 155: return size_t(declined_why[slot - 152]);
            case 156: return size_t(image_exports_device);  // flat images (fls_map_ndt.h) exported on the device / from the mirror,
            case 157: return size_t(image_exports_mirror);  // imported into device mode / through the mirror
            case 158: return size_t(image_imports_device);
            case 159: return size_t(image_imports_mirror);
            default: return alive();
        }
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
        if (!on_device()) {
            for (int vi = mirror.lru_head; vi >= 0 && w < na; vi = mirror.pool[vi].next) {
                const NdtMirror::Voxel& v = mirror.pool[vi];
                put(v.kx, v.ky, v.kz, v.vid, v.num_points, v.estimated, NdtMirror::pending_of(v, q.max_points), v.mu, v.sigma, v.info);
            }
            return w;
        }
        NdtHostRows H(dev_rows);
        H.copy(live(), dev_rows, stream, /*up=*/false);
        const std::vector<size_t> order = H.alive_oldest_first();
        for (auto it = order.rbegin(); it != order.rend() && w < na; ++it) {
            const size_t r = *it;
            int kx, ky, kz;
            unpack_key(H.key[r], kx, ky, kz);
            put(kx, ky, kz, H.vid[r], H.np[r], H.est[r] != 0, NdtMirror::pending_of(H.est[r] != 0, H.np[r], H.cc[r], q.max_points), &H.mu[3 * r], &H.sigma[9 * r], &H.info[9 * r]);
        }
        return w;
    }
};

}  // namespace fls
