// ivox_map.hpp -- the iVox local map of FLS_P2PLANE_IVOX without a matcher around it: the replacement of IVoxMap as LoamPointToPlaneIVOX
// uses it (InitIVox :53-58, the AddPoints side of AddCloudToLocalMap :60-139).  Host mirror (HostIvox) + device image (IvoxImage) + the rule
// which of the two is the map (State; diagram in DESIGN.md 3), the device-side AddPoints (enqueue_update / await_update) and the ways a
// map travels (blob, replica, flat image).  A whole cloud going into an EMPTY map is built on the device (bulk_build, kernels_ivox_build.hpp):
// the image then is the map and the mirror is only reconstructed when something asks for it.  The blob is also packed from and built into the image
// on the device (export_blob_to / import_blob_from, kernels_ivox_blob.hpp).  Everything is queued on the one stream given to init().
#pragma once
#include "ivox_image.hpp"
#include "device_voxelgrid.hpp"
#include "kernels_ivox_build.hpp"
#include "kernels_ivox_blob.hpp"
#include <chrono>
#include <algorithm>

namespace fls {

struct IvoxMap {
    HostIvox ivox;
    IvoxImage image;
    // Who holds the map, and (while the mirror does) how the image stands against it.  The image of a Device or Replica map is current by
    // definition.  Transitions: the functions marked "-> State" below, nothing else assigns `state`.
    enum class State {
        MirrorUnbuilt,  // the host mirror is the map; the image must be flattened from it (never built, or the device refused a batch for lack of room)
        MirrorStale,    // the host mirror is the map; the image lacks the mirror's journal
        MirrorCurrent,  // the host mirror is the map; the image shows it
        Device,         // the device image is the map (points, voxel table, LRU stamps, counts); the mirror is stale until to_mirror()
        ImageOnly,      // the device image is the map and nothing on the device updates it: image current, mirror NOT BUILT until to_mirror().  What
                        // bulk_build leaves where enter_device() would refuse -- every localization handle between two reloads -- complete for
                        // every reader (Match, lanes, replicas, flat image), with the AddPoints side arrays and IvoxUpdState written like a Device map's
        Replica,        // the image is a read-only copy of another map's kNN side; the mirror is empty, there is no AddPoints side
    };
    State state = State::MirrorUnbuilt;
    bool on_device() const { return state == State::Device; }
    bool image_is_map() const { return state == State::Device || state == State::ImageOnly; }  // the mirror is stale or not built
    bool is_replica() const { return state == State::Replica; }

    hipStream_t stream = nullptr;
    unsigned kind = 0;
    bool mapping_mode = true;      // !is_localization_mode: only a map that Match updates goes to the device
    bool allow_device_map = true;  // FLS_IVOX_DEVICE_UPDATE=0: always the host path (A/B)
    bool allow_device_build = true;  // FLS_IVOX_DEVICE_BUILD=0: a cloud into an empty map goes point by point through the mirror (A/B)
    bool use_dense = true;         // brick image instead of the hash table (FLS_IVOX_DENSE=0 disables; a brick pool over its budget too)
    bool is_first = true;          // the reference's function-static flag (:62), per map here
    // map_size slots 100-104, 117, 119-126 (see counter())
    size_t n_incremental = 0, n_full_rebuilds = 0;
    size_t n_device_updates = 0, n_host_fallbacks = 0, n_device_evictions = 0, n_device_recreated = 0, n_refused_conflict = 0, n_refused_full = 0, n_refused_outside = 0;
    size_t n_short_updates = 0, n_speculative = 0, n_speculative_skipped = 0;
    // map_size slots 140-147: bulk builds done / declined, declines by reason, mirrors reconstructed after a bulk build
    enum class BuildDecline { None = 0, TooMany, Capacity, Range, Budget, NotDense, SwitchedOff };
    size_t n_bulk_builds = 0, n_bulk_declined = 0, n_bulk_decline_reason[7] = {}, n_lazy_mirrors = 0;
    BuildDecline last_decline = BuildDecline::None;
    bool mirror_pending = false;  // the map came from a bulk build (or a blob built on the device) and its mirror has not been reconstructed yet
    // map_size slots 168-175: the blob packed / built on the device (include/fls_map_ivox.h)
    bool allow_device_image = true;  // FLS_IVOX_DEVICE_IMAGE=0: export_blob_to / import_blob_from take the host path (A/B)
    enum class BlobDecline { None = 0, SwitchedOff, Size, Range, Budget, NotDense };
    size_t n_blob_exports_device = 0, n_blob_exports_host = 0, n_blob_imports_device = 0, n_blob_imports_declined = 0, n_blob_decline_reason[6] = {};
    double build_ms[3] = {0, 0, 0};  // FLS_HOST_TIMING: keys + sort + scans up to the mailbox | pool set-up + cells + points | total
    // ---- device-side AddPoints: persistent state, the mailbox its commit kernel writes, the counts mirrored from it ----
    DevBuf<IvoxUpdState> d_upd_state;
    IvoxUpdMailbox* upd_mb_host = nullptr;
    IvoxUpdMailbox* upd_mb_dev = nullptr;
    unsigned upd_seq = 0;
    size_t dev_n_points = 0, dev_n_alive = 0, dev_n_bricks = 0;
    unsigned long long stamp_bound = 0;  // upper bound of every LRU stamp on the device (sizes the second sort round)
    // scratch of one update chain
    DevBuf<uint2> d_lx, d_bt;
    DevBuf<unsigned> d_seq_src, d_seq_cell, d_jj, d_tlist;
    DevBuf<uint4> d_px, d_bt2;
    DevBuf<unsigned char> d_fbit;
    DevicePairSort ev_sort;
    DevBuf<unsigned> d_ev_bt, d_crank, d_evict_list;
    PinnedBuf<char> upd_stage;
    DevBuf<unsigned> d_counter_img;
    // scratch of one bulk build
    DevicePairSort bb_sort;
    DevBuf<unsigned long long> bb_vkey;
    DevBuf<unsigned> bb_khi, bb_bt, bb_vidx, bb_first, bb_lcap, bb_btc, bb_vbegin, bb_flag;
    DevBuf<uint2> bb_lx;
    IvbMailbox* bb_mb_host = nullptr;
    IvbMailbox* bb_mb_dev = nullptr;
    unsigned bb_seq = 0;
    // the blob on the device: staging (shifted by 8 bytes: every record 16-byte aligned), the report of the checks, prefixes of the counts
    DevBuf<uint4> d_blob;
    DevBuf<IvblReport> d_blob_rep;
    DevBuf<unsigned> bl_lsrc, bl_bt;

    ~IvoxMap() {
        if (stream) (void)hipStreamSynchronize(stream);  // (the owner destroys the stream after its members)
        if (upd_mb_host) (void)hipHostFree(upd_mb_host);
        if (bb_mb_host) (void)hipHostFree(bb_mb_host);
    }
    void init(hipStream_t s, unsigned kind_, bool localization_mode) {
        stream = s; kind = kind_; mapping_mode = !localization_mode;
        if (const char* e = std::getenv("FLS_IVOX_DENSE")) use_dense = std::atoi(e) != 0;
        if (const char* e = std::getenv("FLS_IVOX_DEVICE_UPDATE")) allow_device_map = std::atoi(e) != 0;
        if (const char* e = std::getenv("FLS_IVOX_DEVICE_BUILD")) allow_device_build = std::atoi(e) != 0;
        if (const char* e = std::getenv("FLS_IVOX_DEVICE_IMAGE")) allow_device_image = std::atoi(e) != 0;
        d_upd_state.reserve(1);
        FLS_HIP(hipHostMalloc((void**)&upd_mb_host, sizeof(IvoxUpdMailbox), hipHostMallocMapped));
        std::memset(upd_mb_host, 0, sizeof(IvoxUpdMailbox));
        FLS_HIP(hipHostGetDevicePointer((void**)&upd_mb_dev, upd_mb_host, 0));
        ivox.resolution = 0.5f;       // InitIVox :53-58
        ivox.inv_resolution = 1.0f / 0.5f;
        ivox.capacity = 1000000;
        if (const char* e = std::getenv("FLS_IVOX_CAPACITY")) { const long c = std::atol(e); if (c > 1) ivox.capacity = size_t(c); }  // test hook (LRU eviction)
    }

    // ---- transitions ----
    // -> MirrorStale (MirrorUnbuilt stays).  Pre: the mirror is the map and the caller has inserted into `ivox`.
    void mirror_changed() { if (state == State::MirrorCurrent) state = State::MirrorStale; }
    // -> MirrorUnbuilt, the mirror empty.  Pre: none (the stream idle if the image may be in use).
    void become_empty() { ivox.clear(); state = State::MirrorUnbuilt; mirror_pending = false; }
    // -> Replica.  Pre: become_empty(), then `image` filled with a complete kNN side (clone_for_reading / import_flat).
    void become_replica() { state = State::Replica; }
    // -> MirrorCurrent, then Device where enter_device() allows.  Pre: none; a Device, ImageOnly, Replica or MirrorCurrent map is left as it is.
    // Scatters the mirror's journal into the image when possible, else re-flattens.
    void refresh() {
        if (state != State::MirrorUnbuilt && state != State::MirrorStale) return;
        image.want_hash = !use_dense;
        if (state == State::MirrorStale && image.collect_incremental(ivox)) {
            if (image.dir_dirty) image.upload_directory(stream);  // the host path created bricks (their slabs are still zero)
            image.scatter_cell_records(stream, upd_stage);
            ++n_incremental;
        } else {
            image.build_from_ivox(ivox, stream, upd_stage);
            if (image.budget_exceeded) use_dense = false;  // brick pool over its byte budget: per-voxel hash table from now on (map_size(132))
            ++n_full_rebuilds;
        }
        state = State::MirrorCurrent;
        enter_device();
    }
    // -> Device.  Pre: MirrorCurrent.  Hands the map over to the device-side AddPoints: the brick image has no extent limit, so the only
    // conditions are the A/B switch, a brick image, mapping mode and an LRU capacity the eviction selection can work with.
    bool device_update_allowed() const { return allow_device_map && use_dense && image.have_bricks && !image.want_hash && mapping_mode && ivox.capacity >= 4; }
    void enter_device() {
        if (!device_update_allowed()) return;
        const unsigned long long stamp_base = image.upload_update_meta(ivox, stream, upd_stage);
        IvoxUpdState st{};
        st.n_points = ivox.n_points; st.used = image.used; st.garbage = image.garbage; st.stamp_base = stamp_base;
        st.pts_capacity = image.d_pts.cap; st.n_alive = unsigned(ivox.n_alive); st.lru_capacity = unsigned(std::min<size_t>(ivox.capacity, 0xffffffffu));
        st.next_id = ivox.next_id;
        st.n_bricks = unsigned(image.n_bricks());
        FLS_HIP(hipMemcpyAsync(d_upd_state.p, &st, sizeof(st), hipMemcpyHostToDevice, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        dev_n_points = ivox.n_points; dev_n_alive = ivox.n_alive; dev_n_bricks = image.n_bricks();
        stamp_bound = stamp_base;
        state = State::Device;
    }
    // -> MirrorCurrent.  Pre: none; anything but a Device or ImageOnly map is left as it is.  The device image back into the host mirror: the
    // alive voxels as records (one compaction kernel), their points, the LRU order from the stamps, and the bricks the device created.  After a
    // bulk build this is where the mirror is built at all, the first time something needs it (export_blob, a host fallback, an external add_cloud).
    void to_mirror() {
        if (!image_is_map()) return;
        if (mirror_pending) { ++n_lazy_mirrors; mirror_pending = false; }
        if (image.dir.size() != size_t(image.dir_mask) + 1) image.dir.assign(size_t(image.dir_mask) + 1, HashEntry{kEmptyKey, kBrickPending, 0u});  // (a bulk build keeps no host copy)
        IvoxUpdState st{};
        FLS_HIP(hipMemcpyAsync(&st, d_upd_state.p, sizeof(st), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        const size_t nb = std::min<size_t>(st.n_bricks, image.n_bricks_cap), ncell = nb * kBrickStride, n_alive = st.n_alive;
        image.d_alive_rec.reserve(std::max<size_t>(n_alive, 1));
        image.d_counter.reserve(1);
        FLS_HIP(hipMemsetAsync(image.d_counter.p, 0, sizeof(unsigned), stream));
        if (ncell)
            hipLaunchKernelGGL(ivox_list_alive_kernel, dim3(unsigned((ncell + 255) / 256)), dim3(256), 0, stream, (const uint2*)image.d_cells.p,
                               (const unsigned long long*)image.d_brick_key.p, unsigned(ncell), (const unsigned char*)image.d_cap_log2.p,
                               (const unsigned long long*)image.d_stamp.p, image.d_alive_rec.p, image.d_counter.p, unsigned(n_alive));
        FLS_HIP(hipGetLastError());
        unsigned n_listed = 0;
        std::vector<IvoxAliveRec> recs(n_alive);
        std::vector<Pt4> pts(st.used);
        FLS_HIP(hipMemcpyAsync(&n_listed, image.d_counter.p, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
        if (n_alive) FLS_HIP(hipMemcpyAsync(recs.data(), image.d_alive_rec.p, n_alive * sizeof(IvoxAliveRec), hipMemcpyDeviceToHost, stream));
        if (st.used) FLS_HIP(hipMemcpyAsync(pts.data(), image.d_pts.p, st.used * sizeof(Pt4), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        if (n_listed != n_alive) throw std::runtime_error("iVox image: the alive-voxel count of the device state does not match its cells");
        image.download_directory(nb, stream);
        std::vector<HostIvox::ImageVoxel> vox;
        vox.reserve(n_alive);
        for (const IvoxAliveRec& r : recs) vox.push_back(HostIvox::ImageVoxel{r.key, r.begin, r.count, r.cap_log2 ? (1u << r.cap_log2) : 0u, r.stamp});
        load_mirror(vox, pts.data(), size_t(st.n_points), st.next_id);
        image.used = size_t(st.used);
        image.garbage = size_t(st.garbage);
        image.n_pts_live = size_t(st.n_points);
        state = State::MirrorCurrent;
    }
    // what await_update learned of the batch queued last
    enum class Verdict {
        Applied,
        Skipped,         // a speculative chain that found nothing to do: nothing ran
        Refused,         // an eviction-order conflict or a point outside the key range: nothing was applied
        RefusedForRoom,  // the point array or the brick pool is full: nothing was applied, the image needs more room
    };
    // -> MirrorCurrent, or MirrorUnbuilt after RefusedForRoom (the next refresh re-flattens with more room).  Pre: Device, and the batch
    // at hand was refused (`v`) or is too large for the device (Refused).  The caller replays it on the mirror.
    void fall_back(const Verdict v) {
        ++n_host_fallbacks;
        to_mirror();
        if (v == Verdict::RefusedForRoom) state = State::MirrorUnbuilt;
    }


    // ---- a whole cloud into the EMPTY map, on the device (kernels_ivox_build.hpp; the closed form is DESIGN.md 3) ----
    bool decline_build(const BuildDecline why) {
        last_decline = why;
        ++n_bulk_declined;
        ++n_bulk_decline_reason[int(why)];
        return false;
    }
    // what can be said before the cloud is touched.  false: declined (counted), the caller takes the host path.
    bool bulk_build_applies(const size_t n) {
        if (!allow_device_build) return decline_build(BuildDecline::SwitchedOff);
        if (!use_dense) return decline_build(BuildDecline::NotDense);
        if (n > size_t(kVgMaxBlocks) * kVgTile) return decline_build(BuildDecline::TooMany);
        return true;
    }
    bool is_blank() const { return state == State::MirrorUnbuilt && ivox.n_alive == 0 && ivox.next_id == 0; }
    // The image's arrays sized and cleared for V voxels in `used` slots, and the voxels' cells written by `launch_cells` (ivb_cells, or ivbl_cells
    // for the voxels of a blob) -- shared by bulk_build and import_blob_device.  Point array: the growth room build_from_ivox reserves.  Brick pool:
    // its rule too -- three times the voxels' own bricks as a first guess, room for as many bricks again once they are all there, never over the
    // byte budget (the host path then takes the hash-table form).  false: over the budget, the stream idle.  true: the cells launch that passed
    // is complete, IvoxUpdState is set.
    struct BuiltPool { size_t dir_size = 0, n_bricks_cap = 0, n_bricks_made = 0; };
    template <class LaunchCells>
    bool build_brick_pool(const size_t own, const size_t used, const size_t n_points, const size_t V, const int next_id, const unsigned long long stamp_base, BuiltPool& out,
                          LaunchCells&& launch_cells) {
        image.d_pts.reserve(used + used / 2 + (size_t(1) << 16));
        size_t cap_guess = std::max<size_t>(image.n_bricks_cap, 256), ds = 0, n_bricks_made = 0;
        while (cap_guess < 3 * own) cap_guess *= 2;
        for (;;) {
            if (cap_guess * IvoxImage::kPoolBrickBytes > IvoxImage::brick_budget_bytes()) {
                FLS_HIP(hipStreamSynchronize(stream));
                return false;
            }
            ds = 4096;
            while (ds < 4 * cap_guess) ds <<= 1;
            const size_t ncell = cap_guess * kBrickStride;
            image.d_dir.reserve(ds); image.d_brick_key.reserve(cap_guess); image.d_cells.reserve(ncell); image.d_nbr.reserve(cap_guess * 32);
            image.d_cap_log2.reserve(ncell); image.d_stamp.reserve(ncell); image.d_pend.reserve(ncell); image.d_rank_mm.reserve(ncell);
            FLS_HIP(hipMemsetAsync(image.d_dir.p, 0xff, ds * sizeof(HashEntry), stream));  // every entry {kEmptyKey, kBrickPending, -}
            FLS_HIP(hipMemsetAsync(image.d_cells.p, 0, ncell * sizeof(uint2), stream));
            FLS_HIP(hipMemsetAsync(image.d_nbr.p, 0xff, cap_guess * 32 * sizeof(unsigned), stream));
            FLS_HIP(hipMemsetAsync(image.d_cap_log2.p, 0, ncell, stream));
            FLS_HIP(hipMemsetAsync(image.d_stamp.p, 0, ncell * sizeof(unsigned long long), stream));
            FLS_HIP(hipMemsetAsync(image.d_pend.p, 0, ncell * sizeof(unsigned), stream));
            FLS_HIP(hipMemsetAsync(image.d_rank_mm.p, 0xff, ncell * sizeof(unsigned), stream));
            IvoxUpdState st{};
            st.n_points = n_points; st.used = used; st.garbage = 0; st.stamp_base = stamp_base;
            st.pts_capacity = image.d_pts.cap; st.n_alive = unsigned(V); st.lru_capacity = unsigned(std::min<size_t>(ivox.capacity, 0xffffffffu));
            st.next_id = next_id; st.n_bricks = 0u; st.status = kUpdOk;
            FLS_HIP(hipMemcpyAsync(d_upd_state.p, &st, sizeof(st), hipMemcpyHostToDevice, stream));
            const IvoxUpdArrays a{image.d_cells.p, image.d_pts.p, image.d_cap_log2.p, image.d_stamp.p, image.d_pend.p, image.d_rank_mm.p,
                                  image.d_dir.p, unsigned(ds - 1), unsigned(cap_guess), image.d_brick_key.p, image.d_nbr.p, ivox.inv_resolution};
            launch_cells(a);
            FLS_HIP(hipGetLastError());
            FLS_HIP(hipMemcpyAsync(&st, d_upd_state.p, sizeof(st), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            n_bricks_made = st.n_bricks;
            if (!(st.status & kUpdArrayFull) && 2 * n_bricks_made <= cap_guess) break;
            cap_guess = std::max(cap_guess * 2, 2 * n_bricks_made);  // (a refused launch counted every brick it wanted)
        }
        out = BuiltPool{ds, cap_guess, n_bricks_made};
        return true;
    }
    // -> Device where enter_device() would go there, else ImageOnly.  Pre: build_brick_pool passed, the points are in their regions, the stream idle.
    void adopt_built_image(const BuiltPool& pool, const size_t used, const size_t n_points, const size_t V, const unsigned long long stamp_base) {
        image.want_hash = false; image.have_bricks = true;
        image.table.clear(); image.mask = 0;
        image.brick_index.clear(); image.brick_keys.clear(); image.dir.clear(); image.dir_dirty = false;  // (no host copy of the directory: to_mirror downloads it)
        image.dir_mask = unsigned(pool.dir_size - 1); image.n_bricks_cap = pool.n_bricks_cap; image.meta_cells = pool.n_bricks_cap * kBrickStride;
        image.cell_upd.clear(); image.pt_upd.clear();
        image.used = used; image.garbage = 0; image.n_pts_live = n_points;
        dev_n_points = n_points; dev_n_alive = V; dev_n_bricks = pool.n_bricks_made;
        stamp_bound = stamp_base;
        mirror_pending = true;
        state = device_update_allowed() ? State::Device : State::ImageOnly;
    }
    // -> Device where enter_device() would go there, else ImageOnly.  Pre: is_blank(), bulk_build_applies(n), n > 0; x | y | z the cloud on the
    // device, lo / hi its coordinate bounds over the points that are not NaN (round() is monotone: the extreme keys come from the extreme
    // coordinates).  false: declined (counted), nothing the host path relies on was changed.  One host wait inside (the mailbox of ivb_report),
    // one at the end (the call returns with the stream idle, like refresh()).
    bool bulk_build(const float* x, const float* y, const float* z, const size_t n, const float (&lo)[3], const float (&hi)[3]) {
        using clock = std::chrono::steady_clock;
        const auto t0 = clock::now();
        IvbExtent ext{};
        int span_bits[3];
        for (int a = 0; a < 3; ++a) {
            const float flo = std::round(lo[a] * ivox.inv_resolution), fhi = std::round(hi[a] * ivox.inv_resolution);
            if (!(std::fabs(flo) < float(kKeyLimit) && std::fabs(fhi) < float(kKeyLimit))) return decline_build(BuildDecline::Range);  // (an extreme point fails key_of)
            ext.bmin[a] = int(flo) >> kBrickLog;
            const unsigned span = unsigned((int(fhi) >> kBrickLog) - ext.bmin[a]);
            span_bits[a] = 0;
            while ((1u << span_bits[a]) <= span) ++span_bits[a];
        }
        ext.bx_bits = span_bits[0]; ext.by_bits = span_bits[1];
        const int key_bits = span_bits[0] + span_bits[1] + span_bits[2] + 3 * kBrickLog;  // <= 3 * 18 + 9
        const bool wide = key_bits > 32;
        const int ni = int(n), nblk = (ni + kIvbBlock - 1) / kIvbBlock;
        const dim3 g{unsigned(nblk), 1u, 1u}, t{unsigned(kIvbBlock), 1u, 1u};
        if (!bb_mb_host) {
            FLS_HIP(hipHostMalloc((void**)&bb_mb_host, sizeof(IvbMailbox), hipHostMallocMapped));
            std::memset(bb_mb_host, 0, sizeof(IvbMailbox));
            FLS_HIP(hipHostGetDevicePointer((void**)&bb_mb_dev, bb_mb_host, 0));
        }
        bb_sort.prepare(n);
        bb_vkey.reserve(n); if (wide) bb_khi.reserve(n);
        bb_lx.reserve(n); bb_vidx.reserve(n); bb_first.reserve(n + 1); bb_lcap.reserve(n); bb_vbegin.reserve(n);
        bb_bt.reserve(size_t(4) * nblk + 1); bb_btc.reserve(size_t(2) * nblk + 1); bb_flag.reserve(1);
        unsigned* const bts = bb_bt.p + 2 * nblk;    // scanned: voxel heads | brick heads, then the total
        unsigned* const btcs = bb_btc.p + nblk;      // scanned capacities, then the total (= used)
        FLS_HIP(hipMemsetAsync(bb_flag.p, 0, sizeof(unsigned), stream));
        hipLaunchKernelGGL(ivb_keys, g, t, 0, stream, x, y, z, ni, ivox.inv_resolution, ext, bb_vkey.p, bb_sort.k0, wide ? bb_khi.p : (unsigned*)nullptr, bb_sort.v0, bb_flag.p);
        bb_sort.run((std::min(key_bits, 32) + 7) / 8, stream);
        if (wide) {  // two stable rounds, low word first (as the eviction selection sorts its 64-bit stamps)
            hipLaunchKernelGGL(ivb_gather_hi, g, t, 0, stream, (const unsigned*)bb_khi.p, (const unsigned*)bb_sort.v0, ni, bb_sort.k0);
            bb_sort.run((key_bits - 32 + 7) / 8, stream);
        }
        const unsigned* const order = bb_sort.v0;
        hipLaunchKernelGGL(ivb_heads, g, t, 0, stream, (const unsigned long long*)bb_vkey.p, order, ni, bb_lx.p, bb_bt.p);
        hipLaunchKernelGGL(vg_scan, dim3(1), dim3(kVgScanBlock), 0, stream, (const unsigned*)bb_bt.p, bts, 2 * nblk, bts + 2 * nblk);
        const unsigned* const d_n_voxels = bts + nblk;  // (the scan's value at the seam of the two planes)
        hipLaunchKernelGGL(ivb_voxels, g, t, 0, stream, (const uint2*)bb_lx.p, (const unsigned*)bts, ni, bb_vidx.p, bb_first.p);
        hipLaunchKernelGGL(ivb_caps, g, t, 0, stream, (const unsigned*)bb_first.p, d_n_voxels, bb_lcap.p, bb_btc.p);
        hipLaunchKernelGGL(vg_scan, dim3(1), dim3(kVgScanBlock), 0, stream, (const unsigned*)bb_btc.p, btcs, nblk, btcs + nblk);
        bb_seq = (bb_seq + 1u) & 0x7fffffffu;
        if (bb_seq == 0u) bb_seq = 1u;
        hipLaunchKernelGGL(ivb_report, dim3(1), dim3(64), 0, stream, (const unsigned*)bb_flag.p, d_n_voxels, (const unsigned*)(bts + 2 * nblk), (const unsigned*)(btcs + nblk), bb_mb_dev, bb_seq);
        FLS_HIP(hipGetLastError());
        (void)spin_until(stream, [&] { return __atomic_load_n(&bb_mb_host->seq, __ATOMIC_ACQUIRE) == bb_seq; });
        if (__atomic_load_n(&bb_mb_host->seq, __ATOMIC_ACQUIRE) != bb_seq) FLS_HIP(hipErrorUnknown);  // (the stream went idle without a report)
        const auto t1 = clock::now();
        if (bb_mb_host->flag != 0u) return decline_build(BuildDecline::Range);
        const size_t V = bb_mb_host->n_voxels, own = bb_mb_host->own_bricks, used = size_t(bb_mb_host->used);
        if (V >= ivox.capacity) return decline_build(BuildDecline::Capacity);  // (evict_tail fires when n_alive >= capacity after a creation)
        BuiltPool pool;
        // (stamps are 1 .. n: index of the last member + 1)
        if (!build_brick_pool(own, used, n, V, /*next_id=*/int(n), /*stamp_base=*/n, pool, [&](const IvoxUpdArrays& a) {
                hipLaunchKernelGGL(ivb_cells, g, t, 0, stream, (const unsigned long long*)bb_vkey.p, order, (const unsigned*)bb_first.p, unsigned(V), (const unsigned*)bb_lcap.p,
                                   (const unsigned*)btcs, a, d_upd_state.p, bb_vbegin.p);
            }))
            return decline_build(BuildDecline::Budget);
        // (ivb_points reads the region begins ivb_cells writes: queued behind the launch that passed)
        hipLaunchKernelGGL(ivb_points, g, t, 0, stream, x, y, z, order, ni, (const unsigned*)bb_vidx.p, (const unsigned*)bb_first.p, (const unsigned*)bb_vbegin.p, image.d_pts.p,
                           (unsigned long long)image.d_pts.cap);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipStreamSynchronize(stream));
        adopt_built_image(pool, used, n, V, /*stamp_base=*/n);
        ++n_bulk_builds;
        last_decline = BuildDecline::None;
        const auto t2 = clock::now();
        build_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
        build_ms[1] = std::chrono::duration<double, std::milli>(t2 - t1).count();
        build_ms[2] = std::chrono::duration<double, std::milli>(t2 - t0).count();
        return true;
    }

    // ---- the device-side AddPoints ----
    static int update_blocks(const size_t n) { return int((n + kUpdBlock - 1) / kUpdBlock); }
    // the count side of a batch of n points, for the launch that decides the insertion codes (it then counts them per block and opens the
    // batch: ivox_upd_count's job).  All null unless the device holds the map and the batch fits one scan workgroup.
    struct CountArgs { uint2 *lx = nullptr, *bt = nullptr; unsigned *status = nullptr, *apply = nullptr; };
    CountArgs count_args(const size_t n) {
        const int nb = update_blocks(n);
        if (!on_device() || nb > kUpdMaxBlocks) return CountArgs{};
        d_lx.reserve(n); d_bt.reserve(size_t(nb));
        return CountArgs{d_lx.p, d_bt.p, &d_upd_state.p->status, &d_upd_state.p->apply};
    }
    // a batch of n points takes the short chain behind a counting decision launch: it fits and cannot reach the LRU capacity
    bool short_chain_applies(const size_t n) const { return on_device() && dev_n_alive + n < ivox.capacity && update_blocks(n) <= kUpdMaxBlocks; }
    // The launches of one batch (no waiting): `code` / `pw` are the decision launch's insertion codes and world points, `counted` says it
    // has counted them (count_args).  Pre: Device.  false: the batch is too large for the device path, nothing was queued.
    // Two forms of the same phases (kernels_ivox_update.hpp): the SHORT chain (five launches behind the decision) and the LONG chain,
    // which batches that may reach the LRU capacity need (the eviction selection has grid-wide steps of its own).
    bool enqueue_update(const unsigned char* code, const float4* pw, const size_t n, const bool counted) {
        const int nb = update_blocks(n);
        if (nb > kUpdMaxBlocks) return false;
        d_lx.reserve(n); d_bt.reserve(size_t(nb)); d_seq_src.reserve(n); d_seq_cell.reserve(n); d_jj.reserve(n); d_tlist.reserve(n);
        d_px.reserve(n); d_bt2.reserve(size_t(nb)); d_fbit.reserve(n);
        const IvoxUpdBatch b{code, pw, int(n), d_lx.p, d_bt.p, d_seq_src.p, d_seq_cell.p, d_jj.p, d_px.p, d_bt2.p, d_fbit.p, d_tlist.p};
        const IvoxUpdArrays a{image.d_cells.p, image.d_pts.p, image.d_cap_log2.p, image.d_stamp.p, image.d_pend.p, image.d_rank_mm.p,
                              image.d_dir.p, image.dir_mask, unsigned(image.n_bricks_cap), image.d_brick_key.p, image.d_nbr.p, ivox.inv_resolution};
        upd_seq = (upd_seq + 1u) & 0x7fffffffu;
        if (upd_seq == 0u) upd_seq = 1u;
        const dim3 g{unsigned(nb), 1u, 1u}, t{unsigned(kUpdBlock), 1u, 1u};
        IvoxUpdState* const st = d_upd_state.p;
        const IvoxUpdState* const cst = st;
        const bool short_chain = dev_n_alive + n < ivox.capacity && counted;
        if (short_chain) {
            hipLaunchKernelGGL(ivox_upd_seq_nb, g, t, 0, stream, b, a, st, nb);
        } else {
            hipLaunchKernelGGL(ivox_upd_count, g, t, 0, stream, b);
            hipLaunchKernelGGL(ivox_upd_scan1, dim3(1), dim3(kUpdMaxBlocks), 0, stream, b, nb, st);
            hipLaunchKernelGGL(ivox_upd_seq, g, t, 0, stream, b, a, st);
        }
        hipLaunchKernelGGL(ivox_upd_plan, g, t, 0, stream, b, a, cst);
        if (short_chain) {
            hipLaunchKernelGGL(ivox_upd_last_regions, g, t, 0, stream, b, a, st);
            ++n_short_updates;
        } else {
            // LRU evictions inside the batch: whenever the batch COULD reach the capacity (every point a new voxel), the alive cells are
            // listed and sorted by their 64-bit stamp (two stable 32-bit radix rounds) so that scan2 / ivox_evict_check can pick the tail
            const bool may_evict = dev_n_alive + n >= ivox.capacity && dev_n_alive > 0;
            const unsigned n_list = may_evict ? unsigned(dev_n_alive) : 0u;
            if (may_evict) {
                const unsigned ncell = unsigned(dev_n_bricks * kBrickStride), nbe = (ncell + kEvBlock - 1) / kEvBlock;  // (bricks this batch creates hold no candidate)
                d_ev_bt.reserve(size_t(2) * nbe);
                ev_sort.prepare(n_list);
                hipLaunchKernelGGL(ivox_evict_count, dim3(nbe), dim3(kEvBlock), 0, stream, (const uint2*)image.d_cells.p, ncell, d_ev_bt.p);
                hipLaunchKernelGGL(vg_scan, dim3(1), dim3(kVgScanBlock), 0, stream, (const unsigned*)d_ev_bt.p, d_ev_bt.p + nbe, int(nbe), (unsigned*)nullptr);
                hipLaunchKernelGGL(ivox_evict_list, dim3(nbe), dim3(kEvBlock), 0, stream, (const uint2*)image.d_cells.p, (const unsigned long long*)image.d_stamp.p, ncell,
                                   (const unsigned*)(d_ev_bt.p + nbe), ev_sort.k0, ev_sort.v0);
                ev_sort.run(4, stream);
                hipLaunchKernelGGL(ivox_evict_hikeys, dim3((n_list + 255u) / 256u), dim3(256), 0, stream, (const unsigned long long*)image.d_stamp.p,
                                   (const unsigned*)ev_sort.v0, n_list, ev_sort.k0);
                ev_sort.run(DevicePairSort::passes_for((unsigned long long)((stamp_bound + n) >> 32) + 1ull), stream);
            }
            hipLaunchKernelGGL(ivox_upd_scan2, dim3(1), dim3(kUpdMaxBlocks), 0, stream, b, st, may_evict ? 1u : 0u, n_list);  // (also decides when no eviction selection follows)
            if (may_evict) {
                d_crank.reserve(n);
                d_evict_list.reserve(n);
                hipLaunchKernelGGL(ivox_upd_cranks, g, t, 0, stream, b, a, cst, d_crank.p);
                hipLaunchKernelGGL(ivox_evict_select, dim3(1), dim3(kEvBlock), 0, stream, (const unsigned*)ev_sort.v0, a, st, (const unsigned*)d_crank.p, d_evict_list.p);
                // voxels the selection evicts BEFORE their first point of this batch arrives are re-created by it (such a batch used to be
                // refused): the plan runs again seeing them as creations, and the totals / block offsets / point-array check with it
                hipLaunchKernelGGL(ivox_upd_plan, g, t, 0, stream, b, a, cst);
                hipLaunchKernelGGL(ivox_upd_scan2_again, dim3(1), dim3(kUpdMaxBlocks), 0, stream, b, st);
                hipLaunchKernelGGL(ivox_upd_decide, dim3(1), dim3(64), 0, stream, st);  // (the selection may still refuse the batch)
                hipLaunchKernelGGL(ivox_evict_apply, g, t, 0, stream, (const unsigned*)d_evict_list.p, a, st);
            }
            hipLaunchKernelGGL(ivox_upd_last, g, t, 0, stream, b, a, cst);
            hipLaunchKernelGGL(ivox_upd_regions, g, t, 0, stream, b, a, cst);
        }
        hipLaunchKernelGGL(ivox_upd_points, g, t, 0, stream, b, a, cst);
        hipLaunchKernelGGL(ivox_upd_finish, dim3(unsigned((n + kUpdBlock / 64 - 1) / (kUpdBlock / 64))), t, 0, stream, b, a, cst);
        hipLaunchKernelGGL(ivox_upd_commit, dim3(1), dim3(64), 0, stream, st, upd_mb_dev, upd_seq, unsigned(image.n_bricks_cap));
        FLS_HIP(hipGetLastError());
        return true;
    }
    // The verdict of the batch of n points queued last.  Pre: Device.  (A few words in host-mapped memory: no copy, no stream synchronisation.)
    Verdict await_update(const size_t n) {
        (void)spin_until(stream, [&] { return __atomic_load_n(&upd_mb_host->seq, __ATOMIC_ACQUIRE) == upd_seq; });  // (a drained stream just ends the wait)
        dev_n_bricks = std::min<size_t>(upd_mb_host->n_bricks, image.n_bricks_cap);  // (bricks are created whatever the verdict)
        const unsigned status = upd_mb_host->status;
        if (status & kUpdSkipped) return Verdict::Skipped;
        if (status != kUpdOk) {
            if (status & kUpdEvictConflict) ++n_refused_conflict;
            if (status & kUpdArrayFull) ++n_refused_full;
            if (status & kUpdOutside) ++n_refused_outside;
            return (status & kUpdArrayFull) ? Verdict::RefusedForRoom : Verdict::Refused;
        }
        dev_n_points = size_t(upd_mb_host->n_points);
        dev_n_alive = size_t(upd_mb_host->n_alive);
        stamp_bound += n;
        n_device_evictions += upd_mb_host->evicted;
        n_device_recreated += upd_mb_host->recreated;
        ++n_device_updates;
        return Verdict::Applied;
    }

    // slots in use + bricks, from the device's own state while it maintains the map
    size_t live_counts(size_t& n_bricks_live) {
        if (!image_is_map()) { n_bricks_live = image.n_bricks(); return image.used; }
        IvoxUpdState st{};
        FLS_HIP(hipMemcpyAsync(&st, d_upd_state.p, sizeof(st), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        n_bricks_live = std::min<size_t>(st.n_bricks, image.n_bricks_cap);
        return size_t(st.used);
    }
    // the mirror from voxel records + their points; resolution and capacity are the map's own, not the records'
    void load_mirror(std::vector<HostIvox::ImageVoxel>& vox, const Pt4* pts, const size_t n_points, const int next_id) {
        const float res = ivox.resolution, inv = ivox.inv_resolution;
        const size_t capacity = ivox.capacity;
        ivox.rebuild_from_image(vox, pts, n_points, next_id);
        ivox.resolution = res; ivox.inv_resolution = inv; ivox.capacity = capacity;
    }

    // ---- map export / import (fls_reg.h): header, voxels from the LRU tail (oldest) to the head {key, count}, then the
    // points {x, y, z, id} of the voxels in the same order
    using BlobHeader = fls_ivox_blob_header;  // (include/fls_map_ivox.h documents the layout)
    using BlobVoxel = fls_ivox_blob_voxel;
    // Pre: not a Replica.  A Device map passes through the mirror and goes back to the device.
    size_t export_blob(void* blob, size_t cap) {
        const bool was_device = on_device();
        to_mirror();
        const size_t need = sizeof(BlobHeader) + ivox.n_alive * sizeof(BlobVoxel) + ivox.n_points * sizeof(Pt4);
        if (blob && cap >= need) {
            char* w = static_cast<char*>(blob);
            BlobHeader hd{};
            std::memcpy(hd.magic, "FLSIVOX1", 8);
            hd.version = FLS_IVOX_BLOB_VERSION; hd.kind = kind; hd.resolution = ivox.resolution; hd.is_first = is_first ? 1u : 0u;
            hd.capacity = ivox.capacity; hd.n_voxels = ivox.n_alive; hd.n_points = ivox.n_points; hd.next_id = ivox.next_id;
            std::memcpy(w, &hd, sizeof(hd));
            BlobVoxel* bv = reinterpret_cast<BlobVoxel*>(w + sizeof(hd));
            Pt4* bp = reinterpret_cast<Pt4*>(w + sizeof(hd) + ivox.n_alive * sizeof(BlobVoxel));
            size_t k = 0, q = 0;
            for (int v = ivox.tail; v >= 0; v = ivox.pool[v].prev) {
                const HostIvox::Voxel& vx = ivox.pool[v];
                bv[k++] = BlobVoxel{vx.key, unsigned(vx.pts.size()), 0u};
                std::memcpy(bp + q, vx.pts.data(), vx.pts.size() * sizeof(Pt4));
                q += vx.pts.size();
            }
        }
        if (was_device) enter_device();
        return need;
    }
    // Any state -> an ordinary map holding the blob's voxels (refreshed: MirrorCurrent or Device).  An invalid blob leaves the map as it was.
    fls_status import_blob(const void* blob, size_t n) {
        const char* r = static_cast<const char*>(blob);
        BlobHeader hd;
        // the header is untrusted (ivox_blob_check_header), and so are the records: every voxel non-empty and unique, the counts must add up in 64 bits
        if (ivox_blob_check_header(blob, n, kind, ivox.resolution, hd) != FLS_OK) return FLS_ERR_INVALID;
        const BlobVoxel* bv = reinterpret_cast<const BlobVoxel*>(r + sizeof(hd));
        const Pt4* bp = reinterpret_cast<const Pt4*>(r + sizeof(hd) + hd.n_voxels * sizeof(BlobVoxel));
        std::vector<HostIvox::ImageVoxel> vox(size_t(hd.n_voxels));
        unsigned long long qsum = 0;
        for (size_t k = 0; k < vox.size(); ++k) {  // stamp = position in the LRU order (tail first)
            if (bv[k].count == 0u || qsum + bv[k].count > hd.n_points) return FLS_ERR_INVALID;
            vox[k] = HostIvox::ImageVoxel{bv[k].key, unsigned(qsum), bv[k].count, 0u, (unsigned long long)(k + 1)};
            qsum += bv[k].count;
        }
        if (qsum != hd.n_points) return FLS_ERR_INVALID;
        {
            std::vector<unsigned long long> keys(vox.size());
            for (size_t k = 0; k < vox.size(); ++k) keys[k] = vox[k].key;
            std::sort(keys.begin(), keys.end());
            if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return FLS_ERR_INVALID;  // a voxel listed twice
        }
        become_empty();  // (the slot layout is rebuilt from the mirror, window order, like the first build of the exporter)
        load_mirror(vox, bp, size_t(hd.n_points), int(hd.next_id));  // (the resolution is the blob's: checked equal above)
        is_first = hd.is_first != 0;
        refresh();
        return FLS_OK;
    }

    // ---- the same blob at device speed (include/fls_map_ivox.h; kernels_ivox_blob.hpp): packed from the image and built into it without the mirror.
    // `dst` / `src`: memory of this map's device (on_device) or host memory.  The kernels work in d_blob, where the blob starts 8 bytes behind a
    // 16-byte boundary so that its records (behind the 56-byte header) are 16-byte aligned; one copy moves it to or from the caller's memory.
    static constexpr size_t kBlobSortMax = size_t(kVgMaxBlocks) * kVgTile;  // records the radix sort takes
    size_t blob_bytes() const {  // (from the counts the host holds: no mirror, no download)
        return sizeof(BlobHeader) + ((image_is_map() ? dev_n_alive : ivox.n_alive) + (image_is_map() ? dev_n_points : ivox.n_points)) * 16;
    }
    char* blob_staging(const size_t n_bytes) {
        d_blob.reserve(n_bytes / 16 + 2);
        return reinterpret_cast<char*>(d_blob.p) + 8;
    }
    // Pre: not a Replica; a queued update chain settled (Match returns with it collected).  A Device / ImageOnly map stays in its state.
    fls_status export_blob_to(void* dst, const size_t cap, const bool dst_on_device) {
        if (!dst) return FLS_ERR_INVALID;
        if (image_is_map() && allow_device_image && dev_n_alive <= kBlobSortMax) return export_blob_device(dst, cap, dst_on_device);
        const size_t need = blob_bytes();
        if (cap < need) return FLS_ERR_RANGE;
        if (!dst_on_device) {
            if (export_blob(dst, cap) != need) return FLS_ERR_STATE;
        } else {
            std::vector<char> host(need);
            if (export_blob(host.data(), need) != need) return FLS_ERR_STATE;
            FLS_HIP(hipMemcpy(dst, host.data(), need, hipMemcpyHostToDevice));
        }
        ++n_blob_exports_host;
        return FLS_OK;
    }
    fls_status export_blob_device(void* dst, const size_t cap, const bool dst_on_device) {
        FLS_HIP(hipStreamSynchronize(stream));
        IvoxUpdState st{};
        FLS_HIP(hipMemcpyAsync(&st, d_upd_state.p, sizeof(st), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        const size_t V = st.n_alive, P = size_t(st.n_points), need = sizeof(BlobHeader) + (V + P) * 16;
        if (V != dev_n_alive || P != dev_n_points) throw std::runtime_error("iVox image: the device state does not match the counts the host holds");
        if (cap < need) return FLS_ERR_RANGE;
        char* const base = blob_staging(need);
        BlobHeader hd{};
        std::memcpy(hd.magic, FLS_IVOX_BLOB_MAGIC, 8);
        hd.version = FLS_IVOX_BLOB_VERSION; hd.kind = kind; hd.resolution = ivox.resolution; hd.is_first = is_first ? 1u : 0u;
        hd.capacity = ivox.capacity; hd.n_voxels = V; hd.n_points = P; hd.next_id = st.next_id;
        FLS_HIP(hipMemcpyAsync(base, &hd, sizeof(hd), hipMemcpyHostToDevice, stream));
        if (V) {
            const unsigned n = unsigned(V), nblk = (n + kIvbBlock - 1) / kIvbBlock;
            const size_t nb = std::min<size_t>(st.n_bricks, image.n_bricks_cap), ncell = nb * kBrickStride;
            const dim3 g{nblk, 1u, 1u}, t{unsigned(kIvbBlock), 1u, 1u};
            image.d_alive_rec.reserve(V);
            d_blob_rep.reserve(1); bl_lsrc.reserve(V); bl_bt.reserve(size_t(2) * nblk + 1);
            FLS_HIP(hipMemsetAsync(d_blob_rep.p, 0, sizeof(IvblReport), stream));
            FLS_HIP(hipMemsetAsync(image.d_alive_rec.p, 0, V * sizeof(IvoxAliveRec), stream));  // (a record the listing does not fill packs nothing: the totals below catch it)
            if (ncell)
                hipLaunchKernelGGL(ivox_list_alive_kernel, dim3(unsigned((ncell + 255) / 256)), dim3(256), 0, stream, (const uint2*)image.d_cells.p,
                                   (const unsigned long long*)image.d_brick_key.p, unsigned(ncell), (const unsigned char*)image.d_cap_log2.p,
                                   (const unsigned long long*)image.d_stamp.p, image.d_alive_rec.p, &d_blob_rep.p->n_listed, n);
            // oldest first: the 64-bit stamps in two stable rounds, low word first (as the eviction selection sorts them); every stamp <= stamp_base
            const IvoxAliveRec* const rec = image.d_alive_rec.p;
            bb_sort.prepare(V);
            hipLaunchKernelGGL(ivbx_stamp_keys, g, t, 0, stream, rec, n, bb_sort.k0, bb_sort.v0);
            bb_sort.run(DevicePairSort::passes_for(std::min<unsigned long long>(st.stamp_base, 0xffffffffull)), stream);
            if (st.stamp_base >> 32) {
                hipLaunchKernelGGL(ivbx_stamp_hi, g, t, 0, stream, rec, (const unsigned*)bb_sort.v0, n, bb_sort.k0);
                bb_sort.run(DevicePairSort::passes_for(st.stamp_base >> 32), stream);
            }
            const unsigned* const order = bb_sort.v0;
            hipLaunchKernelGGL(ivbx_counts, g, t, 0, stream, rec, order, n, bl_lsrc.p, bl_bt.p, d_blob_rep.p);
            hipLaunchKernelGGL(vg_scan, dim3(1), dim3(kVgScanBlock), 0, stream, (const unsigned*)bl_bt.p, bl_bt.p + nblk, int(nblk), (unsigned*)nullptr);
            hipLaunchKernelGGL(ivbx_pack, dim3(unsigned((V * kIvblLanes + kIvbBlock - 1) / kIvbBlock)), t, 0, stream, rec, order, n, (const unsigned*)bl_lsrc.p,
                               (const unsigned*)(bl_bt.p + nblk), (const float4*)image.d_pts.p, (unsigned long long)image.d_pts.cap,
                               reinterpret_cast<ulonglong2*>(base + sizeof(BlobHeader)), reinterpret_cast<float4*>(base + sizeof(BlobHeader) + V * 16), (unsigned long long)P);
            FLS_HIP(hipGetLastError());
            IvblReport rep{};
            FLS_HIP(hipMemcpyAsync(&rep, d_blob_rep.p, sizeof(rep), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            if (rep.n_listed != n || rep.count_sum != P) throw std::runtime_error("iVox image: the alive-voxel or point count of the device state does not match its cells");
        }
        FLS_HIP(hipMemcpyAsync(dst, base, need, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        ++n_blob_exports_device;
        return FLS_OK;
    }
    // Any state -> an ordinary map holding the blob's voxels: Device / ImageOnly without a mirror where the device builds it, else what import_blob
    // leaves.  An invalid blob leaves the map as it was.
    fls_status import_blob_from(const void* src, const size_t n, const bool src_on_device) {
        if (!src || n < sizeof(BlobHeader)) return FLS_ERR_INVALID;
        unsigned char head[sizeof(BlobHeader)];
        FLS_HIP(hipMemcpy(head, src, sizeof(head), src_on_device ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
        BlobHeader hd;
        const fls_status hrc = ivox_blob_check_header(head, n, kind, ivox.resolution, hd);
        if (hrc != FLS_OK) return hrc;
        BlobDecline why = BlobDecline::None;
        if (!allow_device_image) why = BlobDecline::SwitchedOff;
        else if (!use_dense) why = BlobDecline::NotDense;
        else if (hd.n_voxels == 0 || hd.n_voxels >= ivox.capacity || hd.n_voxels > kBlobSortMax || hd.n_points > kBlobSortMax) why = BlobDecline::Size;
        if (why == BlobDecline::None) {
            const fls_status rc = import_blob_device(src, n, src_on_device, hd, why);
            if (why == BlobDecline::None) return rc;
        }
        ++n_blob_imports_declined;
        ++n_blob_decline_reason[int(why)];
        if (!src_on_device) return import_blob(src, n);
        std::vector<char> host(n);
        FLS_HIP(hipMemcpy(host.data(), src, n, hipMemcpyDeviceToHost));
        return import_blob(host.data(), n);
    }
    // The closed form of "a blob into an EMPTY map"  on the device.  `why` set: declined, the host path answers (the map is as it
    // was, or empty where the brick pool went over its budget -- import_blob starts from an empty map anyway).
    fls_status import_blob_device(const void* src, const size_t n, const bool src_on_device, const BlobHeader& hd, BlobDecline& why) {
        const size_t V = size_t(hd.n_voxels), P = size_t(hd.n_points);
        const unsigned nv = unsigned(V), nblk = (nv + kIvbBlock - 1) / kIvbBlock;
        const dim3 g{nblk, 1u, 1u}, t{unsigned(kIvbBlock), 1u, 1u};
        FLS_HIP(hipStreamSynchronize(stream));  // (the staging buffer and the scratch are free)
        char* const base = blob_staging(n);
        FLS_HIP(hipMemcpyAsync(base, src, n, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
        const ulonglong2* const vox = reinterpret_cast<const ulonglong2*>(base + sizeof(BlobHeader));
        const float4* const rows = reinterpret_cast<const float4*>(base + sizeof(BlobHeader) + V * 16);
        // ---- checks: nothing of the map changes before they have all passed ----
        d_blob_rep.reserve(1); bl_lsrc.reserve(V); bl_bt.reserve(size_t(2) * nblk + 1);
        IvblReport rep{};
        for (int a = 0; a < 3; ++a) { rep.bmin[a] = INT_MAX; rep.bmax[a] = INT_MIN; }
        FLS_HIP(hipMemcpyAsync(d_blob_rep.p, &rep, sizeof(rep), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(ivbl_check, g, t, 0, stream, vox, nv, (unsigned long long)P, bl_lsrc.p, bl_bt.p, d_blob_rep.p);
        hipLaunchKernelGGL(vg_scan, dim3(1), dim3(kVgScanBlock), 0, stream, (const unsigned*)bl_bt.p, bl_bt.p + nblk, int(nblk), (unsigned*)nullptr);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipMemcpyAsync(&rep, d_blob_rep.p, sizeof(rep), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        if ((rep.flag & (kIvblZeroCount | kIvblBadCount)) || rep.count_sum != P) return FLS_ERR_INVALID;
        if (rep.flag & kIvblBadKey) { why = BlobDecline::Range; return FLS_OK; }
        const IvoxBrickExtent ext = ivox_brick_extent(rep.bmin, rep.bmax);
        const IvbExtent e{{ext.bmin[0], ext.bmin[1], ext.bmin[2]}, ext.bits[0], ext.bits[1]};
        const int key_bits = ext.key_bits();
        const bool wide = key_bits > 32;
        bb_sort.prepare(V);
        if (wide) bb_khi.reserve(V);
        bb_lcap.reserve(V); bb_vbegin.reserve(V); bb_btc.reserve(size_t(2) * nblk + 1);
        unsigned* const btcs = bb_btc.p + nblk;  // scanned capacities
        hipLaunchKernelGGL(ivbl_keys, g, t, 0, stream, vox, nv, e, bb_sort.k0, wide ? bb_khi.p : (unsigned*)nullptr, bb_sort.v0);
        bb_sort.run((std::min(key_bits, 32) + 7) / 8, stream);
        if (wide) {  // two stable rounds, low word first
            hipLaunchKernelGGL(ivb_gather_hi, g, t, 0, stream, (const unsigned*)bb_khi.p, (const unsigned*)bb_sort.v0, int(nv), bb_sort.k0);
            bb_sort.run((key_bits - 32 + 7) / 8, stream);
        }
        const unsigned* const order = bb_sort.v0;
        hipLaunchKernelGGL(ivbl_layout, g, t, 0, stream, vox, order, nv, bb_lcap.p, bb_btc.p, d_blob_rep.p);
        hipLaunchKernelGGL(vg_scan, dim3(1), dim3(kVgScanBlock), 0, stream, (const unsigned*)bb_btc.p, btcs, int(nblk), &d_blob_rep.p->used);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipMemcpyAsync(&rep, d_blob_rep.p, sizeof(rep), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        if (rep.flag & kIvblDuplicate) return FLS_ERR_INVALID;
        // ---- the build: bulk_build's pool and cells, the voxels and their stamps (blob position + 1) given ----
        const size_t used = rep.used;
        become_empty();
        BuiltPool pool;
        if (!build_brick_pool(rep.own_bricks, used, P, V, int(hd.next_id), /*stamp_base=*/V, pool, [&](const IvoxUpdArrays& a) {
                hipLaunchKernelGGL(ivbl_cells, g, t, 0, stream, vox, order, nv, (const unsigned*)bb_lcap.p, (const unsigned*)btcs, a, d_upd_state.p, bb_vbegin.p);
            })) {
            why = BlobDecline::Budget;
            return FLS_OK;
        }
        hipLaunchKernelGGL(ivbl_points, dim3(unsigned((V * kIvblLanes + kIvbBlock - 1) / kIvbBlock)), t, 0, stream, vox, rows, nv, (unsigned long long)P,
                           (const unsigned*)bl_lsrc.p, (const unsigned*)(bl_bt.p + nblk), (const unsigned*)bb_vbegin.p, image.d_pts.p, (unsigned long long)image.d_pts.cap);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipStreamSynchronize(stream));
        adopt_built_image(pool, used, P, V, /*stamp_base=*/V);
        is_first = hd.is_first != 0;
        ++n_blob_imports_device;
        return FLS_OK;
    }

    // ---- replica sets: `src`'s device image copied device to device (hipMemcpyPeer over xGMI between GPUs; no export blob, no host
    // mirror rebuild, no re-flatten -- SURVEY 8e's replicated read-only map).  Any state -> Replica.  Pre: `src` refreshed and its stream idle,
    // `used_now` / `n_bricks_now` its live_counts; this map's device current.  Both devices' streams are idle when this returns.
    void replicate(const IvoxMap& src, size_t used_now, size_t n_bricks_now, int src_device, int device) {
        FLS_HIP(hipStreamSynchronize(stream));
        become_empty();  // (a copy that fails half-way leaves an empty map that rebuilds its image)
        use_dense = src.use_dense;
        image.clone_for_reading(src.image, used_now, n_bricks_now, src_device, device, stream);
        is_first = src.is_first;
        become_replica();
    }

    // ---- the device image as one flat buffer, for replicas in OTHER processes (torch.distributed ranks): fls_map_image_bytes / _export / _import.
    // The exporter keeps its map; the importer becomes a read-only replica (fls_match / fls_match_batch with update_map == 0), like a
    // member of a replica set.  No host mirror, no re-flatten: 44 MB for the 1e6-point map, copied at memory speed on either side.
    // Pre (both): not a Replica, refreshed, the stream idle.
    IvoxImage::FlatHeader flat_header() {
        size_t nb = 0;
        const size_t used_now = live_counts(nb);
        IvoxImage::FlatHeader h = image.flat_header(used_now, nb);
        h.kind = kind; h.is_first = is_first ? 1u : 0u; h.use_dense = h.have_bricks; h.resolution = ivox.resolution;
        return h;
    }
    size_t image_bytes() { return size_t(flat_header().total_bytes); }
    fls_status export_image(void* dst, size_t cap, bool on_device) {
        const IvoxImage::FlatHeader h = flat_header();
        if (cap < size_t(h.total_bytes)) return FLS_ERR_RANGE;
        image.export_flat(h, dst, on_device, stream);
        return FLS_OK;
    }
    // Any state -> Replica; a buffer whose contents do not validate leaves an empty map (MirrorUnbuilt), a bad header the map as it was.
    fls_status import_image(const void* src, size_t n, bool on_device) {
        if (!src || n < sizeof(IvoxImage::FlatHeader)) return FLS_ERR_INVALID;
        IvoxImage::FlatHeader h;
        FLS_HIP(hipMemcpy(&h, src, sizeof(h), on_device ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
        if (!IvoxImage::flat_header_ok(h, n) || h.kind != kind) return FLS_ERR_INVALID;
        if (!(h.resolution > 0.f) || h.resolution != ivox.resolution) return FLS_ERR_INVALID;
        FLS_HIP(hipStreamSynchronize(stream));
        become_empty();  // (an import that fails half-way leaves an empty map that rebuilds its image)
        use_dense = h.have_bricks != 0;  // (derived, not trusted: the query takes the brick path exactly when the image carries bricks)
        image.import_flat(h, src, on_device, stream);
        // the contents are as untrusted as the header: no {begin, count} may leave the point array, no directory entry may name a missing brick
        d_counter_img.reserve(1);
        FLS_HIP(hipMemsetAsync(d_counter_img.p, 0, sizeof(unsigned), stream));
        const unsigned long long n_cells = image.have_bricks ? (unsigned long long)h.n_bricks_live * kBrickStride : 0ull;
        hipLaunchKernelGGL(ivox_image_validate_kernel, dim3(512), dim3(256), 0, stream, (const uint2*)image.d_cells.p, n_cells, (const HashEntry*)image.d_dir.p,
                           image.have_bricks ? (unsigned long long)h.dir_mask + 1ull : 0ull, unsigned(h.n_bricks_live), (const HashEntry*)image.d_table.p,
                           image.want_hash ? (unsigned long long)h.mask + 1ull : 0ull, (unsigned long long)h.used, d_counter_img.p);
        unsigned bad = 0;
        FLS_HIP(hipMemcpyAsync(&bad, d_counter_img.p, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        if (bad != 0u) return FLS_ERR_INVALID;
        is_first = h.is_first != 0;
        become_replica();
        return FLS_OK;
    }

    // fls_map_size: the map's slots (every other slot: the number of points)
    size_t counter(int slot) const {
        switch (slot) {
            case 100: return n_incremental;          // image updates applied as scatter lists
            case 101: return n_full_rebuilds + n_bulk_builds + n_blob_imports_device;  // full builds of the image: re-flatten + upload from the mirror, or built on the device (slots 140 and 170 say how many of them)
            case 102: return image_is_map() ? dev_n_alive : ivox.n_alive;  // occupied voxels (of a bulk-built map: without building the mirror)
            case 103: return n_device_updates;       // ... by the device-side AddPoints
            case 104: return n_host_fallbacks;       // batches the device refused (replayed on the host)
            case 117: return n_device_evictions;     // voxels evicted inside device batches
            case 119: return n_refused_conflict;     // refusals by reason: eviction order conflict / point array full / point outside the window
            case 120: return n_refused_full;
            case 121: return n_refused_outside;
            case 122: return 0;                      // (the former one-launch form: the slot keeps its number)
            case 123: return n_short_updates;        // device batches in the short chain (five launches behind the decision)
            case 124: return n_speculative;          // chains queued speculatively behind the iterations
            case 125: return n_speculative_skipped;  // ... that the device skipped (the Match needed more iterations / did not converge)
            case 126: return n_device_recreated;     // evicted voxels re-created by a later point of the same batch
            case 132: return image.budget_exceeded ? 1u : 0u;  // the brick pool went over FLS_IVOX_BRICK_BUDGET_MB: hash-table image, host AddPoints
            case 140: return n_bulk_builds;          // whole clouds built into the empty map on the device (bulk_build)
            case 141: return n_bulk_declined;        // ... declined to the host path (FLS_IVOX_DEVICE_BUILD=0 counts here and in no reason slot; an empty cloud nowhere)
            case 142: return n_bulk_decline_reason[int(BuildDecline::TooMany)];   // declines by reason: more points than the sort takes /
            case 143: return n_bulk_decline_reason[int(BuildDecline::Capacity)];  // as many voxels as the LRU capacity (evictions) /
            case 144: return n_bulk_decline_reason[int(BuildDecline::Range)];     // a point outside the key range or not finite (FLS_ERR_RANGE) /
            case 145: return n_bulk_decline_reason[int(BuildDecline::Budget)];    // a brick pool over its byte budget /
            case 146: return n_bulk_decline_reason[int(BuildDecline::NotDense)];  // the hash-table form (FLS_IVOX_DENSE=0, or the budget exceeded earlier)
            case 147: return n_lazy_mirrors;         // mirrors reconstructed from a bulk-built image (to_mirror)
            case 168: return n_blob_exports_device;  // include/fls_map_ivox.h: blobs packed on the device / written by the host writer
            case 169: return n_blob_exports_host;
            case 170: return n_blob_imports_device;  // blobs built into the image on the device / declined to import_blob (FLS_IVOX_DEVICE_IMAGE=0 counts here and in no reason slot)
            case 171: return n_blob_imports_declined;
            case 172: return n_blob_decline_reason[int(BlobDecline::Size)];      // declines by reason: empty, n_voxels >= capacity, more than the sort takes /
            case 173: return n_blob_decline_reason[int(BlobDecline::Range)];     // a key outside the key range or with reserved bits /
            case 174: return n_blob_decline_reason[int(BlobDecline::Budget)];    // a brick pool over its byte budget /
            case 175: return n_blob_decline_reason[int(BlobDecline::NotDense)];  // the hash-table form
            // (176 is the matcher's, not the map's: kNN waves of the last counting Match that took the shared-run path, TrafficCounters::shared)
            default: return image_is_map() ? dev_n_points : ivox.n_points;
        }
    }
};

}  // namespace fls
