// kd_map.hpp -- the local maps of the three kinds whose reference uses pcl::KdTreeFLANN (matchers_kd.hpp holds their Match):
//   DeviceCloudRing, KdMapDevice, KdLocalMap   one map: the reference's deque of clouds, its mirror on the device, the rebuild
//   KdMapImage                                  the maps of one handle as one flat image (include/fls_map_kd.h, kd_image.hpp)
//   kd_push_xform_f/_d, KdPushIntensity         what a keyframe pushed on the device needs besides the scan (kernels_kd_push.hpp)
//   KdMaps                                      the owner: one or two KdLocalMaps with their rebuild recipes, the keyframe gate, the image calls,
//                                               the counters.  A matcher holds one and says when; what happens to the maps is written here.
#pragma once
#include "device_voxelgrid.hpp"
#include "host_math.hpp"
#include "kernels_kd_push.hpp"
#include "kd_lazy_deque.hpp"
#include "kd_image.hpp"
#include "kernels_kd_image.hpp"

namespace fls {

// The local-map deque of the kd-tree kinds on the device (icp_optimized.h:173-184, loam_full_kdtree.h:70-91,
// loam_point_to_plane_kdtree.h:60-71): the clouds of the deque live back to back in four SoA planes, so "concatenate the deque"
// is a pointer + a length.  push_back appends (one host-to-device copy of the NEW cloud + a de-interleave kernel), pop_front
// advances the head; the planes are re-packed when the tail reaches the end.  Only used by the opt-in device map filter.
struct DeviceCloudRing {
    DevBuf<float> planes;  // x | y | z | i, `cap` floats each
    DevBuf<float4> rows;   // staging of the cloud being appended
    PinnedBuf<float4> h_rows;
    size_t cap = 0, head = 0, tail = 0;
    std::deque<size_t> sizes;
    const float* x() const { return planes.p + head; }
    const float* y() const { return planes.p + cap + head; }
    const float* z() const { return planes.p + 2 * cap + head; }
    const float* in() const { return planes.p + 3 * cap + head; }
    size_t size() const { return tail - head; }
    void clear() { head = tail = 0; sizes.clear(); }
    void pop_front() {
        if (sizes.empty()) return;
        head += sizes.front();
        sizes.pop_front();
        if (sizes.empty()) head = tail = 0;
    }
    void make_room(size_t extra, hipStream_t s) {
        if (tail + extra <= cap) return;
        const size_t live = tail - head;
        size_t ncap = cap;
        while (live + extra > ncap || ncap < 65536) ncap = ncap ? ncap * 2 : 65536;
        if (ncap == cap && head >= live) {  // re-pack in place: source and destination do not overlap
            for (int a = 0; a < 4 && live; ++a)
                FLS_HIP(hipMemcpyAsync(planes.p + size_t(a) * cap, planes.p + size_t(a) * cap + head, live * sizeof(float), hipMemcpyDeviceToDevice, s));
        } else {
            if (ncap == cap) ncap *= 2;
            DevBuf<float> np;
            np.reserve(4 * ncap);
            for (int a = 0; a < 4 && live; ++a)
                FLS_HIP(hipMemcpyAsync(np.p + size_t(a) * ncap, planes.p + size_t(a) * cap + head, live * sizeof(float), hipMemcpyDeviceToDevice, s));
            FLS_HIP(hipStreamSynchronize(s));  // the old planes are freed below
            std::swap(planes.p, np.p);  // (np now owns the old planes and frees them)
            std::swap(planes.cap, np.cap);
            cap = ncap;
        }
        head = 0;
        tail = live;
    }
    void push_back(const std::vector<PtI>& c, hipStream_t s) {
        const size_t n = c.size();
        make_room(n, s);
        if (n) {
            static_assert(sizeof(PtI) == sizeof(float4), "PtI rows are float4 rows");
            h_rows.reserve(n);
            rows.reserve(n);
            std::memcpy(h_rows.p, c.data(), n * sizeof(PtI));
            FLS_HIP(hipMemcpyAsync(rows.p, h_rows.p, n * sizeof(float4), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(soa_append, dim3(unsigned((n + kVgBlock - 1) / kVgBlock)), dim3(kVgBlock), 0, s, (const float4*)rows.p, int(n),
                               planes.p + tail, planes.p + cap + tail, planes.p + 2 * cap + tail, planes.p + 3 * cap + tail);
            FLS_HIP(hipGetLastError());
            FLS_HIP(hipStreamSynchronize(s));  // the pinned staging rows are reused by the next push
        }
        tail += n;
        sizes.push_back(n);
    }
    // The same append for clouds that already lie on this device (kernels_kd_push.hpp): n_rings (1 or 2) rings take one cloud each in ONE
    // launch on `s`, transformed on the way as `a.mode` says (the caller fills a.mode / a.R / a.t / a.T; the maps are filled here).  Nothing
    // waits for the launch: whatever reads the rings next is queued behind it on the same stream.  make_room runs unchanged.
    // false: a ring cannot take its cloud (its live points + the cloud would pass the 2^31 - 1 floats the 32-bit point counts of the
    // ring's kernels can address) -- nothing has changed, the caller pushes through the host.
    struct DeviceCloud { const float *x, *y, *z, *in; size_t n; };
    static constexpr size_t kMaxPoints = 0x7fffffffu;
    static bool push_back_device(DeviceCloudRing* const* rings, const DeviceCloud* src, const int n_rings, KdPushArgs a, hipStream_t s) {
        size_t total = 0;
        for (int r = 0; r < n_rings; ++r) {
            if (src[r].n > kMaxPoints || rings[r]->size() > kMaxPoints - src[r].n) return false;
            total += src[r].n;
        }
        if (total > kMaxPoints) return false;
        a.m[0] = a.m[1] = KdPushMap{};
        for (int r = 0; r < n_rings; ++r) {
            DeviceCloudRing& g = *rings[r];
            const size_t n = src[r].n;
            g.make_room(n, s);  // tail + n <= cap from here on: the launch below writes floats tail .. tail + n of every plane
            if (!n) continue;
            float* const at = g.planes.p + g.tail;
            a.m[r] = KdPushMap{src[r].x, src[r].y, src[r].z, reinterpret_cast<const unsigned*>(src[r].in), at, at + g.cap, at + 2 * g.cap,
                               reinterpret_cast<unsigned*>(at + 3 * g.cap), unsigned(n)};
        }
        if (total) {
            hipLaunchKernelGGL(kd_push_kernel, dim3(unsigned((total + kKdPushBlock - 1) / kKdPushBlock)), dim3(kKdPushBlock), 0, s, a);
            FLS_HIP(hipGetLastError());
        }
        for (int r = 0; r < n_rings; ++r) {
            rings[r]->tail += src[r].n;
            rings[r]->sizes.push_back(src[r].n);
        }
        return true;
    }
};

// Map maintenance of one kd-tree kind on the device: the cell-grid build and the deque + map-side pcl::VoxelGrid (bit-identical to
// the reference's since round 4: kernels_exactsort.hpp; FLS_DEVICE_VOXELGRID=0 = the host filter).  Whatever the device
// declines is redone by the host path, on the host deque (KdLocalMap::host_clouds fetches what a device push left in the ring alone).
struct KdMapDevice {
    bool grid_on_device = true;  // FLS_DEVICE_GRID_BUILD=0: host std::sort + bucket loop + upload (A/B)
    bool vg_on_device = true;    // FLS_DEVICE_VOXELGRID=0: the host filter
    DeviceGridBuilder builder;
    DeviceVoxelGrid vg;
    PinnedBuf<float> stage;
    DevBuf<float> xyz;
    bool push_on_device = true;  // FLS_KD_DEVICE_PUSH=0: a keyframe goes through the host (download, host transform, upload) as every other push
    unsigned long long device_filters = 0, host_filters = 0;
    void init() {
        if (const char* e = std::getenv("FLS_DEVICE_GRID_BUILD")) grid_on_device = std::atoi(e) != 0;
        vg_on_device = device_voxelgrid_mode() != 0;
        if (const char* e = std::getenv("FLS_KD_DEVICE_PUSH")) push_on_device = std::atoi(e) != 0;
        push_on_device = push_on_device && vg_on_device && grid_on_device;  // (no ring without the other two)
    }
    // grid over a HOST cloud (the exact host filter's output, or an unfiltered cloud)
    fls_status build_from_host(CellGridImage& grid, const std::vector<PtI>& cloud, float cell, hipStream_t s, int rings = 1) {
        const size_t n = cloud.size();
        if (grid_on_device && n != 0) {
            stage.reserve(3 * n);
            xyz.reserve(3 * n);
            for (size_t i = 0; i < n; ++i) { stage.p[i] = cloud[i].x; stage.p[n + i] = cloud[i].y; stage.p[2 * n + i] = cloud[i].z; }
            FLS_HIP(hipMemcpyAsync(xyz.p, stage.p, 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
            if (builder.run(grid, xyz.p, xyz.p + n, xyz.p + 2 * n, n, cell, rings, false, s)) return FLS_OK;  // (run() synchronises: the staging is free)
            FLS_HIP(hipStreamSynchronize(s));
        }
        return grid.build(cloud, cell, s, rings);
    }
    // local map = [VoxelGrid of] the concatenated deque, then the grid: all on the device.  false: declined, nothing changed.
    bool filter_and_build(CellGridImage& grid, const DeviceCloudRing& ring, bool filter, float leaf, float cell, int rings, size_t& n_map,
                          hipStream_t s) {
        if (!vg_on_device || !grid_on_device) return false;
        size_t n = ring.size();
        if (n == 0) return false;
        const float *x = ring.x(), *y = ring.y(), *z = ring.z();
        if (filter) {
            if (!vg.run(x, y, z, ring.in(), n, leaf, s)) return false;
            x = vg.ox(); y = vg.oy(); z = vg.oz();
            n = vg.n_out;
            if (n == 0) return false;
        }
        if (!builder.run(grid, x, y, z, n, cell, rings, false, s)) return false;
        n_map = n;
        ++device_filters;
        return true;
    }
};

// The local map of one kd-tree kind (LoamFull: of one feature class): the reference's deque of clouds (AddCloudToLocalMap: icp_optimized.h:165-189,
// loam_full_kdtree.h:65-104, loam_point_to_plane_kdtree.h:56-79) and what the Match searches, the cell grid over [the VoxelGrid of] the
// concatenated deque.  The owner pushes / trims as its reference does and calls rebuild() at the same moments; cell size and search depth are
// the owner's.  With `on_device` the deque is mirrored in a DeviceCloudRing and filter + grid build never leave the device.
//
// The host deque is LAZY (kd_lazy_deque.hpp): a keyframe pushed on the device (push_device) exists in the ring alone until something reads
// the host deque -- host_clouds(), the one accessor: a rebuild the device declined, an export through the host -- which first copies what is
// missing out of the ring.  Count and sizes (deque.size(), deque.sizes) are read without a download.
struct KdLocalMap {
    KdLazyDeque deque;        // the reference's deque; host copies of the clouds a host push or an import brought, or a fetch
    DeviceCloudRing ring;     // the deque's clouds back to back on the device (device path only)
    std::vector<PtI> local;   // the map cloud on the host: what the host path built, empty after a device rebuild
    CellGridImage grid;
    KdMapDevice dev;
    size_t n = 0;             // points of the local map, whichever path built it (fls_map_size)
    bool on_device = false;   // the deque is mirrored on the device: FLS_DEVICE_VOXELGRID != 0 and FLS_DEVICE_GRID_BUILD != 0
    bool rebuild_declined = false;  // the last rebuild(): the handle is on the device path and the device declined
    PinnedBuf<unsigned> fetch_stage;  // x | y | z | i of the run being fetched
    unsigned long long device_pushes = 0, host_pushes = 0, fetched = 0;
    void init() {
        dev.init();
        on_device = dev.vg_on_device && dev.grid_on_device;
    }
    void push(const std::vector<PtI>& cloud, hipStream_t s) {
        deque.push_host(cloud);
        if (on_device) { ring.push_back(cloud, s); ++host_pushes; }
    }
    bool can_push_device() const { return on_device && dev.push_on_device; }
    // A keyframe from clouds that lie on this device, one per map of `maps` (LoamFull: two), in one launch (DeviceCloudRing::push_back_device).
    // false: not on the device-push path, or a ring cannot take its cloud -- every map is as it was and the caller pushes through the host.
    static bool push_device(KdLocalMap* const* maps, const DeviceCloudRing::DeviceCloud* src, const int n_maps, const KdPushArgs& a, hipStream_t s) {
        DeviceCloudRing* rings[2] = {nullptr, nullptr};
        for (int m = 0; m < n_maps; ++m) {
            if (!maps[m]->can_push_device()) return false;
            rings[m] = &maps[m]->ring;
        }
        if (!DeviceCloudRing::push_back_device(rings, src, n_maps, a, s)) return false;
        for (int m = 0; m < n_maps; ++m) { maps[m]->deque.push_device(src[m].n); ++maps[m]->device_pushes; }
        return true;
    }
    void trim(size_t max_clouds) {  // (whether or not the cloud that leaves was ever fetched)
        if (deque.trim(max_clouds) && on_device) ring.pop_front();
    }
    void reset_to(const std::vector<PtI>& cloud, hipStream_t s) {  // localization mode: the map is the last cloud alone
        deque.clear();
        ring.clear();
        push(cloud, s);
    }
    // an import: the image's deque, every cloud present on the host (the caller has put the rows into the ring's planes)
    void replace_deque(KdDeque&& all) {
        deque.assign(std::move(all));
        if (!on_device) return;
        ring.sizes.clear();
        for (const size_t sz : deque.sizes) ring.sizes.push_back(sz);
    }
    // THE reader of the host deque: whatever the host does not hold is fetched from the ring first, run by run (four copies and one wait each)
    const KdDeque& host_clouds(hipStream_t s) {
        if (deque.complete()) return deque.clouds;
        for (const KdLazyDeque::Run& r : deque.missing_runs()) {
            if (r.n_points) {
                fetch_stage.reserve(4 * r.n_points);
                for (int a = 0; a < 4; ++a)
                    FLS_HIP(hipMemcpyAsync(fetch_stage.p + size_t(a) * r.n_points, ring.planes.p + size_t(a) * ring.cap + ring.head + r.offset, r.n_points * sizeof(float),
                                           hipMemcpyDeviceToHost, s));
                FLS_HIP(hipStreamSynchronize(s));
            }
            const unsigned* q = fetch_stage.p;
            deque.fill(r, q, q + r.n_points, q + 2 * r.n_points, q + 3 * r.n_points);
            fetched += r.n_clouds;
        }
        return deque.clouds;
    }
    // local map = [VoxelGrid(leaf) of] the concatenated deque, then the grid (cells of `cell`, searched `rings` deep): on the device, or on
    // the host for whatever the device declines
    fls_status rebuild(bool filter, float leaf, float cell, int rings, hipStream_t s) {
        rebuild_declined = false;
        if (on_device && dev.filter_and_build(grid, ring, filter, leaf, cell, rings, n, s)) { local.clear(); return FLS_OK; }
        rebuild_declined = on_device;
        local.clear();
        for (const auto& c : host_clouds(s)) local.insert(local.end(), c.begin(), c.end());
        if (filter) { local = voxel_grid(local, leaf); ++dev.host_filters; }
        n = local.size();
        return dev.build_from_host(grid, local, cell, s, rings);
    }
    // fls_map_size slots 114 / 115 / 116: cell grids built on the device / map updates filtered on the device / ... filtered on the host;
    // 164 / 165 / 166: clouds pushed on the device / pushed through the host while a ring exists / fetched to the host lazily
    size_t counter(int slot) const {
        return size_t(slot == 114 ? dev.builder.builds : slot == 115 ? dev.device_filters : slot == 116 ? dev.host_filters : slot == 164 ? device_pushes
                      : slot == 165 ? host_pushes : fetched);
    }
};

// ---------------------------------------------------------------------------------------------
// The local maps of one kd-tree handle as one flat image (include/fls_map_kd.h, kd_image.hpp): fls_map_export / _import, fls_map_image_*,
// replica sets.  The image carries the deque(s) and the keyframe gate; the bytes are a function of the logical state, so the rings of a
// device-path handle (packed by kd_image_pack_kernel) and the host deques of a host-path one give the same image.  An import checks the
// whole image on the host, unpacks the rows into planes of its own (kept for the next import: a replica refresh allocates nothing after
// the first), and only then swaps them into the handle and runs the kind's own rebuild.  An import fills the host deque EAGERLY (every cloud
// present, as after a host push; a keyframe pushed on the device has no host copy until something reads one, KdLocalMap::host_clouds): one
// device-to-host copy when the source is device memory.  An export from the rings reads sizes alone and fetches nothing.
// fls_map_size slots 160-163.
struct KdMapImage {
    unsigned long long exports_device = 0, exports_host = 0, imports_device = 0, imports_host = 0;
    DevBuf<unsigned char> img_stage;      // the image on the device, where the caller's buffer is not device memory the kernels can use directly
    PinnedBuf<unsigned char> img_pinned;  // header + sizes on their way up; the whole image on its way down
    struct SpareRing { DevBuf<float> planes; size_t cap = 0; } spare[2];  // what an import unpacks into / what it took the handle's planes for
    DevBuf<unsigned char> replica_out, replica_in;  // the image of a replication on the owner's device / on the replica's
    static bool kernel_aligned(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }
    size_t counter(int slot) const { return size_t(slot == 160 ? exports_device : slot == 161 ? exports_host : slot == 162 ? imports_device : imports_host); }

    // (layout, header and sizes need the clouds' sizes alone: no host copy is fetched for them)
    static bool layout_of(KdLocalMap* const* maps, const int n_maps, KdImageLayout& L) {
        const KdSizes* d[2] = {&maps[0]->deque.sizes, n_maps > 1 ? &maps[1]->deque.sizes : nullptr};
        return kd_image_layout_of(d, n_maps, L);
    }
    // the rings hold what the deques hold, in planes a 16-byte access may walk
    static bool rings_usable(KdLocalMap* const* maps, const KdImageLayout& L) {
        unsigned long long quads = 0;
        for (int m = 0; m < L.n_maps; ++m) {
            const DeviceCloudRing& r = maps[m]->ring;
            if (!maps[m]->on_device || r.size() != L.n_points[m] || r.sizes.size() != L.n_clouds[m]) return false;
            if (L.n_points[m] && ((r.cap & 3u) != 0 || !kernel_aligned(r.planes.p) || r.tail > r.cap)) return false;
            quads += (L.n_points[m] + 6) / 4;
        }
        return quads < 0x7fffffffull;
    }
    fls_status export_image(const KdImageParams& q, const KdImageGate& g, KdLocalMap* const* maps, void* dst, size_t cap, int dst_on_device, hipStream_t stream) {
        KdImageLayout L;
        if (!dst || !layout_of(maps, int(q.n_maps), L)) return FLS_ERR_STATE;
        if (cap < L.total) return FLS_ERR_RANGE;
        unsigned char* const out = static_cast<unsigned char*>(dst);
        const KdSizes* d[2] = {&maps[0]->deque.sizes, L.n_maps > 1 ? &maps[1]->deque.sizes : nullptr};
        FLS_HIP(hipStreamSynchronize(stream));
        if (!rings_usable(maps, L)) {  // from the host deques (fetched from the rings where a device push left them there alone)
            unsigned char* const host = dst_on_device ? (img_pinned.reserve(L.total), img_pinned.p) : out;
            const KdDeque* hd[2] = {&maps[0]->host_clouds(stream), L.n_maps > 1 ? &maps[1]->host_clouds(stream) : nullptr};
            kd_image_from_deques(q, g, L, hd, host);
            if (dst_on_device) {
                FLS_HIP(hipMemcpyAsync(out, host, L.total, hipMemcpyHostToDevice, stream));
                FLS_HIP(hipStreamSynchronize(stream));
            }
            ++exports_host;
            return FLS_OK;
        }
        const bool direct = dst_on_device && kernel_aligned(dst);
        unsigned char* img = out;
        if (!direct) { img_stage.reserve(L.total); img = img_stage.p; }
        // header and sizes, with the padding behind them, from the host; the rows from the rings: together every byte of the image
        const size_t meta0 = L.rows[0], meta1 = L.n_maps > 1 ? L.rows[1] - L.sizes[1] : 0;
        img_pinned.reserve(meta0 + meta1);
        unsigned char* const chunk[2] = {img_pinned.p, img_pinned.p + meta0};
        kd_image_write_meta(q, g, L, d, chunk);
        FLS_HIP(hipMemcpyAsync(img, chunk[0], meta0, hipMemcpyHostToDevice, stream));
        if (meta1) FLS_HIP(hipMemcpyAsync(img + L.sizes[1], chunk[1], meta1, hipMemcpyHostToDevice, stream));
        KdPackArgs a{};
        unsigned quads = 0;
        for (int m = 0; m < L.n_maps; ++m) {
            const DeviceCloudRing& r = maps[m]->ring;
            if (!L.n_points[m]) continue;
            const size_t base = r.head & ~size_t(3);
            const unsigned* pl = reinterpret_cast<const unsigned*>(r.planes.p);
            KdPackMap& k = a.m[m];
            k.x = pl + base; k.y = pl + r.cap + base; k.z = pl + 2 * r.cap + base; k.i = pl + 3 * r.cap + base;
            k.rows = reinterpret_cast<uint4*>(img + L.rows[m]);
            k.off = unsigned(r.head - base);
            k.n = unsigned(L.n_points[m]);
            k.quads = (k.off + k.n + 3u) / 4u;  // base + 4 * quads <= cap: cap is a multiple of 4 and tail <= cap
            quads += k.quads;
        }
        if (quads) hipLaunchKernelGGL(kd_image_pack_kernel, dim3((quads + kKdImageBlock - 1) / kKdImageBlock), dim3(kKdImageBlock), 0, stream, a);
        if (!direct) FLS_HIP(hipMemcpyAsync(out, img, L.total, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        FLS_HIP(hipGetLastError());
        ++exports_device;
        return FLS_OK;
    }
    // Everything of an import up to the kind's rebuild: FLS_OK = the deques, the rings and `gate` hold the image (`any_cloud`: it holds a
    // cloud at all); anything else = the handle is as it was.
    fls_status import_image(const KdImageParams& q, KdLocalMap* const* maps, const void* src, size_t n_bytes, int src_on_device, hipStream_t stream,
                            hm::KeyframeGate& gate, bool& any_cloud) {
        if (!src) return FLS_ERR_INVALID;
        // (1) the header
        unsigned char head[sizeof(fls_kd_image_header)];
        if (n_bytes < sizeof(head)) return FLS_ERR_INVALID;
        if (src_on_device) FLS_HIP(hipMemcpy(head, src, sizeof(head), hipMemcpyDeviceToHost));
        else std::memcpy(head, src, sizeof(head));
        fls_kd_image_header h;
        KdImageLayout L;
        const fls_status hrc = kd_image_check_header(head, n_bytes, q, h, L);
        if (hrc != FLS_OK) return hrc;
        // (2) the whole image in host memory: sizes and padding are checked there, and the host deques are filled from it
        const unsigned char* host = static_cast<const unsigned char*>(src);
        if (src_on_device) {
            img_pinned.reserve(L.total);
            FLS_HIP(hipMemcpyAsync(img_pinned.p, src, L.total, hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            host = img_pinned.p;
        }
        const fls_status brc = kd_image_check_body(host, L);
        if (brc != FLS_OK) return brc;
        // (3) the rows into planes of this importer's own
        const bool on_device = maps[0]->on_device;
        unsigned long long quads_all = 0;
        for (int m = 0; m < L.n_maps; ++m) quads_all += (L.n_points[m] + 3) / 4;
        if (on_device && quads_all >= 0x7fffffffull) return FLS_ERR_INVALID;  // (more points than a ring can hold)
        if (on_device && quads_all) {
            const unsigned char* img = static_cast<const unsigned char*>(src);
            if (!(src_on_device && kernel_aligned(src))) {
                img_stage.reserve(L.total);
                FLS_HIP(hipMemcpyAsync(img_stage.p, src, L.total, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
                img = img_stage.p;
            }
            KdUnpackArgs a{};
            unsigned quads = 0;
            for (int m = 0; m < L.n_maps; ++m) {
                const size_t n = L.n_points[m];
                if (!n) continue;
                SpareRing& sp = spare[m];
                if (sp.cap < n || !sp.planes.p) {  // as DeviceCloudRing::make_room sizes a ring: 65,536 floats per plane, doubled until it fits
                    size_t ncap = 65536;
                    while (ncap < n) ncap *= 2;
                    sp.planes.reserve(4 * ncap);
                    sp.cap = ncap;
                }
                unsigned* pl = reinterpret_cast<unsigned*>(sp.planes.p);
                KdUnpackMap& k = a.m[m];
                k.rows = reinterpret_cast<const uint4*>(img + L.rows[m]);
                k.x = pl; k.y = pl + sp.cap; k.z = pl + 2 * sp.cap; k.i = pl + 3 * sp.cap;
                k.n = unsigned(n);
                k.quads = unsigned((n + 3) / 4);  // 4 * quads <= cap: cap is a multiple of 4
                quads += k.quads;
            }
            hipLaunchKernelGGL(kd_image_unpack_kernel, dim3((quads + kKdImageBlock - 1) / kKdImageBlock), dim3(kKdImageBlock), 0, stream, a);
            FLS_HIP(hipStreamSynchronize(stream));
            FLS_HIP(hipGetLastError());
        }
        // (4) the handle takes the image
        FLS_HIP(hipDeviceSynchronize());  // launches of the batch lanes may still read the old grid
        any_cloud = false;
        for (int m = 0; m < L.n_maps; ++m) {
            KdLocalMap& km = *maps[m];
            KdDeque all;
            kd_deque_from_image(host, L, m, all);
            any_cloud = any_cloud || L.n_clouds[m] != 0;
            if (on_device) {
                DeviceCloudRing& r = km.ring;
                if (L.n_points[m]) {
                    std::swap(r.planes.p, spare[m].planes.p);
                    std::swap(r.planes.cap, spare[m].planes.cap);
                    std::swap(r.cap, spare[m].cap);
                }
                r.head = 0;
                r.tail = L.n_points[m];
            }
            km.replace_deque(std::move(all));  // (every cloud present on the host; the ring's sizes follow)
        }
        const KdImageGate g = kd_gate_from_header(h);
        gate = hm::KeyframeGate();
        gate.init = g.init;
        std::memcpy(gate.last_T, g.last_T, sizeof(gate.last_T));
        ++(on_device ? imports_device : imports_host);
        return FLS_OK;
    }
    // a handle without a cloud: what it was before its first one
    static void reset_map(KdLocalMap& km) { km.local.clear(); km.n = 0; }
};
inline KdImageGate kd_gate_of(const hm::KeyframeGate& gate) {
    KdImageGate g;
    g.init = gate.init;
    if (g.init) std::memcpy(g.last_T, gate.last_T, sizeof(g.last_T));
    return g;
}

// ---------------------------------------------------------------------------------------------
// A keyframe pushed on the device (KdLocalMap::push_device, kernels_kd_push.hpp): the transform as the kernel takes it, and the intensity
// plane of scans whose intensities never went to the device.
inline KdPushArgs kd_push_xform_f(const double* T) {  // hm::xform_cloud_f's casts
    KdPushArgs a{};
    a.mode = kKdPushXformF;
    for (int j = 0; j < 3; ++j) for (int i = 0; i < 3; ++i) a.R[i + j * 3] = float(T[i + j * 4]);
    for (int i = 0; i < 3; ++i) a.t[i] = float(T[12 + i]);
    return a;
}
inline KdPushArgs kd_push_xform_d(const double* T) {  // hm::xform_cloud_d
    KdPushArgs a{};
    a.mode = kKdPushXformD;
    std::memcpy(a.T, T, sizeof(a.T));
    return a;
}
// DevScan::upload sends x | y | z; the intensities a keyframe carries into the deque are gathered from the scans' host copies into pinned
// memory and copied up as one plane (cloud 0's, then cloud 1's) when a keyframe is taken, and only then: a Match without one pays nothing.
struct KdPushIntensity {
    PinnedBuf<float> h;
    DevBuf<float> d;
    hipEvent_t copied = nullptr;  // the last copy has read `h`
    ~KdPushIntensity() { if (copied) (void)hipEventDestroy(copied); }
    const float* upload(const std::vector<PtI>* const* clouds, const int n_clouds, hipStream_t s) {
        size_t total = 0;
        for (int c = 0; c < n_clouds; ++c) total += clouds[c]->size();
        if (!total) return nullptr;
        if (copied) FLS_HIP(hipEventSynchronize(copied));  // (long over: a rebuild has waited for the stream since)
        else FLS_HIP(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
        h.reserve(total);
        d.reserve(total);
        size_t at = 0;
        for (int c = 0; c < n_clouds; ++c)
            for (const PtI& q : *clouds[c]) std::memcpy(h.p + at++, &q.i, sizeof(float));
        FLS_HIP(hipMemcpyAsync(d.p, h.p, total * sizeof(float), hipMemcpyHostToDevice, s));
        FLS_HIP(hipEventRecord(copied, s));
        return d.p;
    }
};

// ---------------------------------------------------------------------------------------------
// The maps of one kd-tree handle and everything that happens to them: one KdLocalMap, or two for LoamFull (planar first, then corner), each
// with the recipe of its rebuild, fixed at init() from the parameters; the keyframe gate; the flat image; the counters.  Everything is
// queued on the one stream given to init().  The calls that can change whether a map stands take the handle's `have_map` (fls_matcher's, the
// only such flag) and set it as the kind's AddCloudToLocalMap would.
struct KdMaps {
    struct Recipe {
        bool filter_always;  // the VoxelGrid at every rebuild (Q13); false: only once the deque holds more than 5 clouds (loam_full_kdtree.h:92-100)
        float leaf, cell;    // VoxelGrid leaf; cell of the search grid
        int rings;           // cells searched around the query's
        size_t trim;         // clouds the deque keeps
    };
    KdLocalMap map[2];
    int n_maps = 1;
    Recipe recipe[2]{};
    bool localization = false;  // AddCloudToLocalMap keeps the last cloud alone (never LoamFull: its update has no localization switch)
    hm::KeyframeGate gate;
    KdMapImage image;
    KdImageParams params;
    KdPushIntensity push_i;
    unsigned long long push_declines = 0;  // keyframes after whose device push a device rebuild was declined (fls_map_size slot 167)
    hipStream_t stream = nullptr;
    int device = 0;
    struct Ptrs { KdLocalMap* m[2]; };
    Ptrs ptrs() { return Ptrs{{&map[0], n_maps > 1 ? &map[1] : nullptr}}; }

    void init(const fls_kind kind, const fls_params& p, const int device_id, hipStream_t s, std::initializer_list<Recipe> recipes) {
        stream = s; device = device_id;
        params = kd_image_params(kind, p);
        n_maps = int(recipes.size());
        std::copy(recipes.begin(), recipes.end(), recipe);
        localization = params.localization && n_maps == 1;
        for (int m = 0; m < n_maps; ++m) {
            map[m].init();
            map[m].on_device = map[0].on_device;  // one device-path decision per handle, the first map's (all read the same two switches)
        }
    }
    // every map in order; a failing rebuild before the last returns at once and leaves have_map alone, otherwise it follows the last one's status
    fls_status rebuild(bool& have_map) {
        fls_status rc = FLS_OK;
        for (int m = 0; m < n_maps; ++m) {
            const Recipe& r = recipe[m];
            rc = map[m].rebuild(r.filter_always || map[m].deque.size() > 5, r.leaf, r.cell, r.rings, stream);
            if (rc != FLS_OK && m + 1 < n_maps) return rc;
        }
        have_map = rc == FLS_OK;
        return rc;
    }
    // AddCloudToLocalMap, clouds[m] for map m: every cloud is pushed (last map first) before any deque is trimmed (first map first)
    fls_status add_host(const std::vector<PtI>* clouds, bool& have_map) {
        if (localization) map[0].reset_to(clouds[0], stream);
        else {
            for (int m = n_maps - 1; m >= 0; --m) map[m].push(clouds[m], stream);
            for (int m = 0; m < n_maps; ++m) map[m].trim(recipe[m].trim);
        }
        return rebuild(have_map);
    }
    bool can_push_device() const { return map[0].can_push_device() && (n_maps < 2 || map[1].can_push_device()); }
    // The device sources of a keyframe from scans resident as DevScans, scans[m] for map m.  Intensity: the fourth planes of attached scans
    // (an empty scan needs none); of uploaded ones the host copies', sent up first (one plane for all).  false: a host copy is missing
    bool scan_sources(const DevScan* const* scans, DeviceCloudRing::DeviceCloud* src) {
        bool all_dev = true, any_dev = false, all_host = true;
        for (int m = 0; m < n_maps; ++m) {
            const DevScan& sc = *scans[m];
            all_dev = all_dev && (sc.dev_intensity || sc.n == 0);
            any_dev = any_dev || sc.dev_intensity;
            all_host = all_host && sc.host.size() == sc.n;
        }
        const float* up = nullptr;
        if (!(all_dev && any_dev)) {
            if (!all_host) return false;
            const std::vector<PtI>* clouds[2] = {&scans[0]->host, n_maps > 1 ? &scans[1]->host : nullptr};
            up = push_i.upload(clouds, n_maps, stream);
        }
        for (int m = 0; m < n_maps; ++m) {
            const DevScan& sc = *scans[m];
            const float* in = all_dev && any_dev ? (sc.n ? sc.xyz.p + 3 * sc.n : nullptr) : up;
            src[m] = DeviceCloudRing::DeviceCloud{sc.x.p, sc.y.p, sc.z.p, in, sc.n};
            if (up) up += sc.n;
        }
        return true;
    }
    // A keyframe from clouds on this device, src[m] into map m's ring transformed as `a` says, then trim and rebuild as add_host does.
    // false: the maps cannot take a device push -- nothing has changed; true: `rc` is the rebuild's status
    bool push_keyframe_device(const DeviceCloudRing::DeviceCloud* src, const KdPushArgs& a, bool& have_map, fls_status& rc) {
        if (!KdLocalMap::push_device(ptrs().m, src, n_maps, a, stream)) return false;
        for (int m = 0; m < n_maps; ++m) { map[m].trim(recipe[m].trim); map[m].rebuild_declined = false; }  // (a rebuild that returns early leaves the later flags alone)
        rc = rebuild(have_map);
        bool declined = false;
        for (int m = 0; m < n_maps; ++m) declined = declined || map[m].rebuild_declined;
        if (declined) ++push_declines;
        return true;
    }
    // fls_map_size: 114-116 and 164-166 summed over the maps (LoamFull: two clouds per keyframe), 160-163 the image's, 167
    static bool counts(int slot) { return (slot >= 114 && slot <= 116) || (slot >= 160 && slot <= 167); }
    size_t counter(int slot) const {
        if (slot >= 160 && slot <= 163) return image.counter(slot);
        if (slot == 167) return size_t(push_declines);
        return map[0].counter(slot) + (n_maps > 1 ? map[1].counter(slot) : 0);
    }

    // ---- the maps as one flat image (include/fls_map_kd.h) ----
    size_t image_bytes() {
        KdImageLayout L;
        return KdMapImage::layout_of(ptrs().m, n_maps, L) ? L.total : 0;
    }
    fls_status image_export(void* dst, size_t cap, int on_device) { return image.export_image(params, kd_gate_of(gate), ptrs().m, dst, cap, on_device, stream); }
    size_t export_blob(void* blob, size_t cap) {
        const size_t need = image_bytes();
        if (need && blob && cap >= need && image_export(blob, cap, 0) != FLS_OK) return 0;
        return need;
    }
    // replaced(): the handle forgets what the Match before the import left.  An image without a cloud leaves a handle without a map
    template <class F>
    fls_status image_import(const void* src, size_t n_bytes, int on_device, bool& have_map, F&& replaced) {
        bool any_cloud = false;
        const fls_status rc = image.import_image(params, ptrs().m, src, n_bytes, on_device, stream, gate, any_cloud);
        if (rc != FLS_OK) return rc;
        replaced();
        if (!any_cloud) {
            for (int m = 0; m < n_maps; ++m) KdMapImage::reset_map(map[m]);
            have_map = false;
            return FLS_OK;
        }
        return rebuild(have_map);
    }
    // replica sets: the owner's image, exported on its device, copied device to device and imported on this handle's device.
    // prepare_owner(): the owner's prepare_batch (map current, stream idle)
    template <class P, class F>
    fls_status replicate_from(KdMaps& owner, P&& prepare_owner, bool& have_map, F&& replaced) {
        FLS_HIP(hipSetDevice(owner.device));
        const fls_status prc = prepare_owner();
        if (prc != FLS_OK) return prc;
        const size_t nbytes = owner.image_bytes();
        if (!nbytes) return FLS_ERR_STATE;
        DevBuf<unsigned char>& out = owner.image.replica_out;  // (kept by the owner: a refresh allocates nothing)
        out.reserve(nbytes);
        const fls_status erc = owner.image_export(out.p, nbytes, 1);
        if (erc != FLS_OK) return erc;
        FLS_HIP(hipSetDevice(device));
        if (owner.device == device) return image_import(out.p, nbytes, 1, have_map, replaced);
        image.replica_in.reserve(nbytes);
        FLS_HIP(hipMemcpyPeer(image.replica_in.p, device, out.p, owner.device, nbytes));
        return image_import(image.replica_in.p, nbytes, 1, have_map, replaced);
    }
};

}  // namespace fls
