// matchers_kd.hpp -- host side of the three kinds whose reference uses pcl::KdTreeFLANN:
//   IcpMatcher       <- IcpOptimized<double>            include/registration/icp_optimized.h
//   LoamFullMatcher  <- LoamFull<double>                include/registration/loam_full_kdtree.h
//   P2PlaneKdMatcher <- LoamPointToPlaneKdtree<double>  include/registration/loam_point_to_plane_kdtree.h
// Map bookkeeping follows the reference's AddCloudToLocalMap (deque of clouds, VoxelGrid, rebuild): one KdLocalMap
// (device_voxelgrid.hpp) per map, two for LoamFull; the kd-tree is replaced by an exact-kNN cell grid rebuilt at the same moments.
#pragma once
#include "matcher_base.hpp"
#include "host_math.hpp"
#include "device_voxelgrid.hpp"
#include "kernels_knn.hpp"
#include "kernels_grid_coop.hpp"
#include "fitness_host.hpp"
#include "kd_image.hpp"
#include "kernels_kd_image.hpp"

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
// what the three kinds share of the image calls (M: the matcher; it supplies image_maps(), rebuild_maps() and map_replaced())
template <class M>
struct KdImageCalls {
    static size_t bytes(M& s) {
        if (s.owner) return 0;
        KdImageLayout L;
        KdLocalMap* maps[2];
        s.image_maps(maps);
        return KdMapImage::layout_of(maps, int(kd_image_params(s.kind, s.p).n_maps), L) ? L.total : 0;
    }
    static fls_status export_to(M& s, void* dst, size_t cap, int on_device) {
        if (s.owner) return FLS_ERR_STATE;
        KdLocalMap* maps[2];
        s.image_maps(maps);
        return s.image.export_image(kd_image_params(s.kind, s.p), kd_gate_of(s.gate), maps, dst, cap, on_device, s.stream);
    }
    static size_t export_blob(M& s, void* blob, size_t cap) {
        const size_t need = bytes(s);
        if (need && blob && cap >= need && export_to(s, blob, cap, 0) != FLS_OK) return 0;
        return need;
    }
    static fls_status import_from(M& s, const void* src, size_t n_bytes, int on_device) {
        if (s.owner) return FLS_ERR_INVALID;  // a batch lane has no map of its own
        KdLocalMap* maps[2];
        s.image_maps(maps);
        bool any_cloud = false;
        const fls_status rc = s.image.import_image(kd_image_params(s.kind, s.p), maps, src, n_bytes, on_device, s.stream, s.gate, any_cloud);
        if (rc != FLS_OK) return rc;
        s.map_replaced();
        s.log_n = 0;
        s.log_stale = false;
        if (!any_cloud) {
            for (int m = 0; m < int(kd_image_params(s.kind, s.p).n_maps); ++m) KdMapImage::reset_map(*maps[m]);
            s.have_map = false;
            return FLS_OK;
        }
        return s.rebuild_maps();
    }
    // replica sets: the owner's image, exported on its device, copied device to device and imported on this handle's device
    static fls_status replicate(M& s, fls_matcher& o) {
        if (o.kind != s.kind || s.owner) return FLS_ERR_STATE;
        M& src = static_cast<M&>(o);
        FLS_HIP(hipSetDevice(src.device));
        const fls_status prc = src.prepare_batch();  // map current, stream idle
        if (prc != FLS_OK) return prc;
        const size_t nbytes = bytes(src);
        if (!nbytes) return FLS_ERR_STATE;
        DevBuf<unsigned char>& out = src.image.replica_out;  // (kept by the owner: a refresh allocates nothing)
        out.reserve(nbytes);
        const fls_status erc = export_to(src, out.p, nbytes, 1);
        if (erc != FLS_OK) return erc;
        FLS_HIP(hipSetDevice(s.device));
        if (src.device == s.device) return import_from(s, out.p, nbytes, 1);
        s.image.replica_in.reserve(nbytes);
        FLS_HIP(hipMemcpyPeer(s.image.replica_in.p, s.device, out.p, src.device, nbytes));
        return import_from(s, s.image.replica_in.p, nbytes, 1);
    }
};
// the overrides of fls_matcher every kd kind spells the same way
#define FLS_KD_IMAGE_OVERRIDES(M)                                                                                                              \
    KdMapImage image;                                                                                                                          \
    size_t map_image_bytes() override { return KdImageCalls<M>::bytes(*this); }                                                                \
    fls_status map_image_export(void* dst, size_t cap, int on_device) override { return KdImageCalls<M>::export_to(*this, dst, cap, on_device); } \
    fls_status map_image_import(const void* src, size_t n, int on_device) override { return KdImageCalls<M>::import_from(*this, src, n, on_device); } \
    size_t map_export(void* blob, size_t cap) override { return KdImageCalls<M>::export_blob(*this, blob, cap); }                              \
    fls_status map_import(const void* blob, size_t n) override { return KdImageCalls<M>::import_from(*this, blob, n, 0); }                     \
    bool can_replicate() const override { return !owner && have_map; }                                                                         \
    fls_status replicate_from(fls_matcher& o) override { return KdImageCalls<M>::replicate(*this, o); }

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
struct IcpMatcher final : fls_matcher {
    KdLocalMap map;
    std::vector<PtI> source;
    SourceFilter src_filter;
    DevBuf<unsigned> d_ticket;
    const IcpMatcher* owner = nullptr;  // batch lane: reads the owner's map grid
    DevScan scan;
    size_t raw_n = 0;
    hm::KeyframeGate gate;
    double final_T[16]{};
    bool have_final = false;
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
        map.init();
        init_tickets(d_ticket);
        return FLS_OK;
    }
    fls_status add_cloud_impl(const std::vector<PtI>& new_cloud) {  // :165-189
        if (p.is_localization_mode) map.reset_to(new_cloud, stream);
        else { map.push(new_cloud, stream); map.trim(p.local_map_size); }
        return rebuild_maps();
    }
    fls_status rebuild_maps() {  // (a keyframe update and an image import)
        // gate-sized cells here: the ICP scan starts far from the map (1-NN often beyond half the gate in the early
        // iterations), the two-stage search would run its second stage for most queries (measured 25 vs 13.5 us / launch)
        const fls_status rc = map.rebuild(true, p.map_cloud_filter_size, cell_for_gate(p.point_search_thres), 1, stream);  // Q13: always filtered
        have_map = rc == FLS_OK;
        return rc;
    }
    // ---- the map as one flat image (include/fls_map_kd.h) ----
    void image_maps(KdLocalMap** m) { m[0] = &map; m[1] = nullptr; }
    void map_replaced() { have_final = false; }  // fls_get_fitness_score answers FLS_ERR_STATE until the next Match
    FLS_KD_IMAGE_OVERRIDES(IcpMatcher)
    fls_status add_cloud(const float* c0, size_t n0, const float* c1, size_t n1, int stride) override {
        if (c1 != nullptr && n1 != 0) return FLS_ERR_INVALID;
        return add_cloud_impl(cloud_from(c0, n0, stride));
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
        if (!(owner ? owner->have_map : have_map)) return FLS_ERR_STATE;
        const size_t n = scan.n;
        stats = fls_stats{};
        stats.n_source = int(n);
        d_nn_id.reserve(std::max<size_t>(n, 1));
        d_eff.reserve(std::max<size_t>(n, 1));
        m.n = n;
        m.cg = cell_dev(owner ? owner->map.grid : map.grid);
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
        const bool has_converge = mb.converged != 0;  // Q10: false after max iterations
        stats.converged = has_converge ? 1 : 0;
        fls_status rc = has_converge ? FLS_OK : FLS_NOT_CONVERGED;
        // :153 `has_converge_ && IsNeedAddCloud(T) && !is_localization_mode_`: the gate (and its last_T) is evaluated before the mode
        // switch, as in the reference; update_map == 0 (this ABI's "registration only" switch) skips the whole statement,
        // so such a call leaves the keyframe gate alone
        if (update_map && !owner && has_converge && gate.need(final_T, p.dist_thre_add_cloud, p.rot_thre_add_cloud) && !p.is_localization_mode) {
            fls_status arc;
            if (push_keyframe_device()) {  // the mapping branch of add_cloud_impl, the push on the device
                map.trim(p.local_map_size);
                arc = rebuild_maps();
                if (map.rebuild_declined) ++push_declines;
            } else {
                src_filter.materialize(stream, source);
                arc = add_cloud_impl(hm::xform_cloud_f(source, final_T));
            }
            if (arc != FLS_OK) rc = arc; else stats.map_updated = 1;
        }
        if (out) *out = stats;
        return rc;
    }
    // the filtered scan the Match just used, still on the device (the source filter's output planes), into the ring at final_T; false: the
    // host filter ran, or the map cannot take a device push -- nothing has changed
    unsigned long long push_declines = 0;  // device rebuilds declined after a device push (fls_map_size slot 167)
    bool push_keyframe_device() {
        if (!src_filter.resident || !map.can_push_device()) return false;
        const DeviceVoxelGrid& vg = src_filter.vg;
        const DeviceCloudRing::DeviceCloud src{vg.ox(), vg.oy(), vg.oz(), vg.oi(), vg.n_out};
        KdLocalMap* maps[1] = {&map};
        return KdLocalMap::push_device(maps, &src, 1, kd_push_xform_f(final_T), stream);
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
    void reset_job_state() override { gate = hm::KeyframeGate(); have_final = false; }  // function-static last_T of a fresh process (Q12)
    std::unique_ptr<fls_matcher> clone_for_lane() override { return make_owned_lane(*this); }
    fls_status fitness(float max_range, float* score) override {
        if (owner || !have_map || !have_final) return FLS_ERR_STATE;
        return fitness_score_device(*this, map.grid, scan, final_T, max_range, score);
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
        if ((slot >= 114 && slot <= 116) || (slot >= 164 && slot <= 166)) return map.counter(slot);
        if (slot >= 160 && slot <= 163) return image.counter(slot);
        if (slot == 167) return size_t(push_declines);
        return map.n;
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

struct LoamFullMatcher final : fls_matcher {
    KdLocalMap map_planar, map_corner;
    const LoamFullMatcher* owner = nullptr;  // batch lane: reads the owner's two map grids
    FeatureDev corner, planar;
    hm::KeyframeGate gate;
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
        map_planar.init();
        map_corner.init();
        map_corner.on_device = map_planar.on_device;  // one device-path decision per matcher, the planar map's (both read the same two switches)
        return FLS_OK;
    }
    fls_status add_cloud_impl(const std::vector<PtI>& planar_cloud, const std::vector<PtI>& corner_cloud) {  // :65-104
        map_corner.push(corner_cloud, stream);  // both classes are pushed before either deque is trimmed
        map_planar.push(planar_cloud, stream);
        map_planar.trim(p.local_planar_size);
        map_corner.trim(p.local_corner_size);
        return rebuild_maps();
    }
    fls_status rebuild_maps() {  // (a keyframe update and an image import)
        // half-gate cells + the two-stage kernel; the VoxelGrid only once the deque holds more than 5 frames (:92-100)
        const float cs = 0.5f * cell_for_gate(p.point_search_thres);
        fls_status rc = map_planar.rebuild(map_planar.deque.size() > 5, p.planar_voxel_filter_size, cs, kGridRings, stream);
        if (rc != FLS_OK) return rc;
        rc = map_corner.rebuild(map_corner.deque.size() > 5, p.corner_voxel_filter_size, cs, kGridRings, stream);
        have_map = rc == FLS_OK;  // (the corner rebuild's status alone)
        return rc;
    }
    // ---- the maps as one flat image (include/fls_map_kd.h): planar first, then corner ----
    void image_maps(KdLocalMap** m) { m[0] = &map_planar; m[1] = &map_corner; }
    void map_replaced() {}
    FLS_KD_IMAGE_OVERRIDES(LoamFullMatcher)
    fls_status add_cloud(const float* c0, size_t n0, const float* c1, size_t n1, int stride) override {
        if (c1 == nullptr && n1 != 0) return FLS_ERR_INVALID;  // CHECK_EQ(cloud_list.size(), 2) :66
        return add_cloud_impl(cloud_from(c0, n0, stride), c1 ? cloud_from(c1, n1, stride) : std::vector<PtI>());
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
        if (!(owner ? owner->have_map : have_map)) return FLS_ERR_STATE;
        const size_t np = planar.scan.n, nc = corner.scan.n;
        const int nbp = int((np + 255) / 256), nbc = int((nc + 255) / 256);
        stats = fls_stats{};
        stats.n_source = int(np);
        stats.n_source_corner = int(nc);
        planar.prepare();
        corner.prepare();
        d_partials_a.reserve(size_t(std::max(nbc, 1)) * kPartialStride);
        d_partials_b.reserve(size_t(std::max(nbp, 1)) * kPartialStride);
        const CellGridDev cgp = cell_dev(owner ? owner->map_planar.grid : map_planar.grid), cgc = cell_dev(owner ? owner->map_corner.grid : map_corner.grid);
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
        bool has_converge = true;
        if (mb.n_valid < 50) has_converge = false;  // number_valid_planar_ < 50 :181
        stats.n_valid_corner = mb.n_valid2;
        stats.sum_res_corner = mb.sum_res2;
        stats.converged = has_converge ? 1 : 0;
        fls_status rc = has_converge ? FLS_OK : FLS_NOT_CONVERGED;
        if (update_map && !owner && has_converge && gate.need(mb.T, p.dist_thre_add_cloud, p.rot_thre_add_cloud)) {  // :185-193 (no localization switch)
            fls_status arc;
            if (push_keyframe_device(mb.T)) {  // add_cloud_impl, both pushes in one launch on the device
                map_planar.trim(p.local_planar_size);
                map_corner.trim(p.local_corner_size);
                map_planar.rebuild_declined = map_corner.rebuild_declined = false;
                arc = rebuild_maps();
                if (map_planar.rebuild_declined || map_corner.rebuild_declined) ++push_declines;
            } else {
                planar.scan.fetch_host(stream);  // (attached scans are fetched only here)
                corner.scan.fetch_host(stream);
                arc = add_cloud_impl(hm::xform_cloud_d(planar.scan.host, mb.T), hm::xform_cloud_d(corner.scan.host, mb.T));
            }
            if (arc != FLS_OK) rc = arc; else stats.map_updated = 1;
        }
        if (out) *out = stats;
        return rc;
    }
    // both feature scans, still on the device, into their rings at the pose the Match found.  Intensity: the fourth planes of attached
    // scans (an empty scan needs none); of uploaded ones the host copies', sent up first (one plane for both).  false: the maps cannot
    // take a device push -- nothing has changed
    KdPushIntensity push_i;
    unsigned long long push_declines = 0;  // keyframes after whose device push a device rebuild was declined (fls_map_size slot 167)
    bool push_keyframe_device(const double* T) {
        if (!map_planar.can_push_device() || !map_corner.can_push_device()) return false;
        const DevScan &ps = planar.scan, &cs = corner.scan;
        const float *in_p = nullptr, *in_c = nullptr;
        if ((ps.dev_intensity || ps.n == 0) && (cs.dev_intensity || cs.n == 0) && (ps.dev_intensity || cs.dev_intensity)) {
            if (ps.n) in_p = ps.xyz.p + 3 * ps.n;
            if (cs.n) in_c = cs.xyz.p + 3 * cs.n;
        } else {
            if (ps.host.size() != ps.n || cs.host.size() != cs.n) return false;
            const std::vector<PtI>* clouds[2] = {&ps.host, &cs.host};
            in_p = push_i.upload(clouds, 2, stream);
            in_c = in_p ? in_p + ps.n : nullptr;
        }
        const DeviceCloudRing::DeviceCloud src[2] = {{ps.x.p, ps.y.p, ps.z.p, in_p, ps.n}, {cs.x.p, cs.y.p, cs.z.p, in_c, cs.n}};
        KdLocalMap* maps[2] = {&map_planar, &map_corner};
        return KdLocalMap::push_device(maps, src, 2, kd_push_xform_d(T), stream);
    }
    void reset_job_state() override { gate = hm::KeyframeGate(); }  // function-static last_T of a fresh process (Q12)
    std::unique_ptr<fls_matcher> clone_for_lane() override { return make_owned_lane(*this); }
    fls_status fitness(float, float* score) override { *score = std::numeric_limits<float>::max(); return FLS_OK; }  // FloatNaN :206-208
    int correspondences(int slot, int32_t* ids, uint8_t* cnt, uint8_t* valid, size_t cap) override {
        return (slot == 1 ? corner : planar).fetch(stream, ids, cnt, valid, cap);
    }
    size_t map_size(int slot) const override {
        if ((slot >= 114 && slot <= 116) || (slot >= 164 && slot <= 166)) return map_planar.counter(slot) + map_corner.counter(slot);  // (clouds: two per keyframe)
        if (slot >= 160 && slot <= 163) return image.counter(slot);
        if (slot == 167) return size_t(push_declines);
        return slot == 1 ? map_corner.n : map_planar.n;
    }
};

// ---------------------------------------------------------------------------------------------
struct P2PlaneKdMatcher final : fls_matcher {
    KdLocalMap map;
    const P2PlaneKdMatcher* owner = nullptr;  // batch lane: reads the owner's map grid
    FeatureDev planar;
    hm::KeyframeGate gate;
    double final_T[16]{};
    bool have_final = false;

    fls_status init() {
        if (unset_d(p.point_to_planar_thres) || unset_d(p.position_converge_thres) || unset_d(p.rotation_converge_thres) ||
            unset_d(p.rot_thre_add_cloud) || unset_d(p.dist_thre_add_cloud) || unset_f(p.map_cloud_filter_size))
            return FLS_ERR_INVALID;  // CHECK_NE block loam_point_to_plane_kdtree.h:43-50
        if (!(p.map_cloud_filter_size > 0.f)) return FLS_ERR_INVALID;
        init_common();
        map.init();
        return FLS_OK;
    }
    fls_status add_cloud_impl(const std::vector<PtI>& planar_cloud) {  // :56-79
        if (p.is_localization_mode) map.reset_to(planar_cloud, stream);
        else { map.push(planar_cloud, stream); map.trim(p.local_map_size); }
        return rebuild_maps();
    }
    fls_status rebuild_maps() {  // (a keyframe update and an image import)
        // un-gated 5-NN: ring search with a cell of two map leaves (>= 1 point per leaf after VoxelGrid)
        const fls_status rc = map.rebuild(true, p.map_cloud_filter_size, std::max(2.0f * p.map_cloud_filter_size, 0.5f), 1, stream);
        have_map = rc == FLS_OK;
        return rc;
    }
    // ---- the map as one flat image (include/fls_map_kd.h) ----
    void image_maps(KdLocalMap** m) { m[0] = &map; m[1] = nullptr; }
    void map_replaced() { have_final = false; }
    FLS_KD_IMAGE_OVERRIDES(P2PlaneKdMatcher)
    fls_status add_cloud(const float* c0, size_t n0, const float* c1, size_t n1, int stride) override {
        if (c1 != nullptr && n1 != 0) return FLS_ERR_INVALID;
        return add_cloud_impl(cloud_from(c0, n0, stride));
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
        if (!(owner ? owner->have_map : have_map)) return FLS_ERR_STATE;
        const size_t n = planar.scan.n;
        const int nblk = int((n + 255) / 256);
        stats = fls_stats{};
        stats.n_source = int(n);
        planar.prepare();
        d_partials_b.reserve(size_t(std::max(nblk, 1)) * kPartialStride);
        const CellGridDev cg = cell_dev(owner ? owner->map.grid : map.grid);
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
        bool has_converge = true;
        if (mb.n_valid < 50) has_converge = false;
        stats.converged = has_converge ? 1 : 0;
        fls_status rc = has_converge ? FLS_OK : FLS_NOT_CONVERGED;
        if (update_map && !owner && has_converge && gate.need(final_T, p.dist_thre_add_cloud, p.rot_thre_add_cloud) && !p.is_localization_mode) {  // :145-149
            fls_status arc;
            if (push_keyframe_device()) {  // the mapping branch of add_cloud_impl, the push on the device
                map.trim(p.local_map_size);
                arc = rebuild_maps();
                if (map.rebuild_declined) ++push_declines;
            } else {
                planar.scan.fetch_host(stream);  // (an attached scan is fetched only here)
                arc = add_cloud_impl(hm::xform_cloud_f(planar.scan.host, final_T));
            }
            if (arc != FLS_OK) rc = arc; else stats.map_updated = 1;
        }
        if (out) *out = stats;
        return rc;
    }
    // the scan, still on the device, into the ring at final_T.  Intensity: the fourth plane of an attached scan; of an uploaded one the
    // host copy's, sent up here.  false: the map cannot take a device push -- nothing has changed
    KdPushIntensity push_i;
    unsigned long long push_declines = 0;  // device rebuilds declined after a device push (fls_map_size slot 167)
    bool push_keyframe_device() {
        if (!map.can_push_device()) return false;
        const DevScan& sc = planar.scan;
        const float* in = nullptr;
        if (sc.dev_intensity) in = sc.xyz.p + 3 * sc.n;
        else if (sc.host.size() == sc.n) { const std::vector<PtI>* clouds[1] = {&sc.host}; in = push_i.upload(clouds, 1, stream); }
        else return false;
        const DeviceCloudRing::DeviceCloud src{sc.x.p, sc.y.p, sc.z.p, in, sc.n};
        KdLocalMap* maps[1] = {&map};
        return KdLocalMap::push_device(maps, &src, 1, kd_push_xform_f(final_T), stream);
    }
    void reset_job_state() override { gate = hm::KeyframeGate(); have_final = false; }
    std::unique_ptr<fls_matcher> clone_for_lane() override { return make_owned_lane(*this); }
    fls_status fitness(float max_range, float* score) override {
        if (owner || !have_map || !have_final) return FLS_ERR_STATE;
        return fitness_score_device(*this, map.grid, planar.scan, final_T, max_range, score);
    }
    int correspondences(int, int32_t* ids, uint8_t* cnt, uint8_t* valid, size_t cap) override { return planar.fetch(stream, ids, cnt, valid, cap); }
    size_t map_size(int slot) const override {
        if ((slot >= 114 && slot <= 116) || (slot >= 164 && slot <= 166)) return map.counter(slot);
        if (slot >= 160 && slot <= 163) return image.counter(slot);
        if (slot == 167) return size_t(push_declines);
        return map.n;
    }
};

}  // namespace fls
