// keyframes.hpp -- host side of the device keyframe store (include/fls_keyframes.h): the keyframes' ordered clouds resident as
// x | y | z | intensity planes (the layout DeviceVoxelGrid::run reads and writes, so a cached filtered cloud is its output copied out
// unchanged), up to kKfCacheSlots filtered forms per keyframe, and the sub-map assembly (kernels_keyframes.hpp): the segment table is
// built here and uploaded with the launch.
//
// A keyframe's cloud never changes, so VoxelGridCloud(keyframe, leaf) is computed once and reused by every later sub-map; what the
// device filter declines goes through the exact host filter (host_maps.hpp) and is uploaded, so that a cached cloud is always what
// fls_voxel_grid_cloud returns.  The store keeps no poses.  Every call ends with the stream drained: nothing a call queued reads a
// buffer a later call frees or overwrites.
#pragma once
#include "kernels_keyframes.hpp"
#include "kernels_handoff.hpp"
#include "device_voxelgrid.hpp"
#include "preprocess_host.hpp"
#include <memory>
#include <new>

namespace fls {

constexpr size_t kKfCacheSlots = 4;  // 0.2 (GetSubMap), 0.3 (SaveMap, the global-map publisher) and a visualisation leaf fit
constexpr size_t kKfMaxTotal = 4000000000u;  // merged points of one call: 32-bit output indices with room for a tile

// the four planes of one cloud, allocated to size (the store holds thousands of them for hours: no growth slack)
struct KfCloud {
    float* p = nullptr;
    size_t n = 0;
    explicit KfCloud(size_t count) : n(count) {
        if (n == 0) return;
        const hipError_t e = hipMalloc((void**)&p, bytes());
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); throw std::bad_alloc(); }
        FLS_HIP(e);
    }
    ~KfCloud() { if (p) (void)hipFree(p); }
    KfCloud(const KfCloud&) = delete;
    KfCloud& operator=(const KfCloud&) = delete;
    size_t bytes() const { return 4 * n * sizeof(float); }
    const float* plane(int a) const { return p + size_t(a) * n; }
};

struct Keyframe {
    KfCloud cloud;
    struct Cached { float leaf; std::unique_ptr<KfCloud> cloud; };
    std::vector<Cached> cache;  // oldest first
    explicit Keyframe(size_t n) : cloud(n) {}
};

}  // namespace fls

struct fls_keyframes {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;  // around the last merge launch
    bool timed = false;
    std::vector<std::unique_ptr<fls::Keyframe>> kf;
    fls::DeviceVoxelGrid vg;
    fls::DevScan up;                  // pinned staging of a cloud on its way to the device
    fls::DevBuf<float4> d_rows;       // merge output for the caller (no final filter)
    fls::DevBuf<float> d_planes;      // merge output for the final filter
    fls::DevBuf<unsigned char> d_table;
    fls::PinnedBuf<unsigned char> h_table;
    // fls_keyframes_loop_match_device: the two sub-maps as planes, each with a segment table of its own (the second merge is queued while
    // the first one's table is still on its way), and the event the matcher's stream waits for
    fls::DevBuf<float> d_sub[2];
    fls::DevBuf<unsigned char> d_sub_table[2];
    fls::PinnedBuf<unsigned char> h_sub_table[2];
    hipEvent_t ev_sub = nullptr;
    std::vector<float> tmp;
    size_t n_points = 0, n_cached = 0, n_filters = 0, n_hits = 0, n_declined = 0, n_merges = 0, n_bytes = 0;

    ~fls_keyframes() {
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        if (ev_t0) (void)hipEventDestroy(ev_t0);
        if (ev_t1) (void)hipEventDestroy(ev_t1);
        if (ev_sub) (void)hipEventDestroy(ev_sub);
    }

    void init() {
        FLS_HIP(hipSetDevice(device));
        FLS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        FLS_HIP(hipEventCreate(&ev_t0));
        FLS_HIP(hipEventCreate(&ev_t1));
        FLS_HIP(hipEventCreateWithFlags(&ev_sub, hipEventDisableTiming));
    }

    bool valid_id(int32_t id) const { return id >= 0 && size_t(id) < kf.size(); }

    size_t stat(int slot) {
        switch (slot) {
            case 0: return n_points;
            case 1: return n_cached;
            case 2: return n_filters;
            case 3: return n_hits;
            case 4: return n_declined;
            case 5: return n_merges;
            case 6: return n_bytes;
            case 7: {
                float ms = 0.f;
                if (!timed || hipEventElapsedTime(&ms, ev_t0, ev_t1) != hipSuccess) return 0;
                return size_t(double(ms) * 1.0e6);
            }
            default: return 0;
        }
    }

    // ---- storing -------------------------------------------------------------------------------------------------------------------
    // rows of `stride` floats on the host -> the planes of `c` (one copy; the staging is free again on return)
    void fill(fls::KfCloud& c, const float* pts, int stride) {
        if (c.n == 0) return;
        up.stage_raw(pts, c.n, stride);
        FLS_HIP(hipMemcpyAsync(c.p, up.stage.p, c.bytes(), hipMemcpyHostToDevice, stream));
        FLS_HIP(hipStreamSynchronize(stream));
    }
    int32_t push(std::unique_ptr<fls::Keyframe> k) {
        const size_t n = k->cloud.n, b = k->cloud.bytes();
        kf.push_back(std::move(k));
        n_points += n;
        n_bytes += b;
        return int32_t(kf.size() - 1);
    }
    fls_status add(const float* pts, size_t n, int stride, int32_t* id) {
        if (kf.size() >= size_t(INT32_MAX)) return FLS_ERR_INVALID;
        std::unique_ptr<fls::Keyframe> k(new fls::Keyframe(n));
        fill(k->cloud, pts, stride);
        *id = push(std::move(k));
        return FLS_OK;
    }
    // the same from a cloud of `pre`'s last scan, device to device: the copy waits for the scan, `pre`'s next scan for the copy
    fls_status add_preprocessed(fls_preprocess& pre, int what, int32_t* id) {
        fls::HandoffCloud c;
        const std::vector<fls::PtI>* rows = nullptr;
        if (!pre.device_cloud(what, c, rows))  // the cloud the exact host filter made
            return add(rows->empty() ? nullptr : &(*rows)[0].x, rows->size(), 4, id);
        if (kf.size() >= size_t(INT32_MAX)) return FLS_ERR_INVALID;
        std::unique_ptr<fls::Keyframe> k(new fls::Keyframe(c.n));
        if (c.n) {
            FLS_HIP(hipEventRecord(pre.ev_ready, pre.stream));
            FLS_HIP(hipStreamWaitEvent(stream, pre.ev_ready, 0));
            fls::handoff_launch(c, k->cloud.p, stream);
            FLS_HIP(hipGetLastError());
            FLS_HIP(hipEventRecord(pre.next_consumed_event(), stream));
            FLS_HIP(hipStreamSynchronize(stream));
        }
        *id = push(std::move(k));
        return FLS_OK;
    }

    // ---- reading -------------------------------------------------------------------------------------------------------------------
    // n points of four device planes (row stride `stride`) -> xyzi rows on the host
    void download(const float* planes, size_t stride, size_t n, float* out) {
        if (n == 0) return;
        tmp.resize(4 * n);
        for (int a = 0; a < 4; ++a)
            FLS_HIP(hipMemcpyAsync(tmp.data() + size_t(a) * n, planes + size_t(a) * stride, n * sizeof(float), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        for (size_t i = 0; i < n; ++i) { out[4 * i] = tmp[i]; out[4 * i + 1] = tmp[n + i]; out[4 * i + 2] = tmp[2 * n + i]; out[4 * i + 3] = tmp[3 * n + i]; }
    }
    // VoxelGridCloud(planes, leaf) where the device filter declined: the exact host filter, rows on the host
    std::vector<fls::PtI> host_filter(const float* planes, size_t n, float leaf) {
        std::vector<float> rows(4 * n);
        download(planes, n, n, rows.data());
        ++n_declined;
        return fls::voxel_grid_strided(rows.data(), n, 4, leaf);
    }

    // VoxelGridCloud(keyframe id, leaf), from the cache or computed now
    const fls::KfCloud& filtered(int32_t id, float leaf) {
        fls::Keyframe& k = *kf[size_t(id)];
        for (const auto& c : k.cache)
            if (c.leaf == leaf) { ++n_hits; return *c.cloud; }
        const fls::KfCloud& src = k.cloud;
        std::unique_ptr<fls::KfCloud> f;
        if (vg.run(src.plane(0), src.plane(1), src.plane(2), src.plane(3), src.n, leaf, stream)) {
            f.reset(new fls::KfCloud(vg.n_out));
            for (int a = 0; a < 4 && vg.n_out; ++a)
                FLS_HIP(hipMemcpyAsync(f->p + size_t(a) * vg.n_out, vg.out.p + size_t(a) * vg.n_in, vg.n_out * sizeof(float), hipMemcpyDeviceToDevice, stream));
            FLS_HIP(hipStreamSynchronize(stream));  // (the filter's output planes are the next run's)
        } else {
            const std::vector<fls::PtI> c = host_filter(src.p, src.n, leaf);
            f.reset(new fls::KfCloud(c.size()));
            fill(*f, c.empty() ? nullptr : &c[0].x, 4);
        }
        ++n_filters;
        if (k.cache.size() == fls::kKfCacheSlots) {  // the oldest goes (nothing is in flight: every call drains the stream)
            n_bytes -= k.cache.front().cloud->bytes();
            k.cache.erase(k.cache.begin());
            --n_cached;
        }
        n_bytes += f->bytes();
        ++n_cached;
        k.cache.push_back(fls::Keyframe::Cached{leaf, std::move(f)});
        return *k.cache.back().cloud;
    }

    fls_status get(int32_t id, float leaf, float* out, size_t cap, size_t* n_out) {
        const fls::KfCloud& c = leaf > 0.f ? filtered(id, leaf) : kf[size_t(id)]->cloud;
        *n_out = c.n;
        if (c.n > cap) return FLS_ERR_INVALID;
        download(c.p, c.n, c.n, out);
        return FLS_OK;
    }

    // ---- the sub-map ---------------------------------------------------------------------------------------------------------------
    // out / cap, or `grow`: a vector that takes whatever size the result has (fls_keyframes_loop_match), or sub = 0 / 1: the merged cloud
    // stays on the device as x | y | z | intensity planes of *n_out floats each in d_sub[sub] -- queued, not waited for, no final filter
    fls_status merge(const int32_t* ids, const double* poses, size_t n_ids, float leaf_each, float leaf_final, float* out, size_t cap, size_t* n_out,
                     std::vector<float>* grow = nullptr, int sub = -1) {
        *n_out = 0;
        if (grow) grow->clear();
        if (n_ids == 0) return FLS_OK;
        if (n_ids > size_t(UINT32_MAX)) return FLS_ERR_INVALID;
        std::vector<const fls::KfCloud*> src(n_ids);
        size_t total = 0;
        for (size_t k = 0; k < n_ids; ++k) {
            src[k] = leaf_each > 0.f ? &filtered(ids[k], leaf_each) : &kf[size_t(ids[k])]->cloud;
            total += src[k]->n;
            if (total > fls::kKfMaxTotal) return FLS_ERR_INVALID;
        }
        const auto room = [&](size_t n) {
            *n_out = n;
            if (grow) { grow->resize(4 * n); out = grow->data(); return true; }
            return n <= cap;
        };
        const bool rows = sub < 0 && !(leaf_final > 0.f);
        if (sub >= 0) *n_out = total;
        if (rows && !room(total)) return FLS_ERR_INVALID;
        if (total == 0) return FLS_OK;

        // the table: one entry per selected keyframe, then the first segment of every tile
        const size_t n_tiles = (total + fls::kKfTile - 1) / fls::kKfTile;
        const size_t table_bytes = n_ids * sizeof(fls::KfSegment) + n_tiles * sizeof(unsigned);
        fls::PinnedBuf<unsigned char>& h_table = sub >= 0 ? h_sub_table[sub] : this->h_table;
        fls::DevBuf<unsigned char>& d_table = sub >= 0 ? d_sub_table[sub] : this->d_table;
        fls::DevBuf<float>& d_planes = sub >= 0 ? d_sub[sub] : this->d_planes;
        h_table.reserve(table_bytes);
        d_table.reserve(table_bytes);
        fls::KfSegment* seg = reinterpret_cast<fls::KfSegment*>(h_table.p);
        unsigned* tile_first = reinterpret_cast<unsigned*>(h_table.p + n_ids * sizeof(fls::KfSegment));
        size_t at = 0;
        for (size_t k = 0; k < n_ids; ++k) {
            const fls::KfCloud& c = *src[k];
            seg[k].x = c.plane(0); seg[k].y = c.plane(1); seg[k].z = c.plane(2); seg[k].in = c.plane(3);
            std::memcpy(seg[k].T, poses + 16 * k, sizeof(seg[k].T));
            seg[k].start = unsigned(at);
            seg[k].n = unsigned(c.n);
            at += c.n;
        }
        for (size_t b = 0, s = 0; b < n_tiles; ++b) {
            while (size_t(seg[s].start) + seg[s].n <= b * fls::kKfTile) ++s;  // (empty segments hold no point)
            tile_first[b] = unsigned(s);
        }
        if (rows) d_rows.reserve(total); else d_planes.reserve(4 * total);
        FLS_HIP(hipMemcpyAsync(d_table.p, h_table.p, table_bytes, hipMemcpyHostToDevice, stream));
        const fls::KfSegment* d_seg = reinterpret_cast<const fls::KfSegment*>(d_table.p);
        const unsigned* d_first = reinterpret_cast<const unsigned*>(d_table.p + n_ids * sizeof(fls::KfSegment));
        float* const pl = d_planes.p;
        FLS_HIP(hipEventRecord(ev_t0, stream));
        if (rows)
            hipLaunchKernelGGL(fls::kf_merge_kernel<true>, dim3(unsigned(n_tiles)), dim3(fls::kKfThreads), 0, stream, d_seg, unsigned(n_ids), d_first,
                               unsigned(total), d_rows.p, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr);
        else
            hipLaunchKernelGGL(fls::kf_merge_kernel<false>, dim3(unsigned(n_tiles)), dim3(fls::kKfThreads), 0, stream, d_seg, unsigned(n_ids), d_first,
                               unsigned(total), (float4*)nullptr, pl, pl + total, pl + 2 * total, pl + 3 * total);
        FLS_HIP(hipGetLastError());
        FLS_HIP(hipEventRecord(ev_t1, stream));
        timed = true;
        ++n_merges;
        if (sub >= 0) return FLS_OK;
        if (rows) {
            FLS_HIP(hipMemcpyAsync(out, d_rows.p, total * sizeof(float4), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            return FLS_OK;
        }
        if (vg.run(pl, pl + total, pl + 2 * total, pl + 3 * total, total, leaf_final, stream)) {
            if (!room(vg.n_out)) { FLS_HIP(hipStreamSynchronize(stream)); return FLS_ERR_INVALID; }
            download(vg.out.p, vg.n_in, vg.n_out, out);
            return FLS_OK;
        }
        const std::vector<fls::PtI> c = host_filter(pl, total, leaf_final);
        if (!room(c.size())) return FLS_ERR_INVALID;
        if (!c.empty()) std::memcpy(out, c.data(), c.size() * sizeof(fls::PtI));
        return FLS_OK;
    }
};
