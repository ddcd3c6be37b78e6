// fls_hip_localmap.h -- header-only C++ adapter of include/fls_localmap.h for Localization's map side: the
// global map filtered once in Run (src/slam/localization.cpp:176-187), LoadLocalMap's two branches (:306-410) and
// matcher_->AddCloudToLocalMap({*local_map}) behind them (:127-135, :217-223).  The global map and the tiles live in device memory from
// SetGlobalMap / Split / AddTile on; a reload is a cut or a stitch there, and the result goes into the matcher without visiting the host.
// Templates over the cloud and pose types; needs only fls_localmap.h (no Eigen, no PCL).  A pose type offers data() (16 doubles,
// column-major: Eigen::Matrix4d); a matcher type offers handle() (fls_hip::HipRegistration).
#pragma once
#include "fls_localmap.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace fls_hip {

class HipLocalMapSource {
public:
    explicit HipLocalMapSource(int device = 0) {
        const fls_status rc = fls_localmap_create(device, &h_);
        if (rc != FLS_OK) {
            std::fprintf(stderr, "HipLocalMapSource: fls_localmap_create failed: %s\n", fls_status_string(rc));
            std::abort();
        }
    }
    ~HipLocalMapSource() { fls_localmap_destroy(h_); }
    HipLocalMapSource(const HipLocalMapSource&) = delete;
    HipLocalMapSource& operator=(const HipLocalMapSource&) = delete;

    // Run, :176-182: global_map_cloud_ptr_ = VoxelGridCloud(LoadGlobalMap(path), 0.3); returns the points stored (0: failed or empty)
    template <class Cloud>
    size_t SetGlobalMap(const Cloud& global_map, float leaf = 0.3f) {
        size_t n = 0;
        return Check(fls_localmap_set_global(h_, Rows(global_map), global_map.points.size(), Stride(global_map), leaf, &n), "SetGlobalMap") ? n : 0;
    }

    // LoadLocalMap(pose), crop-box branch: true where the reference returns a new map_cloud (then AddTo the matcher), false where it
    // returns nullptr.  first_or_lost: `first || !has_init_` (:372-376), which clears local_map_edge_
    template <class Mat4>
    bool LoadLocalMap(const Mat4& pose, bool first_or_lost = false) {
        if (first_or_lost) (void)fls_localmap_reset(h_);
        int updated = 0;
        size_t n = 0;
        return Check(fls_localmap_crop(h_, pose.data(), 0, &updated, &n), "LoadLocalMap") && updated != 0;
    }

    // SplitMap::Split(grid_size) of the stored global map, or the tiles of an earlier Split read from their files
    size_t Split(double grid_size) {
        size_t n = 0;
        return Check(fls_localmap_split(h_, grid_size, &n), "Split") ? n : 0;
    }
    template <class Cloud>
    bool AddTile(double grid_size, int32_t gx, int32_t gy, const Cloud& tile) {
        return Check(fls_localmap_add_tile(h_, grid_size, gx, gy, Rows(tile), tile.points.size(), Stride(tile)), "AddTile");
    }
    // LoadLocalMap(pose), tile branch: leaf = registration_local_map_cloud_filter_size_; true: need_update_local_map_
    template <class Mat4>
    bool LoadTileMap(const Mat4& pose, float leaf) {
        int updated = 0;
        size_t n = 0;
        return Check(fls_localmap_load_tiles(h_, pose.data(), leaf, &updated, &n), "LoadTileMap") && updated != 0;
    }

    // matcher_->AddCloudToLocalMap({*local_map}) (:135, :222)
    template <class Matcher>
    bool AddTo(Matcher& matcher) {
        return Check(fls_add_localmap_to_local_map(matcher.handle(), h_), "AddTo");
    }

    // UpdateLocalMapCloud / the local-map publisher: the current local map on the host
    template <class Cloud>
    void GetLocalMap(Cloud& out) {
        size_t n = 0;
        (void)fls_localmap_get_local(h_, nullptr, 0, &n);
        rows_.resize(4 * n);
        if (!Check(fls_localmap_get_local(h_, rows_.data(), n, &n), "GetLocalMap")) n = 0;
        out.points.resize(n);
        for (size_t k = 0; k < n; ++k) {
            auto& p = out.points[k];
            p.x = rows_[4 * k];
            p.y = rows_[4 * k + 1];
            p.z = rows_[4 * k + 2];
            p.intensity = rows_[4 * k + 3];
        }
    }

    void Reset() { (void)fls_localmap_reset(h_); }
    size_t stat(int slot) const { return fls_localmap_stat(h_, slot); }
    fls_localmap_handle handle() const { return h_; }

private:
    template <class Cloud>
    static const float* Rows(const Cloud& c) { return c.points.empty() ? nullptr : &c.points[0].x; }
    template <class Cloud>
    static int Stride(const Cloud& c) {
        using P = typename std::remove_const<typename std::remove_reference<decltype(c.points[0])>::type>::type;
        static_assert(sizeof(P) % sizeof(float) == 0, "point rows of whole floats");
        return int(sizeof(P) / sizeof(float));
    }
    static bool Check(fls_status rc, const char* where) {
        if (rc == FLS_OK) return true;
        std::fprintf(stderr, "HipLocalMapSource::%s: %s\n", where, fls_status_string(rc));
        return false;
    }
    fls_localmap_handle h_ = nullptr;
    std::vector<float> rows_;
};

}  // namespace fls_hip
