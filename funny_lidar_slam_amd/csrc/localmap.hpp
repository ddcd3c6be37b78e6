// localmap.hpp -- host side of the device local-map source (include/fls_localmap.h; kernels: kernels_localmap.hpp): the global map of a
// localization run and its tiles resident as x | y | z | intensity planes (KfCloud, the keyframe store's cloud), the local map cut out of
// the global map by the crop box or stitched from the filtered forms of the resident tiles, and its hand-over to a matcher on the device.
//
// The decisions are the reference's (Localization::LoadLocalMap, src/slam/localization.cpp:306-410) and live in the free functions at the
// top, which touch no device: the hysteresis of the crop box, the edges and their cast, the tile index of a pose, the enter / leave rule of
// the resident set and the stitch table (tests/host/localmap_model_test.cpp runs them on their own).  Every call ends with the stream
// drained; a call that fails has committed nothing (new state is built aside and swapped in at the end).
#pragma once
#include "kernels_localmap.hpp"
#include "keyframes.hpp"
#include <map>
#include <set>
#include <utility>

namespace fls {

constexpr double kLmMargin = 50.0;      // :382-383
constexpr double kLmHalfBox = 100.0;    // :396-402
constexpr size_t kLmCacheSlots = 2;     // filtered forms per tile
constexpr size_t kLmMaxPoints = 4000000000u;  // 32-bit point indices with room for a tile

struct LmEdges {
    bool set = false;  // local_map_edge_.empty()
    double e[6] = {0, 0, 0, 0, 0, 0};
};

// :378-389: does LoadLocalMap cut a new local map at translation t?
inline bool lm_crop_needed(const LmEdges& ed, const double t[3], const bool force) {
    if (!ed.set || force) return true;
    for (int i = 0; i < 3; ++i) {
        if (std::fabs(t[i] - ed.e[i]) > kLmMargin && std::fabs(t[i] - ed.e[i + 3]) > kLmMargin) continue;
        return true;
    }
    return false;
}
// :395-402
inline LmEdges lm_edges_at(const double t[3]) {
    LmEdges ed;
    ed.set = true;
    for (int i = 0; i < 3; ++i) { ed.e[i] = t[i] - kLmHalfBox; ed.e[i + 3] = t[i] + kLmHalfBox; }
    return ed;
}
// :404-405 Vec4d(...).cast<float>()
inline LmBox lm_box_of(const LmEdges& ed) {
    LmBox b;
    for (int i = 0; i < 3; ++i) { b.mn[i] = float(ed.e[i]); b.mx[i] = float(ed.e[i + 3]); }
    return b;
}

using LmTileKey = std::pair<int32_t, int32_t>;  // (gx, gy); std::pair's order is LessGridIndex

// :312-313 the tile of a position.  false: an index does not fit int32
inline bool lm_tile_of(const double x, const double y, const double grid, LmTileKey& c) {
    int gx = 0, gy = 0;
    if (!lm_tile_index(x, grid, grid / 2, gx) || !lm_tile_index(y, grid, grid / 2, gy)) return false;
    c = LmTileKey(gx, gy);
    return true;
}

// :316-346 on the index sets alone: the 3 x 3 neighbours of c (x outer, y inner) that exist and are not resident enter, then the resident
// tiles farther than 2 leave.  entered: in visiting order.  true: the resident set changed (need_update_local_map_).
template <class Exists>
bool lm_resident_step(const LmTileKey c, Exists&& exists, std::set<LmTileKey>& resident, std::vector<LmTileKey>& entered) {
    bool updated = false;
    entered.clear();
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy) {
            const long long gx = (long long)c.first + dx, gy = (long long)c.second + dy;
            if (gx < INT32_MIN || gx > INT32_MAX || gy < INT32_MIN || gy > INT32_MAX) continue;
            const LmTileKey k{int32_t(gx), int32_t(gy)};
            if (!exists(k) || resident.count(k)) continue;
            resident.insert(k);
            entered.push_back(k);
            updated = true;
        }
    for (auto it = resident.begin(); it != resident.end();) {
        const long long dx = (long long)it->first - c.first, dy = (long long)it->second - c.second;
        // (Vec2i difference).cast<float>().norm() > 2, in integers: exact for the small differences, and a far tile leaves before anything is squared
        if (dx > 2 || dx < -2 || dy > 2 || dy < -2 || dx * dx + dy * dy > 4) { it = resident.erase(it); updated = true; }
        else ++it;
    }
    return updated;
}

// the stitch launch's table: start[k] = points before segment k, tile_first[b] = the segment that holds output point b * tile
inline size_t lm_stitch_table(const std::vector<size_t>& counts, const size_t tile, std::vector<unsigned>& start, std::vector<unsigned>& tile_first) {
    size_t at = 0;
    start.resize(counts.size());
    for (size_t k = 0; k < counts.size(); ++k) { start[k] = unsigned(at); at += counts[k]; }
    const size_t n_tiles = (at + tile - 1) / tile;
    tile_first.resize(n_tiles);
    for (size_t b = 0, s = 0; b < n_tiles; ++b) {
        while (size_t(start[s]) + counts[s] <= b * tile) ++s;  // (empty segments hold no point)
        tile_first[b] = unsigned(s);
    }
    return at;
}

}  // namespace fls

struct fls_localmap {
    using Cloud = fls::KfCloud;
    struct Tile {
        std::shared_ptr<Cloud> owner;  // the allocation the planes lie in (one for all tiles of a split)
        const float* p[4] = {nullptr, nullptr, nullptr, nullptr};
        size_t n = 0;
        struct Cached { float leaf; std::shared_ptr<Cloud> cloud; };
        std::vector<Cached> cache;  // oldest first
    };
    using TileMap = std::map<fls::LmTileKey, Tile>;
    struct Src { const float* p[4]; size_t n; };

    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;  // around the last crop / stitch
    hipEvent_t ev_ready = nullptr;                // the hand-over: a matcher's stream waits for it
    bool timed = false;

    std::shared_ptr<Cloud> global;  // null: none stored
    fls::LmEdges edges;
    TileMap tiles;
    double grid_size = 0.0;  // 0: none in force
    std::set<fls::LmTileKey> resident;
    float stitched_leaf = -1.f;
    size_t tile_points = 0, tile_bytes = 0, cache_bytes = 0;

    fls::DevBuf<float> d_local;  // the local map: four planes, row stride n_local
    size_t n_local = 0;
    std::vector<fls::PtI> local_rows;  // its host copy, while current
    bool local_rows_current = false;

    fls::DeviceVoxelGrid vg;
    fls::DevicePairSort sort;
    fls::DevScan up;  // pinned staging of a cloud on its way to the device
    fls::DevBuf<unsigned> d_words;  // crop: counts | offsets | total;  split: mm[4] | bad | n_heads
    fls::PinnedBuf<unsigned> h_words;
    fls::DevBuf<uint2> d_heads;
    fls::DevBuf<unsigned char> d_table;
    fls::PinnedBuf<unsigned char> h_table;
    std::vector<float> tmp;
    size_t n_crops = 0, n_skipped = 0, n_filters = 0, n_hits = 0, n_declined = 0, n_stitches = 0, n_dev_handover = 0, n_host_handover = 0;

    ~fls_localmap() {
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        for (hipEvent_t e : {ev_t0, ev_t1, ev_ready}) if (e) (void)hipEventDestroy(e);
    }
    void init() {
        FLS_HIP(hipSetDevice(device));
        FLS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        FLS_HIP(hipEventCreate(&ev_t0));
        FLS_HIP(hipEventCreate(&ev_t1));
        FLS_HIP(hipEventCreateWithFlags(&ev_ready, hipEventDisableTiming));
        h_words.reserve(8);
    }

    size_t stat(int slot) {
        switch (slot) {
            case 0: return global ? global->n : 0;
            case 1: return tiles.size();
            case 2: return tile_points;
            case 3: return n_crops;
            case 4: return n_skipped;
            case 5: return n_filters;
            case 6: return n_hits;
            case 7: return n_declined;
            case 8: return n_stitches;
            case 9: return n_dev_handover;
            case 10: return n_host_handover;
            case 11: return (global ? global->bytes() : 0) + tile_bytes + cache_bytes + 4 * n_local * sizeof(float);
            case 12: {
                float ms = 0.f;
                if (!timed || hipEventElapsedTime(&ms, ev_t0, ev_t1) != hipSuccess) return 0;
                return size_t(double(ms) * 1.0e6);
            }
            default: return 0;
        }
    }

    // ---- moving clouds -------------------------------------------------------------------------------------------------------------------
    static bool staged_finite(const fls::DevScan& s) {
        for (size_t i = 0; i < 3 * s.n; ++i)
            if (!std::isfinite(s.stage.p[i])) return false;
        return true;
    }
    // the staged cloud (DevScan::stage_raw) -> a new cloud on the device
    std::shared_ptr<Cloud> upload_staged() {
        std::shared_ptr<Cloud> c = std::make_shared<Cloud>(up.n);
        if (up.n) {
            FLS_HIP(hipMemcpyAsync(c->p, up.stage.p, c->bytes(), hipMemcpyHostToDevice, stream));
            FLS_HIP(hipStreamSynchronize(stream));
        }
        return c;
    }
    std::shared_ptr<Cloud> upload_rows(const std::vector<fls::PtI>& rows) {
        up.stage_raw(rows.empty() ? nullptr : &rows[0].x, rows.size(), 4);
        return upload_staged();
    }
    // n points of four device planes -> xyzi rows on the host
    void download(const float* const p[4], size_t n, float* out) {
        if (n == 0) return;
        tmp.resize(4 * n);
        for (int a = 0; a < 4; ++a) FLS_HIP(hipMemcpyAsync(tmp.data() + size_t(a) * n, p[a], n * sizeof(float), hipMemcpyDeviceToHost, stream));
        FLS_HIP(hipStreamSynchronize(stream));
        for (size_t i = 0; i < n; ++i) { out[4 * i] = tmp[i]; out[4 * i + 1] = tmp[n + i]; out[4 * i + 2] = tmp[2 * n + i]; out[4 * i + 3] = tmp[3 * n + i]; }
    }
    // VoxelGridCloud(planes, leaf) on the device; what the device filter declines goes through the exact host filter (host_rows: the cloud on
    // the host already, or null: it is downloaded)
    std::shared_ptr<Cloud> filter(const float* const p[4], size_t n, float leaf, const float* host_rows, int host_stride) {
        if (vg.run(p[0], p[1], p[2], p[3], n, leaf, stream)) {
            std::shared_ptr<Cloud> f = std::make_shared<Cloud>(vg.n_out);
            for (int a = 0; a < 4 && vg.n_out; ++a)
                FLS_HIP(hipMemcpyAsync(f->p + size_t(a) * vg.n_out, vg.out.p + size_t(a) * vg.n_in, vg.n_out * sizeof(float), hipMemcpyDeviceToDevice, stream));
            FLS_HIP(hipStreamSynchronize(stream));  // (the filter's output planes are the next run's)
            return f;
        }
        std::vector<float> rows;
        if (!host_rows) {
            rows.resize(4 * n);
            download(p, n, rows.data());
            host_rows = rows.data();
            host_stride = 4;
        }
        ++n_declined;
        return upload_rows(fls::voxel_grid_strided(host_rows, n, host_stride, leaf));
    }

    // ---- the global cloud ------------------------------------------------------------------------------------------------------------------
    void clear_tiles() {
        tiles.clear();
        resident.clear();
        grid_size = 0.0;
        stitched_leaf = -1.f;
        tile_points = tile_bytes = cache_bytes = 0;
    }
    fls_status set_global(const float* pts, size_t n, int stride, float leaf, size_t* n_stored) {
        up.stage_raw(pts, n, stride);
        if (!(leaf > 0.f) && !staged_finite(up)) return FLS_ERR_RANGE;
        std::shared_ptr<Cloud> g = upload_staged();
        if (leaf > 0.f && n) {
            const float* const p[4] = {g->plane(0), g->plane(1), g->plane(2), g->plane(3)};
            g = filter(p, n, leaf, pts, stride);
        }
        global = std::move(g);
        edges = fls::LmEdges{};
        clear_tiles();
        n_local = 0;
        local_rows_current = false;
        if (n_stored) *n_stored = global->n;
        return FLS_OK;
    }

    // ---- the crop box ------------------------------------------------------------------------------------------------------------------------
    fls_status crop(const double* pose, int force, int* updated, size_t* n_out) {
        const double t[3] = {pose[12], pose[13], pose[14]};
        if (!fls::lm_crop_needed(edges, t, force != 0)) {
            ++n_skipped;
            *updated = 0;
            *n_out = n_local;
            return FLS_OK;
        }
        const fls::LmEdges ne = fls::lm_edges_at(t);
        const fls::LmBox box = fls::lm_box_of(ne);
        const size_t n = global->n;
        size_t kept = 0;
        if (n) {
            const unsigned nb = unsigned((n + fls::kLmTile - 1) / fls::kLmTile);
            d_words.reserve(2 * size_t(nb) + 1);
            unsigned* const counts = d_words.p;
            unsigned* const offs = d_words.p + nb;
            unsigned* const total = d_words.p + 2 * size_t(nb);
            const float *x = global->plane(0), *y = global->plane(1), *z = global->plane(2), *in = global->plane(3);
            FLS_HIP(hipEventRecord(ev_t0, stream));
            hipLaunchKernelGGL(fls::lm_crop_count_kernel, dim3(nb), dim3(fls::kLmThreads), 0, stream, x, y, z, unsigned(n), box, counts);
            hipLaunchKernelGGL(fls::lm_scan_counts_kernel, dim3(1), dim3(fls::kLmScanThreads), 0, stream, (const unsigned*)counts, offs, nb, total);
            FLS_HIP(hipGetLastError());
            FLS_HIP(hipMemcpyAsync(h_words.p, total, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));  // the size of the cut: the local map is allocated to it
            kept = h_words.p[0];
            if (kept > n) return FLS_ERR_DEVICE;
            d_local.reserve(4 * kept);
            if (kept) {
                float* const o = d_local.p;
                hipLaunchKernelGGL(fls::lm_crop_scatter_kernel, dim3(nb), dim3(fls::kLmThreads), 0, stream, x, y, z, in, unsigned(n), box, (const unsigned*)offs,
                                   unsigned(kept), o, o + kept, o + 2 * kept, o + 3 * kept);
                FLS_HIP(hipGetLastError());
            }
            FLS_HIP(hipEventRecord(ev_t1, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            timed = true;
        }
        edges = ne;
        n_local = kept;
        local_rows_current = false;
        ++n_crops;
        *updated = 1;
        *n_out = kept;
        return FLS_OK;
    }

    // ---- tiles -------------------------------------------------------------------------------------------------------------------------------
    static Tile tile_of(const std::shared_ptr<Cloud>& owner, size_t first, size_t n) {
        Tile t;
        t.owner = owner;
        for (int a = 0; a < 4; ++a) t.p[a] = owner->n ? owner->plane(a) + first : nullptr;
        t.n = n;
        return t;
    }
    void commit_tiles(TileMap&& nt, double grid) {
        clear_tiles();
        tiles = std::move(nt);
        grid_size = grid;
        std::set<const Cloud*> owners;
        for (const auto& kv : tiles) {
            tile_points += kv.second.n;
            if (owners.insert(kv.second.owner.get()).second) tile_bytes += kv.second.owner->bytes();
        }
    }
    fls_status split(double grid, size_t* n_tiles) {
        const size_t n = global->n;
        TileMap nt;
        if (n > size_t(fls::kVgMaxBlocks) * fls::kVgTile) return FLS_ERR_INVALID;  // (the radix sort's limit; larger maps come in as tiles)
        if (n) {
            const double half = grid / 2;
            const float *x = global->plane(0), *y = global->plane(1);
            d_words.reserve(8);
            int* const mm = reinterpret_cast<int*>(d_words.p);
            unsigned* const bad = d_words.p + 4;
            unsigned* const n_heads = d_words.p + 5;
            const int init[6] = {INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, 0, 0};
            std::memcpy(h_words.p, init, sizeof(init));
            FLS_HIP(hipMemcpyAsync(d_words.p, h_words.p, sizeof(init), hipMemcpyHostToDevice, stream));
            const unsigned nb_all = unsigned((n + fls::kLmThreads - 1) / fls::kLmThreads);
            hipLaunchKernelGGL(fls::lm_tile_minmax_kernel, dim3(std::min<unsigned>(nb_all, fls::kLmMaxBlocks)), dim3(fls::kLmThreads), 0, stream, x, y, unsigned(n), grid,
                               half, mm, bad);
            FLS_HIP(hipGetLastError());
            FLS_HIP(hipMemcpyAsync(h_words.p, d_words.p, 6 * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            int lim[4];
            std::memcpy(lim, h_words.p, sizeof(lim));
            if (h_words.p[4] != 0u) return FLS_ERR_RANGE;
            const unsigned long long span_x = (unsigned long long)((long long)lim[1] - lim[0]) + 1, span_y = (unsigned long long)((long long)lim[3] - lim[2]) + 1;
            if (span_x > 0xFFFFFFFFull || span_y > 0xFFFFFFFFull || span_x * span_y > 0xFFFFFFFFull) return FLS_ERR_RANGE;
            sort.prepare(n);
            hipLaunchKernelGGL(fls::lm_tile_keys_kernel, dim3(nb_all), dim3(fls::kLmThreads), 0, stream, x, y, unsigned(n), grid, half, lim[0], lim[2], unsigned(span_y),
                               sort.k0, sort.v0);
            FLS_HIP(hipGetLastError());
            sort.run(fls::DevicePairSort::passes_for(span_x * span_y - 1), stream);
            FLS_HIP(hipGetLastError());
            const size_t cap = size_t(std::min<unsigned long long>(n, span_x * span_y));
            d_heads.reserve(cap);
            hipLaunchKernelGGL(fls::lm_tile_heads_kernel, dim3(nb_all), dim3(fls::kLmThreads), 0, stream, (const unsigned*)sort.k0, unsigned(n), d_heads.p, n_heads,
                               unsigned(cap));
            FLS_HIP(hipGetLastError());
            std::shared_ptr<Cloud> sorted = std::make_shared<Cloud>(n);
            hipLaunchKernelGGL(fls::lm_gather4_kernel, dim3(nb_all), dim3(fls::kLmThreads), 0, stream, x, y, global->plane(2), global->plane(3), (const unsigned*)sort.v0,
                               unsigned(n), sorted->p, sorted->p + n, sorted->p + 2 * n, sorted->p + 3 * n);
            FLS_HIP(hipGetLastError());
            FLS_HIP(hipMemcpyAsync(h_words.p, n_heads, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            const size_t nh = h_words.p[0];
            if (nh == 0 || nh > cap) return FLS_ERR_DEVICE;
            std::vector<uint2> heads(nh);
            FLS_HIP(hipMemcpyAsync(heads.data(), d_heads.p, nh * sizeof(uint2), hipMemcpyDeviceToHost, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            std::sort(heads.begin(), heads.end(), [](const uint2& a, const uint2& b) { return a.x < b.x; });
            for (size_t k = 0; k < nh; ++k) {
                const size_t first = heads[k].y, end = k + 1 < nh ? heads[k + 1].y : n;
                if (first >= end || end > n) return FLS_ERR_DEVICE;
                const fls::LmTileKey key{int32_t((long long)lim[0] + (long long)(heads[k].x / unsigned(span_y))), int32_t((long long)lim[2] + (long long)(heads[k].x % unsigned(span_y)))};
                nt.emplace(key, tile_of(sorted, first, end - first));
            }
        }
        commit_tiles(std::move(nt), grid);
        *n_tiles = tiles.size();
        return FLS_OK;
    }
    fls_status add_tile(double grid, int32_t gx, int32_t gy, const float* pts, size_t n, int stride) {
        up.stage_raw(pts, n, stride);
        if (!staged_finite(up)) return FLS_ERR_RANGE;
        const std::shared_ptr<Cloud> c = upload_staged();
        const fls::LmTileKey key{gx, gy};
        const auto it = tiles.find(key);
        if (it != tiles.end()) {  // replaced: what was derived from the old cloud goes
            const Tile& o = it->second;
            tile_points -= o.n;
            if (o.owner.use_count() == 1) tile_bytes -= o.owner->bytes();
            for (const auto& f : o.cache) cache_bytes -= f.cloud->bytes();
            resident.erase(key);
            tiles.erase(it);
        }
        tiles.emplace(key, tile_of(c, 0, n));
        tile_points += n;
        tile_bytes += c->bytes();
        grid_size = grid;
        return FLS_OK;
    }
    fls_status list_tiles(int32_t* gxgy, uint32_t* counts, size_t cap, size_t* n_tiles) const {
        *n_tiles = tiles.size();
        if (tiles.size() > cap) return FLS_ERR_INVALID;
        size_t k = 0;
        for (const auto& kv : tiles) {
            gxgy[2 * k] = kv.first.first; gxgy[2 * k + 1] = kv.first.second;
            counts[k] = uint32_t(kv.second.n);
            ++k;
        }
        return FLS_OK;
    }
    // VoxelGridCloud(tile, leaf), from the cache or computed now (leaf > 0)
    Src filtered(Tile& t, float leaf) {
        const auto src_of = [](const Cloud& c) { return Src{{c.plane(0), c.plane(1), c.plane(2), c.plane(3)}, c.n}; };
        for (const auto& c : t.cache)
            if (c.leaf == leaf) { ++n_hits; return src_of(*c.cloud); }
        std::shared_ptr<Cloud> f = t.n ? filter(t.p, t.n, leaf, nullptr, 0) : std::make_shared<Cloud>(0);
        ++n_filters;
        if (t.cache.size() == fls::kLmCacheSlots) {  // the older one goes (nothing is in flight: every call drains the stream)
            cache_bytes -= t.cache.front().cloud->bytes();
            t.cache.erase(t.cache.begin());
        }
        cache_bytes += f->bytes();
        t.cache.push_back(Tile::Cached{leaf, std::move(f)});
        return src_of(*t.cache.back().cloud);
    }
    // the form of a tile the local map is stitched from, without counting (it was computed or found when the tile entered)
    Src form_of(Tile& t, float leaf) {
        if (!(leaf > 0.f)) return Src{{t.p[0], t.p[1], t.p[2], t.p[3]}, t.n};
        for (const auto& c : t.cache)
            if (c.leaf == leaf) return Src{{c.cloud->plane(0), c.cloud->plane(1), c.cloud->plane(2), c.cloud->plane(3)}, c.cloud->n};
        return filtered(t, leaf);
    }
    fls_status get_tile(int32_t gx, int32_t gy, float leaf, float* out, size_t cap, size_t* n_out) {
        Tile& t = tiles.find(fls::LmTileKey{gx, gy})->second;
        const Src s = leaf > 0.f ? filtered(t, leaf) : Src{{t.p[0], t.p[1], t.p[2], t.p[3]}, t.n};
        *n_out = s.n;
        if (s.n > cap) return FLS_ERR_INVALID;
        download(s.p, s.n, out);
        return FLS_OK;
    }

    // ---- the tile branch ---------------------------------------------------------------------------------------------------------------------
    fls_status load_tiles(const double* pose, float leaf, int* updated, size_t* n_out) {
        fls::LmTileKey c;
        if (!fls::lm_tile_of(pose[12], pose[13], grid_size, c)) return FLS_ERR_RANGE;
        std::set<fls::LmTileKey> next = resident;
        std::vector<fls::LmTileKey> entered;
        bool upd = fls::lm_resident_step(c, [&](const fls::LmTileKey& k) { return tiles.count(k) != 0; }, next, entered);
        const bool other_leaf = leaf != stitched_leaf && !next.empty();
        if (leaf > 0.f)  // the tiles that enter are filtered (or found in the cache) whether they stay or not (:331-333); a new leaf refilters all
            for (const fls::LmTileKey& k : entered) (void)filtered(tiles.find(k)->second, leaf);
        if (other_leaf && leaf > 0.f)
            for (const fls::LmTileKey& k : next)
                if (std::find(entered.begin(), entered.end(), k) == entered.end()) (void)filtered(tiles.find(k)->second, leaf);
        upd = upd || other_leaf;
        if (!upd) {
            *updated = 0;
            *n_out = n_local;
            return FLS_OK;
        }
        std::vector<Src> src;
        std::vector<size_t> counts;
        for (const fls::LmTileKey& k : next) {
            src.push_back(form_of(tiles.find(k)->second, leaf));
            counts.push_back(src.back().n);
        }
        std::vector<unsigned> start, tile_first;
        size_t total = 0;
        for (const size_t q : counts) total += q;
        if (total > fls::kLmMaxPoints) return FLS_ERR_INVALID;
        if (total) {
            fls::lm_stitch_table(counts, fls::kLmTile, start, tile_first);
            const size_t n_seg = src.size(), table_bytes = n_seg * sizeof(fls::LmSegment) + tile_first.size() * sizeof(unsigned);
            h_table.reserve(table_bytes);
            d_table.reserve(table_bytes);
            fls::LmSegment* seg = reinterpret_cast<fls::LmSegment*>(h_table.p);
            for (size_t k = 0; k < n_seg; ++k) seg[k] = fls::LmSegment{src[k].p[0], src[k].p[1], src[k].p[2], src[k].p[3], start[k], unsigned(counts[k])};
            std::memcpy(h_table.p + n_seg * sizeof(fls::LmSegment), tile_first.data(), tile_first.size() * sizeof(unsigned));
            d_local.reserve(4 * total);
            FLS_HIP(hipMemcpyAsync(d_table.p, h_table.p, table_bytes, hipMemcpyHostToDevice, stream));
            float* const o = d_local.p;
            FLS_HIP(hipEventRecord(ev_t0, stream));
            hipLaunchKernelGGL(fls::lm_stitch_kernel, dim3(unsigned(tile_first.size())), dim3(fls::kLmThreads), 0, stream,
                               reinterpret_cast<const fls::LmSegment*>(d_table.p), unsigned(n_seg),
                               reinterpret_cast<const unsigned*>(d_table.p + n_seg * sizeof(fls::LmSegment)), unsigned(total), o, o + total, o + 2 * total,
                               o + 3 * total);
            FLS_HIP(hipGetLastError());
            FLS_HIP(hipEventRecord(ev_t1, stream));
            FLS_HIP(hipStreamSynchronize(stream));
            timed = true;
        }
        resident.swap(next);
        stitched_leaf = leaf;
        n_local = total;
        local_rows_current = false;
        ++n_stitches;
        *updated = 1;
        *n_out = total;
        return FLS_OK;
    }

    void reset() {
        edges = fls::LmEdges{};
        resident.clear();
        stitched_leaf = -1.f;
    }

    // ---- the local map -----------------------------------------------------------------------------------------------------------------------
    const std::vector<fls::PtI>& local_on_host() {
        if (!local_rows_current) {
            local_rows.resize(n_local);
            const float* const p[4] = {d_local.p, d_local.p + n_local, d_local.p + 2 * n_local, d_local.p + 3 * n_local};
            download(p, n_local, n_local ? &local_rows[0].x : nullptr);
            local_rows_current = true;
        }
        return local_rows;
    }
    fls_status get_local(float* out, size_t cap, size_t* n_out) {
        *n_out = n_local;
        if (n_local > cap) return FLS_ERR_INVALID;
        const float* const p[4] = {d_local.p, d_local.p + n_local, d_local.p + 2 * n_local, d_local.p + 3 * n_local};
        download(p, n_local, out);
        return FLS_OK;
    }
    // matcher_->AddCloudToLocalMap({*local_map}): the matcher's stream waits for this store's; both are idle on return
    fls_status add_to(fls_matcher& m) {
        fls::HandoffCloud c;
        c.x = d_local.p; c.y = d_local.p + n_local; c.z = d_local.p + 2 * n_local; c.in = d_local.p + 3 * n_local;
        c.n = n_local;
        FLS_HIP(hipEventRecord(ev_ready, stream));
        FLS_HIP(hipStreamWaitEvent(m.stream, ev_ready, 0));
        bool took_planes = false;
        const fls_status rc = m.add_cloud_device(c, [this]() -> const std::vector<fls::PtI>& { return local_on_host(); }, &took_planes);
        FLS_HIP(hipStreamSynchronize(m.stream));
        FLS_HIP(hipStreamSynchronize(stream));
        ++(took_planes ? n_dev_handover : n_host_handover);
        return rc;
    }
};
