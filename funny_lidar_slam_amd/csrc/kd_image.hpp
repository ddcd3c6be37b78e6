// kd_image.hpp -- host side of the flat image of the kd-tree kinds' local maps (include/fls_map_kd.h): the layout arithmetic with its
// overflow checks, the checks an import runs before it touches anything (header, sizes, padding), and the two conversions deque -> bytes
// and bytes -> deque.  No HIP call in here: tests/host/kd_image_model_test.cpp runs all of it without a device.  A batch lane
// (`KdMatcher::owner != nullptr`, matchers_kd.hpp) never gets here: it exports 0 bytes and refuses every import with FLS_ERR_INVALID.
#pragma once
#include "../../include/fls_map_kd.h"
#include "host_maps.hpp"
#include <cstring>
#include <deque>
#include <vector>

namespace fls {

static_assert(sizeof(fls_kd_image_header) == 224 && sizeof(fls_kd_image_header) % 16 == 0, "the header is 224 bytes");
static_assert(sizeof(PtI) == 16, "a deque point is an image row");

// byte offsets of the arrays of an image
struct KdImageLayout {
    int n_maps = 0;
    size_t n_clouds[2] = {0, 0}, n_points[2] = {0, 0};
    size_t sizes[2] = {0, 0}, rows[2] = {0, 0};
    size_t total = 0;
};
// false: the sizes do not fit a size_t
inline bool kd_image_layout(const int n_maps, const uint64_t* n_clouds, const uint64_t* n_points, KdImageLayout& L) {
    if (n_maps < 1 || n_maps > 2) return false;
    L = KdImageLayout();
    L.n_maps = n_maps;
    size_t o = sizeof(fls_kd_image_header);
    // `bytes` more, rounded up to the next 16-byte boundary (o is one already)
    auto take = [&o](const uint64_t count, const size_t width, size_t& at) {
        if (o > SIZE_MAX - 15 || count > (SIZE_MAX - 15 - o) / width) return false;
        at = o;
        o = (o + size_t(count) * width + 15) & ~size_t(15);
        return true;
    };
    for (int m = 0; m < n_maps; ++m) {
        if (!take(n_clouds[m], 4, L.sizes[m]) || !take(n_points[m], 16, L.rows[m])) return false;
        L.n_clouds[m] = size_t(n_clouds[m]);
        L.n_points[m] = size_t(n_points[m]);
    }
    L.total = o;
    return true;
}

// what of a handle's parameters the image carries, and what they allow
struct KdImageParams {
    uint32_t kind = 0, n_maps = 1;
    bool localization = false;
    float filter_size[2] = {0.f, 0.f};
    uint32_t local_size[2] = {0, 0};
    double point_search_thres = 0.0;
    bool gated = false;          // point_search_thres shapes the map (the cell size of the search grid)
    uint64_t max_clouds[2] = {0, 0};  // what the kind's deque may hold
};
inline uint64_t kd_double_bits(const double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }
inline uint32_t kd_float_bits(const float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }
inline KdImageParams kd_image_params(const fls_kind kind, const fls_params& p) {
    KdImageParams q;
    q.kind = uint32_t(kind);
    q.localization = p.is_localization_mode != 0;
    if (kind == FLS_LOAM_FULL) {  // (no localization switch in this kind's map update)
        q.n_maps = 2;
        q.filter_size[0] = p.planar_voxel_filter_size; q.filter_size[1] = p.corner_voxel_filter_size;
        q.local_size[0] = p.local_planar_size; q.local_size[1] = p.local_corner_size;
        q.max_clouds[0] = p.local_planar_size; q.max_clouds[1] = p.local_corner_size;
    } else {
        q.filter_size[0] = p.map_cloud_filter_size;
        q.local_size[0] = p.local_map_size;
        q.max_clouds[0] = q.localization ? 1u : p.local_map_size;
    }
    q.gated = kind != FLS_P2PLANE_KDTREE;
    q.point_search_thres = q.gated ? p.point_search_thres : 0.0;
    return q;
}
// the keyframe gate as the image carries it
struct KdImageGate {
    bool init = false;
    double last_T[16] = {0};
};
inline fls_kd_image_header kd_image_make_header(const KdImageParams& q, const KdImageGate& g, const KdImageLayout& L) {
    fls_kd_image_header h;
    std::memset(&h, 0, sizeof(h));
    std::memcpy(h.magic, FLS_KD_IMAGE_MAGIC, 8);
    h.revision = FLS_KD_IMAGE_REVISION;
    h.kind = q.kind;
    h.total_bytes = L.total;
    h.n_maps = q.n_maps;
    h.is_localization_mode = q.localization ? 1u : 0u;
    for (int m = 0; m < 2; ++m) { h.filter_size_bits[m] = kd_float_bits(q.filter_size[m]); h.local_size[m] = q.local_size[m]; }
    h.point_search_thres_bits = q.gated ? kd_double_bits(q.point_search_thres) : 0ull;
    h.gate_init = g.init ? 1u : 0u;
    if (g.init) std::memcpy(h.gate_last_T, g.last_T, sizeof(h.gate_last_T));
    for (int m = 0; m < L.n_maps; ++m) { h.n_clouds[m] = L.n_clouds[m]; h.n_points[m] = L.n_points[m]; }
    return h;
}

// The checks of an import that need the header alone (`head`: the first bytes of the image, n_bytes: the size the caller gave).  FLS_OK: `h`
// and `L` describe the image, and kd_image_check_body may read n_bytes of it.
inline fls_status kd_image_check_header(const void* head, const size_t n_bytes, const KdImageParams& q, fls_kd_image_header& h, KdImageLayout& L) {
    if (!head || n_bytes < sizeof(fls_kd_image_header)) return FLS_ERR_INVALID;
    std::memcpy(&h, head, sizeof(h));
    if (std::memcmp(h.magic, FLS_KD_IMAGE_MAGIC, 8) != 0 || h.revision != FLS_KD_IMAGE_REVISION) return FLS_ERR_INVALID;  // (an image of another kind too)
    if (h.kind != q.kind || h.n_maps != q.n_maps || q.n_maps < 1 || q.n_maps > 2) return FLS_ERR_INVALID;
    if (h.total_bytes != uint64_t(n_bytes)) return FLS_ERR_INVALID;
    if (h.is_localization_mode != (q.localization ? 1u : 0u) || h.reserved != 0u) return FLS_ERR_INVALID;
    for (int m = 0; m < 2; ++m)
        if (h.filter_size_bits[m] != kd_float_bits(q.filter_size[m]) || h.local_size[m] != q.local_size[m]) return FLS_ERR_INVALID;
    if (h.point_search_thres_bits != (q.gated ? kd_double_bits(q.point_search_thres) : 0ull)) return FLS_ERR_INVALID;
    if (h.gate_init > 1u) return FLS_ERR_INVALID;
    for (int k = 0; k < 16; ++k) {
        const uint64_t b = kd_double_bits(h.gate_last_T[k]);
        if (h.gate_init ? ((b >> 52) & 0x7ffull) == 0x7ffull : b != 0ull) return FLS_ERR_INVALID;  // NaN / infinity | anything but +0
    }
    for (int m = 0; m < 2; ++m) {
        if (m >= int(q.n_maps) ? (h.n_clouds[m] != 0 || h.n_points[m] != 0) : h.n_clouds[m] > q.max_clouds[m]) return FLS_ERR_INVALID;
        if (h.n_clouds[m] == 0 && h.n_points[m] != 0) return FLS_ERR_INVALID;
    }
    if (!kd_image_layout(int(q.n_maps), h.n_clouds, h.n_points, L) || L.total != n_bytes) return FLS_ERR_INVALID;
    return FLS_OK;
}
// The checks that read the arrays (img: the whole image in host memory, its header has passed): every map's sizes sum to its n_points,
// every padding byte is zero.  Point values are not looked at.
inline fls_status kd_image_check_body(const unsigned char* img, const KdImageLayout& L) {
    for (int m = 0; m < L.n_maps; ++m) {
        uint64_t sum = 0;
        for (size_t c = 0; c < L.n_clouds[m]; ++c) {
            uint32_t s;
            std::memcpy(&s, img + L.sizes[m] + 4 * c, 4);
            sum += s;  // (at most 2^32 clouds of less than 2^32 points each: no wrap)
        }
        if (sum != uint64_t(L.n_points[m])) return FLS_ERR_INVALID;
        for (size_t i = L.sizes[m] + 4 * L.n_clouds[m]; i < L.rows[m]; ++i)
            if (img[i] != 0) return FLS_ERR_INVALID;
        // (rows are whole 16-byte units: no padding behind them)
    }
    return FLS_OK;
}

using KdDeque = std::deque<std::vector<PtI>>;
using KdSizes = std::deque<size_t>;  // the points of every cloud of a deque: all the layout, the header and the sizes array need of it

// the layout of the image of `maps[0 .. n_maps)`; false: too large for the format (a cloud of 2^32 points) or for a size_t
inline bool kd_image_layout_of(const KdSizes* const* maps, const int n_maps, KdImageLayout& L) {
    uint64_t nc[2] = {0, 0}, np[2] = {0, 0};
    for (int m = 0; m < n_maps && m < 2; ++m) {
        nc[m] = maps[m]->size();
        for (const size_t s : *maps[m]) {
            if (s > 0xffffffffull) return false;
            np[m] += s;
        }
    }
    return kd_image_layout(n_maps, nc, np, L);
}
// Header + sizes of every map, with the padding behind them, and nothing of the rows: what the device export writes from the host.
// chunk[0] receives the image bytes [0, rows[0]): the header and map 0's sizes; chunk[1] the bytes [sizes[1], rows[1]): map 1's sizes
inline void kd_image_write_meta(const KdImageParams& q, const KdImageGate& g, const KdImageLayout& L, const KdSizes* const* maps, unsigned char* const* chunk) {
    const fls_kd_image_header h = kd_image_make_header(q, g, L);
    std::memcpy(chunk[0], &h, sizeof(h));
    for (int m = 0; m < L.n_maps; ++m) {
        unsigned char* const at = m == 0 ? chunk[0] + L.sizes[0] : chunk[1];
        std::memset(at, 0, L.rows[m] - L.sizes[m]);
        size_t c = 0;
        for (const size_t n : *maps[m]) {
            const uint32_t s = uint32_t(n);
            std::memcpy(at + 4 * c++, &s, 4);
        }
    }
}
// the same two from the deques themselves
struct KdSizesOf {
    KdSizes s[2];
    const KdSizes* p[2] = {&s[0], &s[1]};
    KdSizesOf(const KdDeque* const* maps, const int n_maps) {
        for (int m = 0; m < n_maps && m < 2; ++m)
            for (const auto& c : *maps[m]) s[m].push_back(c.size());
    }
    KdSizesOf(const KdSizesOf&) = delete;
    KdSizesOf& operator=(const KdSizesOf&) = delete;
};
inline bool kd_image_layout_of(const KdDeque* const* maps, const int n_maps, KdImageLayout& L) {
    const KdSizesOf s(maps, n_maps);
    return kd_image_layout_of(s.p, n_maps, L);
}
inline void kd_image_write_meta(const KdImageParams& q, const KdImageGate& g, const KdImageLayout& L, const KdDeque* const* maps, unsigned char* const* chunk) {
    const KdSizesOf s(maps, L.n_maps);
    kd_image_write_meta(q, g, L, s.p, chunk);
}
// deque -> image.  dst holds L.total bytes; every one of them is written
inline void kd_image_from_deques(const KdImageParams& q, const KdImageGate& g, const KdImageLayout& L, const KdDeque* const* maps, unsigned char* dst) {
    unsigned char* const chunk[2] = {dst, dst + L.sizes[L.n_maps > 1 ? 1 : 0]};
    kd_image_write_meta(q, g, L, maps, chunk);
    for (int m = 0; m < L.n_maps; ++m) {
        size_t at = L.rows[m];
        for (const auto& cloud : *maps[m]) {
            if (!cloud.empty()) std::memcpy(dst + at, cloud.data(), cloud.size() * sizeof(PtI));
            at += cloud.size() * sizeof(PtI);
        }
    }
}
// image -> deque of map m (the image has passed its checks)
inline void kd_deque_from_image(const unsigned char* img, const KdImageLayout& L, const int m, KdDeque& out) {
    out.clear();
    size_t at = L.rows[m];
    for (size_t c = 0; c < L.n_clouds[m]; ++c) {
        uint32_t s;
        std::memcpy(&s, img + L.sizes[m] + 4 * c, 4);
        out.emplace_back(size_t(s));
        if (s) std::memcpy(static_cast<void*>(out.back().data()), img + at, size_t(s) * sizeof(PtI));
        at += size_t(s) * sizeof(PtI);
    }
}
inline KdImageGate kd_gate_from_header(const fls_kd_image_header& h) {
    KdImageGate g;
    g.init = h.gate_init != 0u;
    if (g.init) std::memcpy(g.last_T, h.gate_last_T, sizeof(g.last_T));
    return g;
}

}  // namespace fls
