// ndt_image.hpp -- host side of the flat image of the NDT voxel map (include/fls_map_ndt.h): the array layout, the header checks an import
// runs before it touches anything, and the host mirror of the map (pool + intrusive LRU list + key map, the replacement of the reference's
// std::list + unordered_map, incremental_ndt.h:352-353) with the host side of AddCloudToLocalMap (insert) and its two conversions: mirror ->
// image and image rows -> mirror.  No HIP call in here: tests/host/ndt_image_model_test.cpp runs it without a device.
#pragma once
#include "../../include/fls_map_ndt.h"
#include "host_math.hpp"
#include <chrono>
#include <cstring>
#include <vector>

namespace fls {

constexpr int kNdtImageCarry = FLS_NDT_IMAGE_CARRY;  // == kNdtCarry (kernels_ndt_update.hpp)

// byte offsets of the arrays of an image of n voxels
struct NdtImageLayout {
    size_t n = 0;
    size_t key = 0, num_points = 0, vid = 0, estimated = 0, pending = 0, points = 0, mu = 0, sigma = 0, info = 0, total = 0;
};
constexpr size_t kNdtImageBytesPerVoxel = 8 + 4 + 4 + 1 + 1 + size_t(kNdtImageCarry) * 24 + 24 + 72 + 72;
// false: the sizes do not fit a size_t
inline bool ndt_image_layout(const uint64_t n_voxels, NdtImageLayout& L) {
    constexpr size_t kSlack = sizeof(fls_ndt_image_header) + 9 * 16;  // header + the padding in front of every array and behind the last
    if (n_voxels > (SIZE_MAX - kSlack) / kNdtImageBytesPerVoxel) return false;
    const size_t n = size_t(n_voxels);
    size_t o = sizeof(fls_ndt_image_header);
    auto take = [&o](const size_t bytes) { const size_t at = o; o = (o + bytes + 15) & ~size_t(15); return at; };
    L.n = n;
    L.key = take(n * 8); L.num_points = take(n * 4); L.vid = take(n * 4); L.estimated = take(n); L.pending = take(n);
    L.points = take(n * kNdtImageCarry * 24); L.mu = take(n * 24); L.sigma = take(n * 72); L.info = take(n * 72);
    L.total = o;
    return true;
}

// what of a handle's parameters the image carries
struct NdtImageParams {
    double voxel_size;
    int min_points, max_points, capacity;
};
inline uint64_t ndt_double_bits(const double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }
inline fls_ndt_image_header ndt_image_make_header(const NdtImageParams& q, const NdtImageLayout& L, const int next_vid, const bool flag_first_scan) {
    fls_ndt_image_header h;
    std::memset(&h, 0, sizeof(h));
    std::memcpy(h.magic, FLS_NDT_IMAGE_MAGIC, 8);
    h.revision = FLS_NDT_IMAGE_REVISION;
    h.carry = FLS_NDT_IMAGE_CARRY;
    h.total_bytes = L.total;
    h.n_voxels = L.n;
    h.next_vid = next_vid;
    h.flag_first_scan = flag_first_scan ? 1u : 0u;
    h.ndt_voxel_size_bits = ndt_double_bits(q.voxel_size);
    h.ndt_min_points_in_voxel = q.min_points; h.ndt_max_points_in_voxel = q.max_points; h.ndt_capacity = q.capacity;
    return h;
}
// The checks of an import that need the header alone (`head`: the first bytes of the image, n_bytes: the size the caller gave).  FLS_OK: `h` and
// `L` describe the image.  Everything per voxel is checked on the device (ndt_image_check_unpack_kernel).
inline fls_status ndt_image_check_header(const void* head, const size_t n_bytes, const NdtImageParams& q, fls_ndt_image_header& h, NdtImageLayout& L) {
    if (!head || n_bytes < sizeof(fls_ndt_image_header)) return FLS_ERR_INVALID;
    std::memcpy(&h, head, sizeof(h));
    if (std::memcmp(h.magic, FLS_NDT_IMAGE_MAGIC, 8) != 0 || h.revision != FLS_NDT_IMAGE_REVISION) return FLS_ERR_INVALID;  // (an image of another kind too)
    if (h.total_bytes != uint64_t(n_bytes)) return FLS_ERR_INVALID;
    if (h.carry != uint32_t(FLS_NDT_IMAGE_CARRY) || h.flag_first_scan > 1u || h.reserved != 0u) return FLS_ERR_INVALID;
    if (!ndt_image_layout(h.n_voxels, L) || L.total != n_bytes) return FLS_ERR_INVALID;
    if (h.ndt_voxel_size_bits != ndt_double_bits(q.voxel_size) || h.ndt_min_points_in_voxel != q.min_points || h.ndt_max_points_in_voxel != q.max_points ||
        h.ndt_capacity != q.capacity)
        return FLS_ERR_INVALID;
    if (q.capacity <= 0 || h.n_voxels >= uint64_t(q.capacity)) return FLS_ERR_INVALID;  // (an insert evicts as soon as the count reaches the capacity)
    if (h.next_vid < 0 || uint64_t(h.next_vid) < h.n_voxels) return FLS_ERR_INVALID;     // (n distinct ids below next_vid)
    return FLS_OK;
}

// ---- the host mirror ----
struct NdtMirror {
    struct Voxel {
        int kx, ky, kz;
        std::vector<double> pts;  // xyz triples waiting for the next estimate
        double mu[3] = {0, 0, 0}, sigma[9] = {0}, info[9] = {0};
        bool estimated = false;
        int num_points = 0;
        int vid = 0;
        int prev = -1, next = -1;  // LRU list (head = most recently touched)
        int slot = -1;             // row of the device image (estimated voxels only)
        unsigned epoch = 0;        // last add_cloud call that touched it
        bool dirty = false;        // mu / info changed in this call
    };
    // std::list + unordered_map of the reference (incremental_ndt.h:352-353) as a pool with an intrusive LRU list and an
    // open-addressing key map: same sequence of creations, touches and evictions, no node allocation per point
    std::vector<Voxel> pool;
    std::vector<int> free_ix;
    int lru_head = -1, lru_tail = -1;
    size_t n_alive = 0;
    FlatKeyMap grids;  // key -> pool index
    unsigned epoch = 0;
    bool flag_first_scan = true;
    int next_vid = 0;
    std::vector<unsigned long long> evicted_image_keys;  // voxels evicted since the last image sync that had a row in the host-path image
    void lru_unlink(int v) {
        Voxel& x = pool[v];
        if (x.prev >= 0) pool[x.prev].next = x.next; else lru_head = x.next;
        if (x.next >= 0) pool[x.next].prev = x.prev; else lru_tail = x.prev;
        x.prev = x.next = -1;
    }
    void lru_push_front(int v) {
        Voxel& x = pool[v];
        x.prev = -1;
        x.next = lru_head;
        if (lru_head >= 0) pool[lru_head].prev = v; else lru_tail = v;
        lru_head = v;
    }
    void clear_mirror() {
        pool.clear(); free_ix.clear(); grids.clear();
        lru_head = lru_tail = -1;
        n_alive = 0;
    }
    // one voxel from its row (device rows, image entries), as the most recently touched so far: rows fed oldest first rebuild the LRU list
    void push_row(const unsigned long long key, const int num_points, const int vid, const bool estimated, const size_t pending, const double* points,
                  const double* mu, const double* sigma, const double* info) {
        pool.emplace_back();
        Voxel& v = pool.back();
        unpack_key(key, v.kx, v.ky, v.kz);
        v.pts.assign(points, points + pending * 3);
        std::memcpy(v.mu, mu, sizeof(v.mu)); std::memcpy(v.sigma, sigma, sizeof(v.sigma)); std::memcpy(v.info, info, sizeof(v.info));
        v.estimated = estimated; v.num_points = num_points; v.vid = vid;
        const int vi = int(pool.size()) - 1;
        lru_push_front(vi);
        grids.insert(key, vi);
        ++n_alive;
    }
    // the pending points an image entry (or a device row) carries for v: none for a voxel beyond max_points, whose list is never read again
    // (`held`: the points waiting in the voxel, or a device row's carry count)
    static size_t pending_of(const bool estimated, const int num_points, const size_t held, const int max_points) {
        return std::min<size_t>((estimated && num_points > max_points) ? 0 : held, size_t(kNdtImageCarry));
    }
    static size_t pending_of(const Voxel& v, const int max_points) { return pending_of(v.estimated, v.num_points, v.pts.size() / 3, max_points); }

    static void mean_cov(const std::vector<double>& pts, double* mean, double* cov) {  // ComputeMeanAndCov :91-110
        const double* P = pts.data();
        hm::ndt_mean_cov(int(pts.size() / 3), [P](int k, double* q) { q[0] = P[3 * k]; q[1] = P[3 * k + 1]; q[2] = P[3 * k + 2]; }, mean, cov);
    }
    void update_voxel(Voxel& v, const NdtImageParams& q) const {  // UpdateVoxel :130-179
        if (flag_first_scan) {
            if (v.pts.size() / 3 > 1u) { mean_cov(v.pts, v.mu, v.sigma); hm::ndt_regularised_info(v.sigma, v.info); }
            else {
                v.mu[0] = v.pts[0]; v.mu[1] = v.pts[1]; v.mu[2] = v.pts[2];
                for (int k = 0; k < 9; ++k) v.info[k] = ((k % 4 == 0) ? 1.0 : 0.0) * 1.0e2;
            }
            v.estimated = v.dirty = true; v.pts.clear();
            return;
        }
        if (v.estimated && v.num_points > q.max_points) return;
        const int npts = int(v.pts.size() / 3);
        if (!v.estimated && npts > q.min_points) {
            mean_cov(v.pts, v.mu, v.sigma);
            hm::ndt_regularised_info(v.sigma, v.info);
            v.estimated = v.dirty = true; v.pts.clear();
        } else if (v.estimated && npts > q.min_points) {
            double cmu[3], cvar[9];
            mean_cov(v.pts, cmu, cvar);
            hm::ndt_merge(v.mu, v.sigma, v.info, v.num_points, cmu, cvar, npts);
            v.num_points += npts;
            v.dirty = true; v.pts.clear();
        }
    }
    // AddCloudToLocalMap :192-221 on the mirror: the filtered world cloud (keys in range) point by point -- insert, LRU touch, eviction at the
    // capacity -- then UpdateVoxel once per voxel the call touched.  Returns those voxels' pool indices; *t_inserted: the time between the two parts.
    std::vector<int> insert(const std::vector<PtI>& cloud_world, const NdtImageParams& q, std::chrono::steady_clock::time_point* t_inserted = nullptr) {
        const double inv_voxel = 1.0 / q.voxel_size;
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
                v.estimated = false; v.num_points = 1;
                for (int a = 0; a < 3; ++a) v.mu[a] = 0.0;  // VoxelData's initialisers (:79-81): a recycled pool entry is a new voxel
                for (int a = 0; a < 9; ++a) v.sigma[a] = v.info[a] = 0.0;
                v.vid = next_vid++;
                v.slot = -1; v.dirty = false; v.epoch = 0;
                lru_push_front(vi); grids.insert(key, vi); ++n_alive;
                if (n_alive >= size_t(q.capacity)) {  // :202-205
                    const int b = lru_tail;
                    Voxel& e = pool[b];
                    const unsigned long long ek = pack_key(e.kx, e.ky, e.kz);
                    grids.erase(ek);
                    if (e.slot >= 0) evicted_image_keys.push_back(ek);
                    e.slot = -1;
                    e.epoch = 0;  // a voxel evicted within the call that touched it gets no UpdateVoxel (the reference would dereference a null entry)
                    lru_unlink(b); free_ix.push_back(b); --n_alive;
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
        if (t_inserted) *t_inserted = std::chrono::steady_clock::now();
        size_t w = 0;
        for (size_t k = 0; k < touched.size(); ++k) {
            const int vi = touched[k];
            if (pool[vi].epoch != epoch) continue;  // evicted after its touch
            pool[vi].epoch = epoch + 0x40000000u;   // a pool entry re-created after an eviction appears twice: processed once
            update_voxel(pool[vi], q);
            touched[w++] = vi;
        }
        touched.resize(w);
        for (int vi : touched) pool[vi].epoch = epoch;
        return touched;
    }
};

// mirror -> image: lru_tail -> prev, the oldest voxel first.  dst holds ndt_image_layout(n_alive).total bytes
inline void ndt_image_from_mirror(const NdtMirror& m, const NdtImageParams& q, const int next_vid, const bool flag_first_scan, const NdtImageLayout& L,
                                  unsigned char* dst) {
    std::memset(dst, 0, L.total);
    const fls_ndt_image_header h = ndt_image_make_header(q, L, next_vid, flag_first_scan);
    std::memcpy(dst, &h, sizeof(h));
    size_t r = 0;
    for (int vi = m.lru_tail; vi >= 0 && r < L.n; vi = m.pool[vi].prev, ++r) {
        const NdtMirror::Voxel& v = m.pool[vi];
        const unsigned long long key = pack_key(v.kx, v.ky, v.kz);
        const int32_t np = v.num_points, vid = v.vid;
        const size_t pend = NdtMirror::pending_of(v, q.max_points);
        std::memcpy(dst + L.key + 8 * r, &key, 8);
        std::memcpy(dst + L.num_points + 4 * r, &np, 4);
        std::memcpy(dst + L.vid + 4 * r, &vid, 4);
        dst[L.estimated + r] = v.estimated ? 1 : 0;
        dst[L.pending + r] = (unsigned char)pend;
        if (pend) std::memcpy(dst + L.points + size_t(kNdtImageCarry) * 24 * r, v.pts.data(), pend * 24);
        std::memcpy(dst + L.mu + 24 * r, v.mu, 24);
        std::memcpy(dst + L.sigma + 72 * r, v.sigma, 72);
        std::memcpy(dst + L.info + 72 * r, v.info, 72);
    }
}
// image -> mirror (the image has passed its checks)
inline void ndt_mirror_from_image(NdtMirror& m, const unsigned char* src, const NdtImageLayout& L) {
    m.clear_mirror();
    m.pool.reserve(L.n);
    for (size_t r = 0; r < L.n; ++r) {
        unsigned long long key;
        int32_t np, vid;
        double pts[kNdtImageCarry * 3], mu[3], sg[9], inf[9];
        std::memcpy(&key, src + L.key + 8 * r, 8);
        std::memcpy(&np, src + L.num_points + 4 * r, 4);
        std::memcpy(&vid, src + L.vid + 4 * r, 4);
        std::memcpy(pts, src + L.points + size_t(kNdtImageCarry) * 24 * r, sizeof(pts));
        std::memcpy(mu, src + L.mu + 24 * r, 24); std::memcpy(sg, src + L.sigma + 72 * r, 72); std::memcpy(inf, src + L.info + 72 * r, 72);
        m.push_row(key, np, vid, src[L.estimated + r] != 0, std::min<size_t>(src[L.pending + r], size_t(kNdtImageCarry)), pts, mu, sg, inf);
    }
}

}  // namespace fls
