// ivox_blob_model_test.cpp -- the host side of the FLSIVOX1 blob built on the device (include/fls_map_ivox.h, funny_lidar_slam_amd/csrc/ivox_blob.hpp):
//   1. ivox_blob_check_header over hand-made good and bad headers, sizes that would wrap a 64-bit product included
//   2. the closed form of "a blob into an EMPTY map"  that IvoxMap::import_blob_device computes with a radix sort and two scans,
//      restated here with the product's own sort key (ivox_brick_extent, ivox_brick_major_key) and compared with the host path of an import:
//      HostIvox::rebuild_from_image (what IvoxMap::load_mirror calls) followed by HostIvox::assign_layout (what build_from_ivox uploads)
//        order   = voxels by the brick-major key, an unsigned integer compare
//        regions = cap_for(count) slots back to back from slot 0, in that order
//        stamps  = blob position + 1: the LRU list from the tail is the blob's order
// Test infrastructure: host code only, no HIP runtime call.  Built a second time with -fsanitize=address,undefined by tests/test_ivox_blob_model.py.
#include "../../funny_lidar_slam_amd/csrc/ivox_blob.hpp"
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>

using namespace fls;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { if (++g_fail < 20) std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); } } while (0)
#define CHECK(c) do { if (!(c)) { if (++g_fail < 20) std::printf("FAIL %s:%d  %s  (case %s)\n", __FILE__, __LINE__, #c, name); return; } } while (0)

static constexpr unsigned kKind = 1;  // FLS_P2PLANE_IVOX

static fls_ivox_blob_header good_header(const unsigned long long nv, const unsigned long long np) {
    fls_ivox_blob_header h{};
    std::memcpy(h.magic, FLS_IVOX_BLOB_MAGIC, 8);
    h.version = FLS_IVOX_BLOB_VERSION; h.kind = kKind; h.resolution = 0.5f; h.is_first = 0; h.capacity = 1000000; h.n_voxels = nv; h.n_points = np; h.next_id = (long long)np + 7;
    return h;
}
static fls_status check(const fls_ivox_blob_header& h, const size_t n_bytes) {
    fls_ivox_blob_header out;
    return ivox_blob_check_header(&h, n_bytes, kKind, 0.5f, out);
}
static size_t bytes_for(const unsigned long long nv, const unsigned long long np) { return sizeof(fls_ivox_blob_header) + size_t(nv + np) * 16; }

static void header_checks() {
    const size_t n = bytes_for(3, 10);
    fls_ivox_blob_header h = good_header(3, 10), out;
    EXPECT(ivox_blob_check_header(&h, n, kKind, 0.5f, out) == FLS_OK && out.n_voxels == 3 && out.n_points == 10 && out.next_id == 17);
    EXPECT(check(good_header(0, 0), bytes_for(0, 0)) == FLS_OK);  // an empty map is a blob
    EXPECT(ivox_blob_check_header(nullptr, n, kKind, 0.5f, out) == FLS_ERR_INVALID);
    for (size_t cut : {size_t(0), size_t(8), sizeof(h) - 1}) EXPECT(check(h, cut) == FLS_ERR_INVALID);                   // shorter than a header
    for (size_t m : {n - 16, n - 1, n + 1, n + 16, sizeof(h)}) EXPECT(check(h, m) == FLS_ERR_INVALID);                    // truncated, ragged, too long
    { auto b = h; b.magic[7] = '2'; EXPECT(check(b, n) == FLS_ERR_INVALID); }
    { auto b = h; std::memcpy(b.magic, "FLSIMG01", 8); EXPECT(check(b, n) == FLS_ERR_INVALID); }
    { auto b = h; b.version = 2; EXPECT(check(b, n) == FLS_ERR_INVALID); }
    { auto b = h; b.kind = 2; EXPECT(check(b, n) == FLS_ERR_INVALID); }
    for (float r : {0.25f, 0.f, -0.5f, std::nanf(""), INFINITY}) { auto b = h; b.resolution = r; EXPECT(check(b, n) == FLS_ERR_INVALID); }
    { auto b = h; b.next_id = 9; EXPECT(check(b, n) == FLS_ERR_INVALID); }    // next_id < n_points
    { auto b = h; b.next_id = 10; EXPECT(check(b, n) == FLS_OK); }
    { auto b = h; b.next_id = -1; EXPECT(check(b, n) == FLS_ERR_INVALID); }
    { auto b = good_header(10, 3); EXPECT(check(b, n) == FLS_ERR_INVALID); }  // more voxels than points
    { auto b = good_header(4, 9); EXPECT(check(b, n) == FLS_OK); }            // (the same payload split differently is a header like any other)
    { auto b = good_header(3, 11); EXPECT(check(b, n) == FLS_ERR_INVALID); }
    // counts that only fit the payload after a 64-bit wrap: (n_voxels + n_points) * 16 == payload bytes modulo 2^64
    { auto b = h; b.n_voxels = (1ull << 60) + 3; b.n_points = (1ull << 60) + 10; b.next_id = LLONG_MAX; EXPECT(check(b, n) == FLS_ERR_INVALID); }
    { auto b = h; b.n_voxels = 3; b.n_points = ~0ull - 2; b.next_id = LLONG_MAX; EXPECT(check(b, n) == FLS_ERR_INVALID); }  // n_voxels + n_points wraps to 0
    { auto b = h; b.n_voxels = ~0ull; b.n_points = 14; b.next_id = LLONG_MAX; EXPECT(check(b, n) == FLS_ERR_INVALID); }
    // the importer's own kind and resolution decide
    EXPECT(ivox_blob_check_header(&h, n, 2u, 0.5f, out) == FLS_ERR_INVALID && ivox_blob_check_header(&h, n, kKind, 0.25f, out) == FLS_ERR_INVALID);
    // keys: what pack_key writes inside the key range is canonical, nothing else
    int x, y, z;
    EXPECT(ivox_key_canonical(pack_key(-5, 7, kKeyLimit - 1), x, y, z) && x == -5 && y == 7 && z == kKeyLimit - 1);
    EXPECT(ivox_key_canonical(pack_key(-(kKeyLimit - 1), 0, 0), x, y, z) && x == -(kKeyLimit - 1));
    EXPECT(!ivox_key_canonical(pack_key(kKeyLimit, 0, 0), x, y, z) && !ivox_key_canonical(pack_key(0, -kKeyLimit, 0), x, y, z));
    EXPECT(!ivox_key_canonical(pack_key(1, 2, 3) | (1ull << 63), x, y, z) && !ivox_key_canonical(kEmptyKey, x, y, z));
}

struct Entry { unsigned long long key; unsigned k, begin, count, cap; };

// the closed form: the blob's voxel records -> layout order, regions, stamps
static std::vector<Entry> closed_form(const std::vector<fls_ivox_blob_voxel>& bv, size_t& used, int& key_bits) {
    int bmin[3] = {INT_MAX, INT_MAX, INT_MAX}, bmax[3] = {INT_MIN, INT_MIN, INT_MIN};
    for (const auto& v : bv) {
        int c[3];
        unpack_key(v.key, c[0], c[1], c[2]);
        for (int a = 0; a < 3; ++a) { bmin[a] = std::min(bmin[a], c[a] >> kBrickLog); bmax[a] = std::max(bmax[a], c[a] >> kBrickLog); }
    }
    const IvoxBrickExtent e = ivox_brick_extent(bmin, bmax);
    key_bits = e.key_bits();
    std::vector<std::pair<unsigned long long, unsigned>> order(bv.size());
    for (size_t k = 0; k < bv.size(); ++k) {
        int x, y, z;
        unpack_key(bv[k].key, x, y, z);
        order[k] = {ivox_brick_major_key(x, y, z, e.bmin[0], e.bmin[1], e.bmin[2], e.bits[0], e.bits[1]), unsigned(k)};
    }
    std::stable_sort(order.begin(), order.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    std::vector<Entry> out;
    used = 0;
    for (const auto& o : order) {
        const fls_ivox_blob_voxel& v = bv[o.second];
        const unsigned cap = HostIvox::cap_for(v.count);
        out.push_back(Entry{v.key, o.second, unsigned(used), v.count, cap});
        used += cap;
    }
    return out;
}

static void compare(const char* name, const std::vector<fls_ivox_blob_voxel>& bv, const bool expect_wide = false) {
    size_t P = 0;
    for (const auto& v : bv) P += v.count;
    std::vector<Pt4> rows(P);
    for (size_t q = 0; q < P; ++q) rows[q] = Pt4{float(q), 0.5f * float(q), -float(q), int(q) + 3};
    // the host path of an import (IvoxMap::import_blob): records with begin = prefix of the counts, stamp = position + 1
    std::vector<HostIvox::ImageVoxel> vox(bv.size());
    unsigned long long qsum = 0;
    for (size_t k = 0; k < bv.size(); ++k) { vox[k] = HostIvox::ImageVoxel{bv[k].key, unsigned(qsum), bv[k].count, 0u, (unsigned long long)(k + 1)}; qsum += bv[k].count; }
    HostIvox iv;
    iv.rebuild_from_image(vox, rows.data(), P, int(P) + 3);
    std::vector<HostIvox::LayoutRef> refs;
    const size_t slots = iv.assign_layout(refs);
    size_t used = 0;
    int key_bits = 0;
    const std::vector<Entry> m = closed_form(bv, used, key_bits);
    CHECK(key_bits <= 63 && (key_bits > 32) == expect_wide);
    CHECK(slots == used && refs.size() == m.size() && iv.n_alive == bv.size() && iv.n_points == P);
    std::vector<unsigned> src(bv.size());  // where voxel k's rows start in the blob
    for (size_t k = 0, q = 0; k < bv.size(); ++k) { src[k] = unsigned(q); q += bv[k].count; }
    for (size_t j = 0; j < m.size(); ++j) {
        const HostIvox::Voxel& v = *refs[j].v;
        CHECK(v.key == m[j].key && v.img_begin == m[j].begin && v.img_cnt == m[j].count && v.img_cap == m[j].cap && v.pts.size() == m[j].count);
        CHECK(std::memcmp(v.pts.data(), rows.data() + src[m[j].k], m[j].count * sizeof(Pt4)) == 0);
    }
    // stamps k + 1: the LRU list from the tail (oldest) is the blob's order, and IvoxImage::upload_update_meta numbers it 1 .. n from there
    size_t k = 0;
    for (int v = iv.tail; v >= 0; v = iv.pool[v].prev, ++k) { CHECK(k < bv.size()); CHECK(iv.pool[v].key == bv[k].key); }
    CHECK(k == bv.size());
}

static fls_ivox_blob_voxel vx(int x, int y, int z, unsigned count) { return fls_ivox_blob_voxel{pack_key(x, y, z), count, 0u}; }

int main() {
    header_checks();
    std::mt19937 rng(20261020);
    compare("one voxel", {vx(3, -2, 1, 1)});
    for (unsigned c : {1u, 4u, 5u, 37u, 1000u}) compare("cap steps", {vx(3, -2, 1, c), vx(4, -2, 1, 2)});
    {   // brick faces, edges and a corner
        std::vector<fls_ivox_blob_voxel> bv;
        const int edge[4] = {7, 8, -1, 0};
        for (int a : edge) for (int b : edge) for (int d : edge) bv.push_back(vx(a, b, d, 1 + unsigned(bv.size() % 9)));
        std::shuffle(bv.begin(), bv.end(), rng);
        compare("brick boundaries", bv);
    }
    {   // an extent of 2^20 voxels per axis: a sort key wider than 32 bits
        std::vector<fls_ivox_blob_voxel> bv;
        for (int sx : {-1, 1}) for (int sy : {-1, 1}) for (int sz : {-1, 1}) bv.push_back(vx(sx * 1000001, sy * 999983, sz * 1000003, 3));
        bv.push_back(vx(0, 0, 0, 5)); bv.push_back(vx(1, 0, 0, 1));
        bv.push_back(vx(kKeyLimit - 1, -(kKeyLimit - 1), kKeyLimit - 1, 2)); bv.push_back(vx(-(kKeyLimit - 1), kKeyLimit - 1, -(kKeyLimit - 1), 2));
        std::shuffle(bv.begin(), bv.end(), rng);
        compare("far corners", bv, true);
    }
    // ---- 300 seeded random voxel lists of 1 to 4,000 distinct voxels, from one brick to an extent beyond 32 key bits ----
    int wide = 0;
    for (int t = 0; t < 300; ++t) {
        std::uniform_int_distribution<int> un(1, 4000), cnt(1, t % 3 == 0 ? 70 : 9);
        const int n = t == 0 ? 1 : t == 1 ? 4000 : un(rng);
        const int extent = t % 5 == 0 ? 4 : t % 5 == 1 ? 40 : t % 5 == 2 ? 700 : t % 5 == 3 ? 60000 : kKeyLimit - 1;
        std::uniform_int_distribution<int> u(-extent, extent), w(-std::max(1, extent / 8), std::max(1, extent / 8));
        std::set<unsigned long long> seen;
        std::vector<fls_ivox_blob_voxel> bv;
        for (int i = 0; i < n; ++i) {
            const fls_ivox_blob_voxel v = vx(u(rng), u(rng), w(rng), unsigned(cnt(rng)));
            if (seen.insert(v.key).second) bv.push_back(v);
        }
        size_t used = 0;
        int key_bits = 0;
        (void)closed_form(bv, used, key_bits);
        if (key_bits > 32) ++wide;
        char name[32];
        std::snprintf(name, sizeof(name), "random %d", t);
        compare(name, bv, key_bits > 32);
    }
    EXPECT(wide >= 50);
    std::printf("ivox blob model: %d of 300 random lists with a sort key wider than 32 bits, mismatches %d\n", wide, g_fail);
    return g_fail ? 1 : 0;
}
