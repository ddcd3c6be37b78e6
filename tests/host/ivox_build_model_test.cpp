// ivox_build_model_test.cpp -- the closed form of "a cloud inserted into an EMPTY iVox map" (DESIGN.md 3), which the device-side bulk build
// (funny_lidar_slam_amd/csrc/kernels_ivox_build.hpp, IvoxMap::bulk_build) computes, restated on the host as a stable sort plus scans and
// compared with the product's sequential path: HostIvox::add_points (the reference's insert / LRU loop) followed by the slot layout of a full
// image build (HostIvox::assign_layout, what IvoxImage::build_from_ivox uploads).  The model never calls add_points.
//   voxels  = the distinct keys; members in cloud order, ids = cloud indices; next_id = n_points = n
//   layout  = voxels by (z >> 3, y >> 3, x >> 3, z, y, x), regions of cap_for(count) slots back to back from 0, slack {0, 0, 0, -1}
//   LRU     = voxels by the index of their LAST member, descending from the head
//   decline = a point that fails key_of (the call fails with FLS_ERR_RANGE), or V >= capacity (the sequential insert evicts)
// Test infrastructure: host code only, no HIP runtime call.  Built a second time with -fsanitize=address,undefined by tests/test_ivox_build_model.py.
#include "../../funny_lidar_slam_amd/csrc/host_maps.hpp"
#include <cstdio>
#include <cstring>
#include <random>

using namespace fls;

struct ModelVoxel { unsigned long long key; unsigned begin, count, cap; };
struct Model {
    bool range_error = false, declined = false;  // declined: range_error or V >= capacity
    size_t V = 0, used = 0;
    std::vector<ModelVoxel> vox;          // layout order
    std::vector<Pt4> pts;                 // [used]
    std::vector<unsigned long long> lru;  // head (most recent) first
};

static Model model_build(const std::vector<PtI>& c, const float inv, const size_t capacity) {
    Model m;
    const size_t n = c.size();
    struct Rec { int bz, by, bx, z, y, x; unsigned i; };
    std::vector<Rec> r(n);
    for (size_t i = 0; i < n; ++i) {
        int x, y, z;
        if (!HostIvox::key_of(c[i].x, c[i].y, c[i].z, inv, x, y, z)) { m.range_error = m.declined = true; return m; }
        r[i] = Rec{z >> kBrickLog, y >> kBrickLog, x >> kBrickLog, z, y, x, unsigned(i)};
    }
    std::stable_sort(r.begin(), r.end(), [](const Rec& a, const Rec& b) {
        return std::make_tuple(a.bz, a.by, a.bx, a.z, a.y, a.x) < std::make_tuple(b.bz, b.by, b.bx, b.z, b.y, b.x);
    });
    std::vector<std::pair<unsigned, unsigned long long>> last;  // {index of the last member, key}
    for (size_t a = 0; a < n;) {  // segment heads, counts, capacities, exclusive scan of the capacities
        size_t b = a + 1;
        while (b < n && r[b].x == r[a].x && r[b].y == r[a].y && r[b].z == r[a].z) ++b;
        ModelVoxel v{pack_key(r[a].x, r[a].y, r[a].z), unsigned(m.used), unsigned(b - a), HostIvox::cap_for(b - a)};
        m.pts.resize(m.used + v.cap, Pt4{0.f, 0.f, 0.f, -1});
        for (size_t k = a; k < b; ++k) m.pts[m.used + (k - a)] = Pt4{c[r[k].i].x, c[r[k].i].y, c[r[k].i].z, int(r[k].i)};
        last.push_back({r[b - 1].i, v.key});  // (stable sort: the members are in cloud order)
        m.used += v.cap;
        m.vox.push_back(v);
        a = b;
    }
    m.V = m.vox.size();
    std::sort(last.begin(), last.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    for (const auto& l : last) m.lru.push_back(l.second);
    if (m.V >= capacity) m.declined = true;
    return m;
}

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { if (++g_fail < 20) std::printf("FAIL %s:%d  %s  (case %s)\n", __FILE__, __LINE__, #c, name); return; } } while (0)

static void compare(const char* name, const std::vector<PtI>& c, const size_t capacity) {
    HostIvox iv;
    iv.capacity = capacity;
    const Model m = model_build(c, iv.inv_resolution, capacity);
    const fls_status rc = iv.add_points(c.data(), c.size());
    CHECK((rc == FLS_ERR_RANGE) == m.range_error);
    if (m.range_error) { CHECK(iv.n_alive == 0 && iv.n_points == 0 && iv.next_id == 0); return; }  // all or nothing
    CHECK(rc == FLS_OK);
    CHECK(iv.evicted_keys.empty() == !m.declined);  // the sequential insert evicts exactly when V >= capacity
    if (m.declined) return;
    CHECK(iv.n_alive == m.V && iv.n_points == c.size() && size_t(iv.next_id) == c.size());
    std::vector<HostIvox::LayoutRef> refs;
    const size_t slots = iv.assign_layout(refs);
    CHECK(slots == m.used && refs.size() == m.V);
    for (size_t k = 0; k < m.V; ++k) {
        const HostIvox::Voxel& v = *refs[k].v;
        const ModelVoxel& w = m.vox[k];
        CHECK(v.key == w.key && v.img_begin == w.begin && v.img_cnt == w.count && v.img_cap == w.cap && v.pts.size() == w.count);
        CHECK(std::memcmp(v.pts.data(), m.pts.data() + w.begin, w.count * sizeof(Pt4)) == 0);
        for (unsigned s = w.count; s < w.cap; ++s) {
            const Pt4& q = m.pts[w.begin + s];
            CHECK(q.x == 0.f && q.y == 0.f && q.z == 0.f && q.id == -1);
        }
    }
    size_t k = 0;
    for (int v = iv.head; v >= 0; v = iv.pool[v].next, ++k) { CHECK(k < m.lru.size()); CHECK(iv.pool[v].key == m.lru[k]); }
    CHECK(k == m.V);
    CHECK(m.V == 0 || iv.pool[iv.tail].key == m.lru.back());
}

static PtI at_voxel(int x, int y, int z, float jitter = 0.f) { return PtI{0.5f * x + jitter, 0.5f * y - jitter, 0.5f * z + jitter, 1.f}; }

int main() {
    const size_t big = 1000000;
    std::mt19937 rng(20251019);
    // ---- hand-made clouds ----
    compare("one point", {PtI{1.f, 2.f, 3.f, 0.f}}, big);
    for (int n : {1, 4, 5, 37}) {  // the cap_for steps
        std::vector<PtI> c;
        for (int i = 0; i < n; ++i) c.push_back(at_voxel(3, -2, 1, 0.001f * i));
        compare("one voxel", c, big);
    }
    {   // brick faces, edges and a corner: voxel coordinates 7 | 8 and -1 | 0 on each axis
        std::vector<PtI> c;
        const int edge[4] = {7, 8, -1, 0};
        for (int a : edge) for (int b : edge) for (int d : edge) { c.push_back(at_voxel(a, b, d)); c.push_back(at_voxel(d, a, b, 0.01f)); }
        std::shuffle(c.begin(), c.end(), rng);
        compare("brick boundaries", c, big);
    }
    {   // round half away from zero: coordinates exactly at +-0.25 and +-0.75
        std::vector<PtI> c;
        const float h[4] = {0.25f, -0.25f, 0.75f, -0.75f};
        for (float a : h) for (float b : h) for (float d : h) c.push_back(PtI{a, b, d, 0.f});
        compare("half-way coordinates", c, big);
        int x, y, z;
        HostIvox::key_of(0.25f, -0.25f, 0.75f, 2.0f, x, y, z);
        if (!(x == 1 && y == -1 && z == 2)) { std::printf("FAIL round half away\n"); ++g_fail; }
    }
    {   // A, B, A, A, B: LRU by last member, and the consecutive-same-key shortcut of add_points
        const PtI A = at_voxel(1, 1, 1), B = at_voxel(20, 1, 1);
        compare("ABAAB", {A, B, A, A, B}, big);
        compare("ABAA", {A, B, A, A}, big);
    }
    for (int V : {63, 64, 65}) {  // capacity 64: the model must decline at exactly V >= C
        std::vector<PtI> c;
        for (int v = 0; v < V; ++v) { c.push_back(at_voxel(v, 0, 0)); c.push_back(at_voxel(v, 0, 0, 0.01f)); }
        std::shuffle(c.begin(), c.end(), rng);
        compare("capacity 64", c, 64);
        const Model m = model_build(c, 2.0f, 64);
        if (m.declined != (V >= 64)) { std::printf("FAIL decline at V=%d\n", V); ++g_fail; }
    }
    {   // outside the key range, not a number
        std::vector<PtI> c{at_voxel(1, 2, 3), PtI{float(kKeyLimit) * 0.5f, 0.f, 0.f, 0.f}, at_voxel(4, 5, 6)};
        compare("key limit", c, big);
        if (!model_build(c, 2.0f, big).range_error) { std::printf("FAIL key limit not flagged\n"); ++g_fail; }
        c[1] = PtI{0.f, std::nanf(""), 0.f, 0.f};
        compare("NaN", c, big);
        if (!model_build(c, 2.0f, big).range_error) { std::printf("FAIL NaN not flagged\n"); ++g_fail; }
        c[1] = PtI{(float(kKeyLimit) - 1.f) * 0.5f, 0.f, 0.f, 0.f};  // the last key inside
        compare("last key inside", c, big);
        if (model_build(c, 2.0f, big).range_error) { std::printf("FAIL last key inside flagged\n"); ++g_fail; }
    }
    // ---- 200 seeded random clouds of 1 to 5,000 points: dense (many members per voxel) to sparse, some at a capacity near their voxel count ----
    int declined = 0;
    for (int t = 0; t < 200; ++t) {
        std::uniform_int_distribution<int> un(1, 5000);
        const size_t n = t == 0 ? 1 : t == 1 ? 5000 : size_t(un(rng));
        const float extent = t % 4 == 0 ? 1.5f : t % 4 == 1 ? 6.f : t % 4 == 2 ? 30.f : 400.f;
        std::uniform_real_distribution<float> u(-extent, extent), w(-0.1f * extent, 0.1f * extent);
        std::vector<PtI> c(n);
        for (auto& p : c) { p.x = u(rng); p.y = u(rng); p.z = w(rng); p.i = 0.f; }
        if (t % 3 == 0)  // runs of consecutive points in one voxel, as a scan line gives
            for (size_t i = 1; i < n; ++i) if (i % 4) { c[i] = c[i - 1]; c[i].x += 0.001f; }
        size_t cap = big;
        if (t % 5 == 4) { const Model probe = model_build(c, 2.0f, big); cap = std::max<size_t>(2, probe.V + size_t(t % 3) - 1); }  // V - 1, V, V + 1
        if (model_build(c, 2.0f, cap).declined) ++declined;
        char name[32];
        std::snprintf(name, sizeof(name), "random %d", t);
        const char* nm = name;
        (void)nm;
        compare(name, c, cap);
    }
    std::printf("ivox build model: %d random clouds declined at their capacity, mismatches %d\n", declined, g_fail);
    return g_fail ? 1 : 0;
}
