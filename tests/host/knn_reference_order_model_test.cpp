// knn_reference_order_model_test.cpp -- csrc/knn_reference_order.hpp against the toolchain's own std::nth_element.  Host code only.
//   (a) kro::nth_element vs std::nth_element, the whole permutation of payloads: every n in 1..300, nth in {0, 4, n - 1, random}, keys of 1, 2, 3, 8
//       distinct values and all distinct
//   (b) the same up to n = 4,096 on sequences an adversary (McIlroy's, played against std::nth_element itself) made bad for the median of three;
//       counts the cases that reached the depth-limit branch
//   (c) kro::closest_points vs GetClosestPoint / KNNPointByCondition written with std::vector and std::nth_element: 19 voxels of 0..40 points on
//       a 1/8 m lattice, voxel misses, points beyond max_range, a voxel above the limit
// Prints "mismatches N" and "depth_limit_cases M".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../funny_lidar_slam_amd/csrc/knn_reference_order.hpp"

using fls::kro::Rec;

static long g_mismatches = 0, g_cases = 0, g_depth_cases = 0;

static bool by_d2(const Rec& a, const Rec& b) { return a.d2 < b.d2; }

// one comparison of the two selections on `keys`; returns whether the restated one reached its depth limit
static bool check_nth(const std::vector<float>& keys, const int nth) {
    const int n = int(keys.size());
    std::vector<Rec> mine(keys.size()), ref(keys.size());
    for (int i = 0; i < n; ++i) mine[size_t(i)] = ref[size_t(i)] = Rec{keys[size_t(i)], unsigned(i)};
    int hits = 0;
    fls::kro::nth_element(mine.data(), 0, nth, n, &hits);
    std::nth_element(ref.begin(), ref.begin() + nth, ref.end(), by_d2);
    bool same = true;
    for (int i = 0; i < n; ++i) same = same && mine[size_t(i)].payload == ref[size_t(i)].payload && mine[size_t(i)].d2 == ref[size_t(i)].d2;
    ++g_cases;
    if (!same) {
        if (g_mismatches < 10) std::printf("nth_element differs: n %d nth %d\n", n, nth);
        ++g_mismatches;
    }
    return hits != 0;
}

static void part_a() {
    std::mt19937 rng(20240607u);
    for (int n = 1; n <= 300; ++n) {
        for (const int distinct : {1, 2, 3, 8, 0}) {  // 0: all distinct
            std::vector<float> keys(size_t(n), 0.0f);
            if (distinct == 0) {
                for (int i = 0; i < n; ++i) keys[size_t(i)] = float(i) * 0.25f;
                std::shuffle(keys.begin(), keys.end(), rng);
            } else {
                for (float& k : keys) k = float(rng() % unsigned(distinct)) * 0.015625f;
            }
            const int nths[4] = {0, std::min(4, n - 1), n - 1, int(rng() % unsigned(n))};
            for (const int nth : nths) check_nth(keys, nth);
        }
    }
}

// McIlroy's adversary against std::nth_element(.., nth, ..) on n items: every item is "gas" until a comparison of two gas items freezes one
// to the next small value; the values it ends with make the same calls compare the same way again
static std::vector<float> killer(const int n, const int nth) {
    std::vector<int> val(static_cast<size_t>(n), n), items(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) items[size_t(i)] = i;
    int nsolid = 0, candidate = 0;
    auto cmp = [&](const int x, const int y) {
        if (val[size_t(x)] == n && val[size_t(y)] == n) val[size_t(x == candidate ? x : y)] = nsolid++;
        if (val[size_t(x)] == n) candidate = x;
        else if (val[size_t(y)] == n) candidate = y;
        return val[size_t(x)] < val[size_t(y)];
    };
    std::nth_element(items.begin(), items.begin() + nth, items.end(), cmp);
    std::vector<float> keys(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) keys[size_t(i)] = float(val[size_t(i)]);
    return keys;
}

static void part_b() {
    std::mt19937 rng(77u);
    for (const int n : {33, 64, 100, 257, 300, 1000, 2049, 4096}) {
        for (const int made_for : {0, 4, n / 2, n - 1}) {
            const std::vector<float> keys = killer(n, made_for);
            const int nths[5] = {0, 4, n / 2, n - 1, int(rng() % unsigned(n))};
            for (const int nth : nths)
                if (check_nth(keys, nth)) ++g_depth_cases;
        }
    }
}

// ---- (c) ----
struct P3 { float x, y, z; };
struct Cand { double dist; unsigned slot; bool operator<(const Cand& r) const { return dist < r.dist; } };
static const int kNearby[19][3] = {{0, 0, 0}, {-1, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, -1}, {0, 0, 1}, {1, 1, 0}, {-1, 1, 0}, {1, -1, 0},
                                   {-1, -1, 0}, {1, 0, 1}, {-1, 0, 1}, {1, 0, -1}, {-1, 0, -1}, {0, 1, 1}, {0, -1, 1}, {0, 1, -1}, {0, -1, -1}};

struct Neighbourhood {
    std::vector<P3> pts;
    unsigned begin[3][3][3], count[3][3][3];  // [dz + 1][dy + 1][dx + 1]
};

// the reference's GetClosestPoint spelled with std::vector and std::nth_element
static std::vector<unsigned> closest_std(const Neighbourhood& nb, const P3 q) {
    std::vector<Cand> cand;
    const size_t K = 5;
    for (const auto& d : kNearby) {
        const unsigned b = nb.begin[d[2] + 1][d[1] + 1][d[0] + 1], c = nb.count[d[2] + 1][d[1] + 1][d[0] + 1];
        if (c == 0) continue;
        const size_t old = cand.size();
        for (unsigned s = b; s < b + c; ++s) {
            const P3 p = nb.pts[s];
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            const double dd = dx * dx + (dy * dy + dz * dz);
            if (dd < 5.0f * 5.0f) cand.push_back(Cand{dd, s});
        }
        if (old + K >= cand.size()) {
        } else {
            std::nth_element(cand.begin() + int(old), cand.begin() + int(old) + K - 1, cand.end());
            cand.resize(old + K);
        }
    }
    std::vector<unsigned> out;
    if (cand.empty()) return out;
    if (cand.size() > K) {
        std::nth_element(cand.begin(), cand.begin() + K - 1, cand.end());
        cand.resize(K);
    }
    std::nth_element(cand.begin(), cand.begin(), cand.end());
    for (const Cand& c : cand) out.push_back(c.slot);
    return out;
}

static int closest_mine(const Neighbourhood& nb, const P3 q, const int key[3], Rec* work, const int stride) {
    return fls::kro::closest_points(
        fls::kro::Strided{work, stride}, q.x, q.y, q.z, key[0], key[1], key[2],
        [&](const int vx, const int vy, const int vz, unsigned& b, unsigned& c) {
            b = nb.begin[vz - key[2] + 1][vy - key[1] + 1][vx - key[0] + 1];
            c = nb.count[vz - key[2] + 1][vy - key[1] + 1][vx - key[0] + 1];
        },
        [&](const unsigned s, float& x, float& y, float& z) { x = nb.pts[s].x; y = nb.pts[s].y; z = nb.pts[s].z; });
}

static void part_c() {
    std::mt19937 rng(4242u);
    const int stride = 3;  // (a strided work array, as the device's)
    std::vector<Rec> work(size_t(fls::kro::kWork) * stride);
    for (int trial = 0; trial < 4000; ++trial) {
        Neighbourhood nb;
        const int key[3] = {int(rng() % 41u) - 20, int(rng() % 41u) - 20, int(rng() % 41u) - 20};
        const P3 q{float(key[0]) * 0.5f + float(int(rng() % 5u) - 2) * 0.125f, float(key[1]) * 0.5f + float(int(rng() % 5u) - 2) * 0.125f,
                   float(key[2]) * 0.5f + float(int(rng() % 5u) - 2) * 0.125f};
        const unsigned miss_pct = trial % 4 == 0 ? 90u : trial % 4 == 1 ? 50u : 10u;
        const int span = trial % 3 == 0 ? 3 : 9;  // lattice steps around the voxel centre: a narrow span makes more ties
        bool too_large = false;
        for (int z = 0; z < 3; ++z)
            for (int y = 0; y < 3; ++y)
                for (int x = 0; x < 3; ++x) {
                    unsigned c = rng() % 100u < miss_pct ? 0u : rng() % 41u;
                    if (trial % 500 == 499 && x == 1 && y == 1 && z == 0) c = unsigned(fls::kro::kVoxelLimit) + 1u;  // (0, 0, -1) is probed
                    nb.begin[z][y][x] = unsigned(nb.pts.size());
                    nb.count[z][y][x] = c;
                    too_large = too_large || c > unsigned(fls::kro::kVoxelLimit);
                    for (unsigned i = 0; i < c; ++i) {
                        P3 p{float(key[0] + x - 1) * 0.5f + float(int(rng() % unsigned(span)) - span / 2) * 0.125f,
                             float(key[1] + y - 1) * 0.5f + float(int(rng() % unsigned(span)) - span / 2) * 0.125f,
                             float(key[2] + z - 1) * 0.5f + float(int(rng() % unsigned(span)) - span / 2) * 0.125f};
                        if (rng() % 16u == 0u) p.x += 6.0f;  // beyond max_range
                        nb.pts.push_back(p);
                    }
                }
        const int n = closest_mine(nb, q, key, work.data(), stride);
        ++g_cases;
        if (too_large) {
            if (n != -1) { ++g_mismatches; std::printf("trial %d: a voxel above the limit was not refused\n", trial); }
            continue;
        }
        const std::vector<unsigned> ref = closest_std(nb, q);
        bool same = n == int(ref.size());
        for (int i = 0; same && i < n; ++i) same = work[size_t(i) * stride].payload == ref[size_t(i)];
        if (!same) {
            if (g_mismatches < 10) std::printf("closest_points differs: trial %d (%d vs %zu)\n", trial, n, ref.size());
            ++g_mismatches;
        }
    }
}

int main() {
    part_a();
    const long a_cases = g_cases;
    part_b();
    const long b_cases = g_cases - a_cases;
    part_c();
    std::printf("cases %ld + %ld + %ld\n", a_cases, b_cases, g_cases - a_cases - b_cases);
    std::printf("depth_limit_cases %ld\n", g_depth_cases);
    std::printf("mismatches %ld\n", g_mismatches);
    return g_mismatches == 0 ? 0 : 1;
}
