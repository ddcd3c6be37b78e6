// The host logic of the device local-map source (csrc/localmap.hpp) without a device, held against a direct restatement of
// Localization::LoadLocalMap (src/slam/localization.cpp:306-410): the hysteresis decision of the crop box, the edges and their cast to
// float corners, the box test on its faces, the tile index of a position (also where it does not fit an int), the enter / leave rule of
// the resident tile set and the stitch table -- on hand-made cases and on 240 seeded random pose walks.  Built by
// tests/test_localmap_model.py with hipcc (the product headers include the HIP headers; no HIP runtime call is made), once plain and once
// with AddressSanitizer and UBSan on the host side.
#include "../../funny_lidar_slam_amd/csrc/localmap.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

using namespace fls;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// ---- the restatement: the reference's own statements on its own containers -------------------------------------------------------------
struct RefCrop {
    std::vector<double> edge;  // local_map_edge_
    bool step(const double t[3]) {  // :378-402; true: need_update_local_map_
        bool need = false;
        if (edge.empty()) {
            need = true;
        } else {
            for (int i = 0; i < 3; ++i) {
                if (std::fabs(t[i] - edge[i]) > 50.0 && std::fabs(t[i] - edge[i + 3]) > 50.0) continue;
                need = true;
                break;
            }
        }
        if (!need) return false;
        edge.resize(6);
        edge[0] = t[0] - 100.0; edge[1] = t[1] - 100.0; edge[2] = t[2] - 100.0;
        edge[3] = t[0] + 100.0; edge[4] = t[1] + 100.0; edge[5] = t[2] + 100.0;
        return true;
    }
};
struct RefTiles {
    std::set<std::pair<int, int>> map_data_indices;  // the tiles there are
    std::map<std::pair<int, int>, int> local_map_data;  // resident: index -> times filtered (the value stands for the cloud)
    std::vector<std::pair<int, int>> entered;
    bool step(const double x, const double y, const double g) {  // :310-346
        bool need = false;
        entered.clear();
        const double half = g / 2;
        const int cx = int(std::floor((x - half) / g)), cy = int(std::floor((y - half) / g));
        for (int i = -1; i <= 1; ++i)      // GenerateTileMapIndices(curr, 1): x outer, y inner
            for (int j = -1; j <= 1; ++j) {
                const std::pair<int, int> k(cx + i, cy + j);
                if (map_data_indices.find(k) == map_data_indices.end()) continue;
                if (local_map_data.find(k) == local_map_data.end()) { local_map_data[k] = 1; entered.push_back(k); need = true; }
            }
        for (auto it = local_map_data.begin(); it != local_map_data.end();) {
            const float dx = float(it->first.first - cx), dy = float(it->first.second - cy);
            if (std::sqrt(dx * dx + dy * dy) > 2) { local_map_data.erase(it++); need = true; }
            else ++it;
        }
        return need;
    }
};

static void test_crop_decision() {
    LmEdges ed;
    const double t0[3] = {12.25, -3.5, 1.125};
    CHECK(lm_crop_needed(ed, t0, false), "empty edges");
    ed = lm_edges_at(t0);
    CHECK(ed.set && ed.e[0] == -87.75 && ed.e[3] == 112.25 && ed.e[1] == -103.5 && ed.e[4] == 96.5 && ed.e[2] == -98.875 && ed.e[5] == 101.125, "edges");
    CHECK(!lm_crop_needed(ed, t0, false) && lm_crop_needed(ed, t0, true), "centre / force");
    // exactly 50 m from an edge is NOT "> 50": the call does the work; one step inside it does not
    for (int a = 0; a < 3; ++a)
        for (int s = -1; s <= 1; s += 2) {
            double t[3] = {t0[0], t0[1], t0[2]};
            t[a] = t0[a] + s * 50.0;
            CHECK(lm_crop_needed(ed, t, false), "axis %d side %d at the margin", a, s);
            t[a] = std::nextafter(t[a], t0[a]);
            CHECK(!lm_crop_needed(ed, t, false), "axis %d side %d inside the margin", a, s);
            t[a] = t0[a] + s * 250.0;  // beyond the box on that axis: both distances > 50 again -- the reference's rule, kept as it is
            CHECK(!lm_crop_needed(ed, t, false), "axis %d side %d far outside", a, s);
        }
    // the cast and the faces
    const double t1[3] = {1234.56789, -0.1, 1e-9};
    const LmEdges e1 = lm_edges_at(t1);
    const LmBox b = lm_box_of(e1);
    for (int a = 0; a < 3; ++a) CHECK(b.mn[a] == float(t1[a] - 100.0) && b.mx[a] == float(t1[a] + 100.0), "corner cast %d", a);
    const float c[3] = {float(t1[0]), float(t1[1]), float(t1[2])};
    CHECK(lm_in_box(b, c[0], c[1], c[2]), "centre");
    for (int a = 0; a < 3; ++a) {
        float p[3] = {c[0], c[1], c[2]};
        p[a] = b.mn[a]; CHECK(lm_in_box(b, p[0], p[1], p[2]), "on min face %d", a);
        p[a] = std::nextafter(b.mn[a], -INFINITY); CHECK(!lm_in_box(b, p[0], p[1], p[2]), "below min face %d", a);
        p[a] = std::nextafter(b.mn[a], INFINITY); CHECK(lm_in_box(b, p[0], p[1], p[2]), "above min face %d", a);
        p[a] = b.mx[a]; CHECK(lm_in_box(b, p[0], p[1], p[2]), "on max face %d", a);
        p[a] = std::nextafter(b.mx[a], INFINITY); CHECK(!lm_in_box(b, p[0], p[1], p[2]), "above max face %d", a);
        p[a] = std::nextafter(b.mx[a], -INFINITY); CHECK(lm_in_box(b, p[0], p[1], p[2]), "below max face %d", a);
    }
}

static void test_tile_index() {
    LmTileKey k;
    CHECK(lm_tile_of(0.0, 0.0, 100.0, k) && k == LmTileKey(-1, -1), "origin: floor(-0.5)");
    CHECK(lm_tile_of(50.0, 149.999, 100.0, k) && k == LmTileKey(0, 0), "boundary belongs to the upper tile");
    CHECK(lm_tile_of(std::nextafter(50.0, 0.0), 150.0, 100.0, k) && k == LmTileKey(-1, 1), "one step below the boundary");
    CHECK(lm_tile_of(-150.0, -150.0001, 100.0, k) && k == LmTileKey(-2, -3), "negative side");
    CHECK(lm_tile_of(18.75 + 3 * 37.5, 18.75 - 2 * 37.5, 37.5, k) && k == LmTileKey(3, -2), "grid 37.5");
    CHECK(!lm_tile_of(1e300, 0.0, 100.0, k) && !lm_tile_of(0.0, -1e13, 1e-3, k), "does not fit an int");
    CHECK(!lm_tile_of(NAN, 0.0, 100.0, k) && !lm_tile_of(0.0, INFINITY, 100.0, k), "not finite");
    int g = 0;
    CHECK(lm_tile_index(2147483647.0 * 2.0 + 1.0, 2.0, 1.0, g) && g == 2147483647, "INT_MAX fits");
    CHECK(!lm_tile_index(2147483648.0 * 2.0 + 1.0, 2.0, 1.0, g), "INT_MAX + 1 does not");
    CHECK(lm_tile_index(-2147483648.0 * 2.0 + 1.0, 2.0, 1.0, g) && g == -2147483647 - 1, "INT_MIN fits");
}

static void test_resident_rule_at_int_limits() {
    std::set<LmTileKey> res = {LmTileKey(INT32_MIN, INT32_MIN), LmTileKey(INT32_MAX, INT32_MAX), LmTileKey(0, 0)};
    std::vector<LmTileKey> entered;
    const auto all = [](const LmTileKey&) { return true; };
    CHECK(lm_resident_step(LmTileKey(INT32_MAX, INT32_MIN), all, res, entered), "updated");
    CHECK(entered.size() == 4 && res.size() == 4, "only the neighbours inside the int range enter (%zu, %zu)", entered.size(), res.size());
    CHECK(!res.count(LmTileKey(0, 0)) && !res.count(LmTileKey(INT32_MIN, INT32_MIN)) && !res.count(LmTileKey(INT32_MAX, INT32_MAX)), "the far ones left");
}

static void test_stitch_table() {
    std::vector<unsigned> start, first;
    const std::vector<size_t> counts = {0, 5, 0, 1024, 3, 0, 2048, 1, 0};
    const size_t total = lm_stitch_table(counts, 1024, start, first);
    CHECK(total == 3081 && first.size() == 4, "total %zu tiles %zu", total, first.size());
    for (size_t b = 0; b < first.size(); ++b) {
        const size_t s = first[b], p = b * 1024;
        CHECK(counts[s] > 0 && start[s] <= p && p < start[s] + counts[s], "tile %zu starts in segment %zu", b, s);
    }
    CHECK(lm_stitch_table({}, 1024, start, first) == 0 && first.empty(), "no segments");
    CHECK(lm_stitch_table({0, 0}, 1024, start, first) == 0 && first.empty(), "empty segments");
    CHECK(lm_stitch_table({1}, 1024, start, first) == 1 && first.size() == 1 && first[0] == 0, "one point");
}

static void test_random_walks(const int n_walks) {
    for (int w = 0; w < n_walks; ++w) {
        std::mt19937_64 rng(1000 + w);
        std::uniform_real_distribution<double> u(-1.0, 1.0);
        const double grid = (w % 3 == 0) ? 100.0 : (w % 3 == 1) ? 37.5 : 12.0 + 50.0 * std::fabs(u(rng));
        const double step = (w % 4 == 0) ? 10.0 : (w % 4 == 1) ? 45.0 : (w % 4 == 2) ? 120.0 : 400.0;
        // the tiles there are: a patch with random holes
        RefTiles ref;
        for (int i = -8; i <= 8; ++i)
            for (int j = -8; j <= 8; ++j)
                if (u(rng) > -0.6) ref.map_data_indices.insert({i, j});
        RefCrop rc;
        LmEdges ed;
        std::set<LmTileKey> resident;
        std::vector<LmTileKey> entered;
        double t[3] = {300.0 * u(rng), 300.0 * u(rng), 20.0 * u(rng)};
        for (int s = 0; s < 60; ++s) {
            const bool forced = s % 17 == 16, reset = s % 23 == 22;
            if (reset) { rc.edge.clear(); ed = LmEdges{}; ref.local_map_data.clear(); resident.clear(); }
            if (forced) rc.edge.clear();  // (force = the caller's way to say "cut anyway": the reference has none; an empty edge list does it)
            const bool need_ref = rc.step(t);
            const bool need = lm_crop_needed(ed, t, forced);
            CHECK(need == need_ref, "walk %d step %d: crop decision %d vs %d", w, s, int(need), int(need_ref));
            if (need) ed = lm_edges_at(t);
            CHECK(ed.set == !rc.edge.empty() && (rc.edge.empty() || std::memcmp(ed.e, rc.edge.data(), sizeof(ed.e)) == 0), "walk %d step %d: edges", w, s);
            const LmBox b = lm_box_of(ed);
            for (int a = 0; a < 3 && !rc.edge.empty(); ++a) CHECK(b.mn[a] == float(rc.edge[a]) && b.mx[a] == float(rc.edge[a + 3]), "walk %d step %d: corners", w, s);

            const bool upd_ref = ref.step(t[0], t[1], grid);
            LmTileKey c;
            CHECK(lm_tile_of(t[0], t[1], grid, c), "walk %d step %d: tile of the pose", w, s);
            const bool upd = lm_resident_step(c, [&](const LmTileKey& k) { return ref.map_data_indices.count({k.first, k.second}) != 0; }, resident, entered);
            CHECK(upd == upd_ref, "walk %d step %d: updated %d vs %d", w, s, int(upd), int(upd_ref));
            bool same = resident.size() == ref.local_map_data.size() && entered.size() == ref.entered.size();
            if (same) {
                auto it = ref.local_map_data.begin();
                for (const LmTileKey& k : resident) { same = same && k.first == it->first.first && k.second == it->first.second; ++it; }  // the stitch order
                for (size_t q = 0; q < entered.size(); ++q) same = same && entered[q].first == ref.entered[q].first && entered[q].second == ref.entered[q].second;
            }
            CHECK(same, "walk %d step %d: resident set / entering order", w, s);
            for (int a = 0; a < 3; ++a) t[a] += (a == 2 ? 0.05 : 1.0) * step * u(rng);
        }
    }
}

int main() {
    test_crop_decision();
    test_tile_index();
    test_resident_rule_at_int_limits();
    test_stitch_table();
    test_random_walks(240);
    std::printf("localmap model: 240 walks, mismatches %d\n", g_fail);
    return g_fail ? 1 : 0;
}
