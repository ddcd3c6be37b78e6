// The bookkeeping of the kd-tree kinds' lazy host deque (csrc/kd_lazy_deque.hpp) without a device: 200 seeded random sequences of
// push-device, push-host, trim, reset, fetch and import on a KdLazyDeque, with a plain std::deque of vectors kept beside it as the checker
// and four host arrays standing in for the DeviceCloudRing's (csrc/kd_map.hpp) planes (clouds back to back from a head that advances with every pop and
// returns to 0 with a re-pack).  After every step: count, sizes and point total equal the checker's, every cloud the host holds equals the
// checker's bit for bit (NaN payloads and negative zeros among the values), the missing runs are maximal, cover exactly what is missing
// and name the ring floats the clouds lie at; after a fetch nothing is missing and the whole deque equals the checker.  Built by
// tests/test_kd_push_model.py with hipcc (the product headers include the HIP headers; no HIP runtime call is made), once plain and once
// with AddressSanitizer and UBSan on the host side.
#include "../../funny_lidar_slam_amd/csrc/kd_lazy_deque.hpp"
#include <cstdio>
#include <cstring>
#include <random>

using namespace fls;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// the ring's stand-in: four planes of 32-bit words, the live clouds at head .. tail
struct HostRing {
    std::vector<unsigned> pl[4];
    size_t head = 0;
    size_t tail() const { return pl[0].size(); }
    void push(const std::vector<PtI>& c) {
        for (const PtI& q : c) {
            unsigned w[4];
            std::memcpy(w, &q, 16);
            for (int a = 0; a < 4; ++a) pl[a].push_back(w[a]);
        }
    }
    void pop(const size_t n) { head += n; }
    void repack() {  // DeviceCloudRing::make_room: the live floats move to the front
        for (int a = 0; a < 4; ++a) pl[a].erase(pl[a].begin(), pl[a].begin() + long(head));
        head = 0;
    }
    void clear() { for (int a = 0; a < 4; ++a) pl[a].clear(); head = 0; }
};

static int g_nan = 0, g_negzero = 0, g_empty = 0;
static std::vector<PtI> random_cloud(std::mt19937& rng) {
    auto u = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
    std::uniform_real_distribution<float> f(-50.f, 50.f);
    const int n = u(0, 4) == 0 ? 0 : u(1, 40);
    g_empty += n == 0;
    std::vector<PtI> cloud(size_t(n), PtI{0.f, 0.f, 0.f, 0.f});
    for (PtI& q : cloud) {
        unsigned w[4];
        for (unsigned& x : w) {
            const float v = f(rng);
            std::memcpy(&x, &v, 4);
            const int k = u(0, 19);
            if (k == 0) { x = 0x7fc00000u | unsigned(u(1, 0x3fffff)); ++g_nan; }        // a quiet NaN with a payload
            else if (k == 1) { x = 0xff800001u + unsigned(u(0, 0x3ffffe)); ++g_nan; }  // a signalling one, sign set
            else if (k == 2) { x = 0x80000000u; ++g_negzero; }
        }
        std::memcpy(static_cast<void*>(&q), w, 16);
    }
    return cloud;
}
static bool same_cloud(const std::vector<PtI>& a, const std::vector<PtI>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(PtI)) == 0);
}

struct World {
    KdLazyDeque lazy;
    KdDeque ref;   // the checker: what the reference's deque holds
    HostRing ring;
    void fetch() {
        for (const KdLazyDeque::Run& r : lazy.missing_runs()) {
            const size_t at = ring.head + r.offset;
            CHECK(at + r.n_points <= ring.tail(), "a run reaches past the ring's tail");
            lazy.fill(r, ring.pl[0].data() + at, ring.pl[1].data() + at, ring.pl[2].data() + at, ring.pl[3].data() + at);
        }
    }
    void check(const int seq, const int step, const char* op) {
        CHECK(lazy.size() == ref.size() && lazy.clouds.size() == ref.size() && lazy.have.size() == ref.size(), "%d.%d %s: count", seq, step, op);
        if (lazy.size() != ref.size()) return;
        size_t points = 0, missing = 0;
        for (size_t k = 0; k < ref.size(); ++k) {
            CHECK(lazy.sizes[k] == ref[k].size(), "%d.%d %s: size of cloud %zu", seq, step, op, k);
            points += ref[k].size();
            if (lazy.have[k]) CHECK(same_cloud(lazy.clouds[k], ref[k]), "%d.%d %s: host copy of cloud %zu", seq, step, op, k);
            else { ++missing; CHECK(lazy.clouds[k].empty(), "%d.%d %s: a missing cloud holds memory", seq, step, op); }
        }
        CHECK(lazy.points() == points && ring.tail() - ring.head == points, "%d.%d %s: points", seq, step, op);
        CHECK(lazy.n_missing == missing && lazy.complete() == (missing == 0), "%d.%d %s: missing count", seq, step, op);
        // the runs: ascending, maximal, exactly the missing clouds, at the clouds' ring offsets
        std::vector<unsigned char> covered(ref.size(), 0);
        size_t prev_end = 0;
        bool first = true;
        for (const KdLazyDeque::Run& r : lazy.missing_runs()) {
            CHECK(r.n_clouds > 0 && r.first + r.n_clouds <= ref.size(), "%d.%d %s: run bounds", seq, step, op);
            CHECK(first || r.first > prev_end, "%d.%d %s: runs touch or overlap", seq, step, op);  // (touching runs would be one run)
            size_t off = 0, np = 0;
            for (size_t k = 0; k < r.first; ++k) off += ref[k].size();
            for (size_t k = r.first; k < r.first + r.n_clouds && k < ref.size(); ++k) { np += ref[k].size(); covered[k] = 1; }
            CHECK(r.offset == off && r.n_points == np, "%d.%d %s: run at %zu + %zu, expected %zu + %zu", seq, step, op, r.offset, r.n_points, off, np);
            prev_end = r.first + r.n_clouds;
            first = false;
        }
        for (size_t k = 0; k < ref.size(); ++k) CHECK(covered[k] == (lazy.have[k] ? 0 : 1), "%d.%d %s: cloud %zu and the runs", seq, step, op, k);
    }
};

int main() {
    int n_op[6] = {0, 0, 0, 0, 0, 0}, dropped_unfetched = 0, fetched_runs_of_two = 0, fetches_with_missing = 0;
    for (int seq = 0; seq < 200; ++seq) {
        std::mt19937 rng(20250300u + unsigned(seq));
        auto u = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
        World w;
        const size_t max_clouds = size_t(u(1, 6));
        const int steps = u(10, 60);
        for (int step = 0; step < steps; ++step) {
            const int r = u(0, 99);
            const char* op;
            if (r < 40) {  // a keyframe pushed on the device, then the reference's trim
                op = "push-device";
                ++n_op[0];
                const std::vector<PtI> c = random_cloud(rng);
                w.ring.push(c); w.ref.push_back(c);
                w.lazy.push_device(c.size());
            } else if (r < 60) {
                op = "push-host";
                ++n_op[1];
                const std::vector<PtI> c = random_cloud(rng);
                w.ring.push(c); w.ref.push_back(c);
                w.lazy.push_host(c);
            } else if (r < 75) {
                op = "trim";
                ++n_op[2];
                const size_t keep = u(0, 3) == 0 ? size_t(u(0, 3)) : max_clouds;
                const bool expect = w.ref.size() > keep;
                if (expect) {
                    dropped_unfetched += !w.lazy.have.front();
                    w.ring.pop(w.ref.front().size());
                    w.ref.pop_front();
                }
                CHECK(w.lazy.trim(keep) == expect, "%d.%d trim's answer", seq, step);
                if (u(0, 2) == 0) w.ring.repack();
            } else if (r < 80) {  // localization mode: the map is the last cloud alone
                op = "reset";
                ++n_op[3];
                const std::vector<PtI> c = random_cloud(rng);
                w.ring.clear(); w.ref.clear();
                w.ring.push(c); w.ref.push_back(c);
                w.lazy.clear();
                w.lazy.push_host(c);
            } else if (r < 93) {
                op = "fetch";
                ++n_op[4];
                fetches_with_missing += !w.lazy.complete();
                for (const KdLazyDeque::Run& q : w.lazy.missing_runs()) fetched_runs_of_two += q.n_clouds >= 2;
                w.fetch();
                CHECK(w.lazy.complete() && w.lazy.missing_runs().empty(), "%d.%d fetch left something missing", seq, step);
                for (size_t k = 0; k < w.ref.size() && k < w.lazy.clouds.size(); ++k) CHECK(same_cloud(w.lazy.clouds[k], w.ref[k]), "%d.%d fetched cloud %zu", seq, step, k);
            } else {
                op = "import";
                ++n_op[5];
                KdDeque all;
                const int n = u(0, int(max_clouds));
                for (int k = 0; k < n; ++k) all.push_back(random_cloud(rng));
                w.ring.clear();
                for (const auto& c : all) w.ring.push(c);
                w.ref = all;
                w.lazy.assign(std::move(all));
                CHECK(w.lazy.complete(), "%d.%d an import leaves everything present", seq, step);
            }
            w.check(seq, step, op);
        }
        w.fetch();
        w.check(seq, steps, "final fetch");
        CHECK(w.lazy.complete(), "%d: final fetch", seq);
    }
    for (int k = 0; k < 6; ++k) CHECK(n_op[k] > 100, "operation %d ran %d times", k, n_op[k]);
    CHECK(dropped_unfetched > 50 && fetched_runs_of_two > 50 && fetches_with_missing > 100 && g_nan > 100 && g_negzero > 100 && g_empty > 50,
          "the random sequences missed a case: %d %d %d %d %d %d", dropped_unfetched, fetched_runs_of_two, fetches_with_missing, g_nan, g_negzero, g_empty);
    std::printf("kd push model: 200 sequences (%d device pushes, %d host pushes, %d trims of which %d dropped a cloud never fetched, %d resets, %d fetches, %d imports), mismatches %d\n",
                n_op[0], n_op[1], n_op[2], dropped_unfetched, n_op[3], n_op[4], n_op[5], g_fail);
    return g_fail ? 1 : 0;
}
