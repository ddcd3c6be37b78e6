// The host side of the flat NDT map image (include/fls_map_ndt.h, csrc/ndt_image.hpp) without a device: the header checks an import runs
// before it touches anything, over everything a header can be wrong in (sizes that overflow size_t included), and mirror -> bytes -> mirror
// on 200 seeded random small maps: LRU order, pending lists and the normalisation of voxels beyond max_points kept, padding zero,
// export(import(x)) == x.  Built by tests/test_ndt_image_model.py with hipcc (the product headers include the HIP headers; no HIP runtime
// call is made), once plain and once with AddressSanitizer and UBSan on the host side.
#include "../../funny_lidar_slam_amd/csrc/ndt_image.hpp"
#include <cstdio>
#include <cstring>
#include <random>

using namespace fls;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static const NdtImageParams kP{1.0, 5, 50, 400};

static fls_status check(const std::vector<unsigned char>& b, const size_t n_bytes, const NdtImageParams& q = kP) {
    fls_ndt_image_header h;
    NdtImageLayout L;
    return ndt_image_check_header(b.data(), n_bytes, q, h, L);
}
static fls_ndt_image_header header_of(const std::vector<unsigned char>& b) { fls_ndt_image_header h; std::memcpy(&h, b.data(), sizeof(h)); return h; }
static std::vector<unsigned char> with_header(std::vector<unsigned char> b, const fls_ndt_image_header& h) { std::memcpy(b.data(), &h, sizeof(h)); return b; }

// a random map: voxels created in random key order, some touched again (moved to the LRU front), every state a voxel can be in
static void random_mirror(std::mt19937& rng, NdtMirror& m, int& next_vid, const int n) {
    m.clear_mirror();
    next_vid = 0;
    auto u = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
    std::uniform_real_distribution<double> f(-50.0, 50.0);
    for (int i = 0; i < n; ++i) {
        unsigned long long key;
        do key = pack_key(u(-30, 30), u(-30, 30), u(-3, 3)); while (m.grids.find(key) >= 0);
        const int state = u(0, 3);  // 0 waiting for its first estimate, 1 estimated, 2 estimated with pending points, 3 beyond max_points
        const bool est = state != 0;
        const size_t pend = state == 0 ? size_t(u(1, kP.min_points)) : state == 2 ? size_t(u(1, kP.min_points)) : 0;
        const int np = state == 0 ? int(pend) : state == 3 ? kP.max_points + u(1, 40) : u(kP.min_points + 1, kP.max_points);
        double pts[kNdtImageCarry * 3] = {0}, mu[3] = {0}, sg[9] = {0}, inf[9] = {0};
        for (size_t k = 0; k < pend * 3; ++k) pts[k] = f(rng);
        if (est) { for (double& v : mu) v = f(rng); for (double& v : sg) v = f(rng); for (double& v : inf) v = f(rng); }
        m.push_row(key, np, next_vid++, est, pend, pts, mu, sg, inf);
        if (state == 3)  // the host path goes on appending to a list it never reads again: the image must not carry it
            for (int k = 0, e = 3 * u(1, 20); k < e; ++k) m.pool.back().pts.push_back(f(rng));
        if (u(0, 3) == 0) next_vid += u(1, 3);  // ids of voxels that were evicted since
    }
    for (int t = 0, e = u(0, 2 * n); t < e && n > 0; ++t) {  // touches
        const int vi = u(0, n - 1);
        if (m.lru_head != vi) { m.lru_unlink(vi); m.lru_push_front(vi); }
    }
}

static std::vector<unsigned char> export_mirror(const NdtMirror& m, const int next_vid, const bool first) {
    NdtImageLayout L;
    CHECK(ndt_image_layout(m.n_alive, L), "layout of %zu voxels", m.n_alive);
    std::vector<unsigned char> b(L.total, 0xAB);  // (every byte must be written: no stale 0xAB may survive)
    ndt_image_from_mirror(m, kP, next_vid, first, L, b.data());
    return b;
}

static void same_mirror(const NdtMirror& a, const NdtMirror& b, const int round) {
    CHECK(a.n_alive == b.n_alive, "round %d: %zu vs %zu voxels", round, a.n_alive, b.n_alive);
    int va = a.lru_head, vb = b.lru_head;
    size_t seen = 0;
    for (; va >= 0 && vb >= 0; va = a.pool[va].next, vb = b.pool[vb].next, ++seen) {
        const NdtMirror::Voxel &x = a.pool[va], &y = b.pool[vb];
        const size_t px = NdtMirror::pending_of(x, kP.max_points), py = NdtMirror::pending_of(y, kP.max_points);
        const bool same = x.kx == y.kx && x.ky == y.ky && x.kz == y.kz && x.estimated == y.estimated && x.num_points == y.num_points && x.vid == y.vid && px == py &&
                          (px == 0 || std::memcmp(x.pts.data(), y.pts.data(), px * 24) == 0) && std::memcmp(x.mu, y.mu, 24) == 0 &&
                          std::memcmp(x.sigma, y.sigma, 72) == 0 && std::memcmp(x.info, y.info, 72) == 0;
        CHECK(same, "round %d: voxel %zu of the LRU list differs", round, seen);
        CHECK(y.pts.size() == py * 3, "round %d: an imported voxel holds %zu doubles for %zu pending points", round, y.pts.size(), py);
        CHECK(b.grids.find(pack_key(y.kx, y.ky, y.kz)) == vb, "round %d: key map", round);
    }
    CHECK(va < 0 && vb < 0 && seen == a.n_alive, "round %d: list lengths", round);
    // the tail end of the list too
    int ta = a.lru_tail, tb = b.lru_tail;
    if (ta >= 0 && tb >= 0) CHECK(a.pool[ta].vid == b.pool[tb].vid, "round %d: LRU tails", round);
}

static void padding_is_zero(const std::vector<unsigned char>& b, const NdtImageLayout& L, const int round) {
    const size_t ends[9][2] = {{L.key, 8}, {L.num_points, 4}, {L.vid, 4}, {L.estimated, 1}, {L.pending, 1}, {L.points, size_t(kNdtImageCarry) * 24}, {L.mu, 24}, {L.sigma, 72}, {L.info, 72}};
    for (int a = 0; a < 9; ++a) {
        const size_t from = ends[a][0] + L.n * ends[a][1], to = a + 1 < 9 ? ends[a + 1][0] : L.total;
        CHECK(ends[a][0] % 16 == 0 && from <= to && to - from < 16, "round %d: array %d placed at %zu", round, a, ends[a][0]);
        for (size_t i = from; i < to; ++i) CHECK(b[i] == 0, "round %d: padding byte %zu is %u", round, i, unsigned(b[i]));
    }
    for (size_t r = 0; r < L.n; ++r) {  // the unused part of every points entry
        const size_t pend = b[L.pending + r];
        for (size_t i = pend * 24; i < size_t(kNdtImageCarry) * 24; ++i) CHECK(b[L.points + r * kNdtImageCarry * 24 + i] == 0, "round %d: entry %zu carries bytes beyond its %zu points", round, r, pend);
    }
}

int main() {
    std::mt19937 rng(20240607u);
    static_assert(sizeof(fls_ndt_image_header) == 64, "the header is 64 bytes");
    // ---- the header checks ----
    NdtMirror m;
    int next_vid = 0;
    random_mirror(rng, m, next_vid, 37);
    const std::vector<unsigned char> good = export_mirror(m, next_vid, false);
    const size_t nb = good.size();
    CHECK(check(good, nb) == FLS_OK, "a valid image is refused");
    { fls_ndt_image_header h = header_of(good); h.ndt_capacity = 38; CHECK(check(with_header(good, h), nb, NdtImageParams{1.0, 5, 50, 38}) == FLS_OK, "37 voxels fit a capacity of 38"); }
    { fls_ndt_image_header h = header_of(good); h.magic[3] ^= 0x20; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "flipped magic"); }
    { fls_ndt_image_header h = header_of(good); std::memcpy(h.magic, "FLSIVX01", 8); CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "another kind's magic"); }
    { std::vector<unsigned char> other(nb, 0); const unsigned ivox_like[4] = {0x584f5649u, 3u, 0u, 17u}; std::memcpy(other.data(), ivox_like, sizeof(ivox_like));
      CHECK(check(other, nb) == FLS_ERR_INVALID, "a blob of another kind"); }
    { fls_ndt_image_header h = header_of(good); h.revision = 2; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "revision 2"); }
    CHECK(check(good, nb - 16) == FLS_ERR_INVALID, "truncated by 16 bytes");
    CHECK(check(good, nb + 16) == FLS_ERR_INVALID, "16 bytes too many");
    CHECK(check(good, 63) == FLS_ERR_INVALID && check(good, 0) == FLS_ERR_INVALID, "shorter than a header");
    { fls_ndt_image_header h = header_of(good); h.total_bytes -= 16; CHECK(check(with_header(good, h), nb - 16) == FLS_ERR_INVALID, "truncated, total_bytes adjusted"); }
    { fls_ndt_image_header h = header_of(good); h.n_voxels += 1; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "n_voxels inflated by 1"); }
    { fls_ndt_image_header h = header_of(good); h.n_voxels *= 1000; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "n_voxels inflated"); }
    for (const uint64_t n : {~0ull, ~0ull / 378ull, ~0ull / 378ull + 1ull, (1ull << 63), (1ull << 61) + 5ull, ~0ull / 192ull}) {  // array sizes beyond size_t
        fls_ndt_image_header h = header_of(good);
        h.n_voxels = n;
        CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "n_voxels %llu", (unsigned long long)n);
        NdtImageLayout L;
        if (ndt_image_layout(n, L)) CHECK(L.total > n && L.total / 378 >= n / 2, "layout of %llu voxels wrapped around", (unsigned long long)n);
    }
    { fls_ndt_image_header h = header_of(good); h.total_bytes = ~0ull; h.n_voxels = ~0ull / 378ull; CHECK(check(with_header(good, h), size_t(~0ull)) == FLS_ERR_INVALID, "everything huge"); }
    CHECK(check(good, nb, NdtImageParams{0.5, 5, 50, 400}) == FLS_ERR_INVALID, "another voxel size");
    CHECK(check(good, nb, NdtImageParams{std::nextafter(1.0, 2.0), 5, 50, 400}) == FLS_ERR_INVALID, "a voxel size one ulp away");
    CHECK(check(good, nb, NdtImageParams{1.0, 9, 50, 400}) == FLS_ERR_INVALID, "importer with min_points 9");
    { fls_ndt_image_header h = header_of(good); h.ndt_min_points_in_voxel = 9; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "exporter with min_points 9"); }
    CHECK(check(good, nb, NdtImageParams{1.0, 5, 51, 400}) == FLS_ERR_INVALID, "another max_points");
    CHECK(check(good, nb, NdtImageParams{1.0, 5, 50, 401}) == FLS_ERR_INVALID, "another capacity");
    { fls_ndt_image_header h = header_of(good); h.ndt_capacity = 37; CHECK(check(with_header(good, h), nb, NdtImageParams{1.0, 5, 50, 37}) == FLS_ERR_INVALID, "as many voxels as the capacity"); }
    { fls_ndt_image_header h = header_of(good); h.carry = 5; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "carry width 5"); }
    { fls_ndt_image_header h = header_of(good); h.flag_first_scan = 2; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "flag_first_scan 2"); }
    { fls_ndt_image_header h = header_of(good); h.next_vid = -1; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "negative next_vid"); }
    { fls_ndt_image_header h = header_of(good); h.next_vid = 36; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "fewer ids than voxels"); }
    { fls_ndt_image_header h = header_of(good); h.reserved = 1; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "reserved word set"); }
    // ---- header only ----
    {
        NdtMirror e;
        const std::vector<unsigned char> b = export_mirror(e, 0, true);
        CHECK(b.size() == 64 && check(b, 64) == FLS_OK && header_of(b).flag_first_scan == 1 && header_of(b).n_voxels == 0, "the image of an empty map is its header");
        NdtImageLayout L;
        ndt_image_layout(0, L);
        NdtMirror back;
        ndt_mirror_from_image(back, b.data(), L);
        CHECK(back.n_alive == 0 && back.lru_head < 0 && back.lru_tail < 0, "an empty image gives an empty mirror");
    }
    // ---- mirror -> bytes -> mirror ----
    int saturated_with_points = 0, waiting = 0, estimated_pending = 0;
    for (int round = 0; round < 200; ++round) {
        NdtMirror a, b;
        int nv = 0;
        const int n = round < 4 ? round : std::uniform_int_distribution<int>(1, 150)(rng);
        random_mirror(rng, a, nv, n);
        for (int v = a.lru_head; v >= 0; v = a.pool[v].next) {
            const NdtMirror::Voxel& x = a.pool[v];
            const bool sat = x.estimated && x.num_points > kP.max_points;
            saturated_with_points += sat && !x.pts.empty();
            waiting += !x.estimated && !x.pts.empty();
            estimated_pending += x.estimated && !sat && !x.pts.empty();
        }
        const bool first = (round & 1) != 0;
        const std::vector<unsigned char> img = export_mirror(a, nv, first);
        fls_ndt_image_header h;
        NdtImageLayout L;
        CHECK(ndt_image_check_header(img.data(), img.size(), kP, h, L) == FLS_OK, "round %d: own image refused", round);
        CHECK(h.n_voxels == uint64_t(n) && h.next_vid == nv && h.flag_first_scan == (first ? 1u : 0u) && L.total == img.size(), "round %d: header", round);
        padding_is_zero(img, L, round);
        // oldest first: entry 0 is the LRU tail
        if (n) { int32_t vid0; std::memcpy(&vid0, img.data() + L.vid, 4); CHECK(vid0 == a.pool[a.lru_tail].vid, "round %d: entry 0 is not the LRU tail", round); }
        ndt_mirror_from_image(b, img.data(), L);
        same_mirror(a, b, round);
        const std::vector<unsigned char> again = export_mirror(b, nv, first);
        CHECK(again == img, "round %d: export(import(x)) != x", round);
    }
    CHECK(saturated_with_points > 0 && waiting > 0 && estimated_pending > 0, "the random maps missed a voxel state: %d %d %d", saturated_with_points, waiting, estimated_pending);
    std::printf("ndt image model: 200 random maps (%d voxels beyond max_points holding points, %d waiting, %d estimated with pending points), mismatches %d\n",
                saturated_with_points, waiting, estimated_pending, g_fail);
    return g_fail ? 1 : 0;
}
