// The host side of the flat image of the kd-tree kinds' local maps (include/fls_map_kd.h, csrc/kd_image.hpp) without a device: the checks
// an import runs before it touches anything, over everything a header can be wrong in (sizes that overflow size_t included) and over the
// arrays (sizes that do not sum up, non-zero padding), and deque -> bytes -> deque on 200 seeded random small deques: 0-8 clouds of 0-50
// points, one and two maps, NaN payloads and negative zeros in the rows, byte-exact, export(import(x)) == x.  Built by
// tests/test_kd_image_model.py with hipcc (the product headers include the HIP headers; no HIP runtime call is made), once plain and once
// with AddressSanitizer and UBSan on the host side.
// A batch lane (a matcher with `owner != nullptr`) never reaches this code: its export answers 0 bytes and its import FLS_ERR_INVALID
// before anything is read (KdMatcher in csrc/matchers_kd.hpp); no public call hands out a lane, so no test drives one.
#include "../../funny_lidar_slam_amd/csrc/kd_image.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

using namespace fls;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static fls_params icp_params(const int localization = 0) {
    fls_params p;
    std::memset(&p, 0, sizeof(p));
    p.is_localization_mode = localization;
    p.local_map_size = 8;
    p.local_planar_size = 8;
    p.local_corner_size = 6;
    p.map_cloud_filter_size = 0.5f;
    p.planar_voxel_filter_size = 0.4f;
    p.corner_voxel_filter_size = 0.2f;
    p.point_search_thres = 1.0;
    return p;
}
static const KdImageParams kIcp = kd_image_params(FLS_ICP_OPTIMIZED, icp_params());
static const KdImageParams kLoam = kd_image_params(FLS_LOAM_FULL, icp_params());
static const KdImageParams kKd = kd_image_params(FLS_P2PLANE_KDTREE, icp_params());

static fls_status check(const std::vector<unsigned char>& b, const size_t n_bytes, const KdImageParams& q = kIcp) {
    fls_kd_image_header h;
    KdImageLayout L;
    const fls_status rc = kd_image_check_header(b.data(), n_bytes, q, h, L);
    if (rc != FLS_OK) return rc;
    return kd_image_check_body(b.data(), L);  // (n_bytes == L.total == what `b` holds, or the header check has refused)
}
static fls_kd_image_header header_of(const std::vector<unsigned char>& b) { fls_kd_image_header h; std::memcpy(&h, b.data(), sizeof(h)); return h; }
static std::vector<unsigned char> with_header(std::vector<unsigned char> b, const fls_kd_image_header& h) { std::memcpy(b.data(), &h, sizeof(h)); return b; }

static float float_of(const uint32_t bits) { float f; std::memcpy(&f, &bits, 4); return f; }
static int g_nan = 0, g_negzero = 0, g_empty = 0;
static void random_deque(std::mt19937& rng, KdDeque& d, const int n_clouds) {
    d.clear();
    auto u = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
    std::uniform_real_distribution<float> f(-50.f, 50.f);
    for (int c = 0; c < n_clouds; ++c) {
        const int n = u(0, 3) == 0 ? 0 : u(0, 50);
        g_empty += n == 0;
        std::vector<PtI> cloud(size_t(n), PtI{0.f, 0.f, 0.f, 0.f});
        for (PtI& q : cloud) {
            float v[4] = {f(rng), f(rng), f(rng), f(rng)};
            for (float& x : v) {
                const int k = u(0, 19);
                if (k == 0) { x = float_of(0x7fc00000u | uint32_t(u(1, 0x3fffff))); ++g_nan; }        // a quiet NaN with a payload
                else if (k == 1) { x = float_of(0xff800001u + uint32_t(u(0, 0x3ffffe))); ++g_nan; }  // a signalling one, sign set
                else if (k == 2) { x = float_of(0x80000000u); ++g_negzero; }
            }
            std::memcpy(static_cast<void*>(&q), v, 16);
        }
        d.push_back(std::move(cloud));
    }
}
static bool same_deque(const KdDeque& a, const KdDeque& b) {
    if (a.size() != b.size()) return false;
    for (size_t c = 0; c < a.size(); ++c) {
        if (a[c].size() != b[c].size()) return false;
        if (!a[c].empty() && std::memcmp(a[c].data(), b[c].data(), a[c].size() * sizeof(PtI)) != 0) return false;
    }
    return true;
}
static std::vector<unsigned char> export_deques(const KdImageParams& q, const KdImageGate& g, const KdDeque* const* maps, KdImageLayout& L) {
    CHECK(kd_image_layout_of(maps, int(q.n_maps), L), "layout");
    std::vector<unsigned char> b(L.total, 0xAB);  // (every byte must be written: no stale 0xAB may survive)
    kd_image_from_deques(q, g, L, maps, b.data());
    return b;
}
static KdImageGate some_gate(std::mt19937& rng, const bool init) {
    KdImageGate g;
    g.init = init;
    std::uniform_real_distribution<double> f(-100.0, 100.0);
    if (init) for (double& v : g.last_T) v = f(rng);
    return g;
}

int main() {
    std::mt19937 rng(20240611u);
    // ---- the header checks ----
    KdDeque d0;
    random_deque(rng, d0, 5);
    d0.push_back(std::vector<PtI>(7, PtI{1.f, 2.f, 3.f, 4.f}));  // (never empty altogether)
    const KdDeque* one[2] = {&d0, nullptr};
    KdImageLayout L0;
    const KdImageGate gate1 = some_gate(rng, true);
    const std::vector<unsigned char> good = export_deques(kIcp, gate1, one, L0);
    const size_t nb = good.size();
    CHECK(check(good, nb) == FLS_OK, "a valid image is refused");
    CHECK(nb % 16 == 0 && L0.sizes[0] == 224 && L0.rows[0] % 16 == 0, "layout");
    { fls_kd_image_header h = header_of(good); h.magic[3] ^= 0x20; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "flipped magic"); }
    { fls_kd_image_header h = header_of(good); std::memcpy(h.magic, "FLSNDT01", 8); CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "the NDT image's magic"); }
    { std::vector<unsigned char> other(nb, 0); const unsigned ivox_like[4] = {0x584f5649u, 3u, 0u, 17u}; std::memcpy(other.data(), ivox_like, sizeof(ivox_like));
      CHECK(check(other, nb) == FLS_ERR_INVALID, "a blob of another kind"); }
    { fls_kd_image_header h = header_of(good); h.revision = 2; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "revision 2"); }
    CHECK(check(good, nb, kKd) == FLS_ERR_INVALID, "an ICP image into a P2PlaneKd handle");
    CHECK(check(good, nb, kLoam) == FLS_ERR_INVALID, "an ICP image into a LoamFull handle");
    { fls_kd_image_header h = header_of(good); h.kind = uint32_t(FLS_P2PLANE_KDTREE); CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "kind rewritten"); }
    { fls_kd_image_header h = header_of(good); h.n_maps = 2; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "two maps in an ICP image"); }
    { fls_kd_image_header h = header_of(good); h.n_maps = 0; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "no map"); }
    CHECK(check(good, nb - 16) == FLS_ERR_INVALID, "truncated by 16 bytes");
    CHECK(check(good, nb + 16) == FLS_ERR_INVALID, "16 bytes too many");
    CHECK(check(good, 223) == FLS_ERR_INVALID && check(good, 0) == FLS_ERR_INVALID, "shorter than a header");
    { fls_kd_image_header h = header_of(good); h.total_bytes -= 16; CHECK(check(with_header(good, h), nb - 16) == FLS_ERR_INVALID, "truncated, total_bytes adjusted"); }
    { fls_kd_image_header h = header_of(good); h.n_points[0] += 1; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "n_points inflated by 1"); }
    { fls_kd_image_header h = header_of(good); h.n_points[0] -= 1; h.total_bytes -= 16; CHECK(check(with_header(good, h), nb - 16) == FLS_ERR_INVALID, "sizes sum to one more than n_points"); }
    { fls_kd_image_header h = header_of(good); h.n_clouds[0] += 3; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "nine clouds where the deque holds eight"); }
    { fls_kd_image_header h = header_of(good); h.n_clouds[0] += 3; KdImageParams q = kIcp; q.max_clouds[0] = 9; CHECK(check(with_header(good, h), nb, q) == FLS_ERR_INVALID, "n_clouds inflated by 3"); }
    { fls_kd_image_header h = header_of(good); h.n_clouds[1] = 1; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "clouds of a map the kind does not have"); }
    { fls_kd_image_header h = header_of(good); h.n_points[1] = 1; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "points of a map the kind does not have"); }
    for (const uint64_t n : {~0ull, ~0ull / 16ull, ~0ull / 16ull + 1ull, (1ull << 63), (1ull << 60), (1ull << 60) - 14ull, ~0ull / 4ull}) {  // array sizes beyond size_t
        fls_kd_image_header h = header_of(good);
        h.n_points[0] = n;
        CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "n_points %llu", (unsigned long long)n);
        h = header_of(good);
        h.n_clouds[0] = n;
        KdImageParams q = kIcp;
        q.max_clouds[0] = ~0ull;  // (past the deque limit, so that the layout arithmetic is what refuses)
        CHECK(check(with_header(good, h), nb, q) == FLS_ERR_INVALID, "n_clouds %llu", (unsigned long long)n);
        KdImageLayout L;
        const uint64_t nc[2] = {3, 0}, np[2] = {n, 0};
        if (kd_image_layout(1, nc, np, L)) CHECK(L.total > n && L.total / 16 >= n, "layout of %llu points wrapped around", (unsigned long long)n);
        const uint64_t nc2[2] = {n, n}, np2[2] = {n, n};
        if (kd_image_layout(2, nc2, np2, L)) CHECK(L.total > n && L.total / 40 >= n, "layout of 2 x %llu wrapped around", (unsigned long long)n);
    }
    { fls_kd_image_header h = header_of(good); h.total_bytes = ~0ull; h.n_points[0] = ~0ull / 16ull - 20ull; CHECK(check(with_header(good, h), size_t(~0ull)) == FLS_ERR_INVALID, "everything huge"); }
    { KdImageParams q = kIcp; q.filter_size[0] = 0.25f; CHECK(check(good, nb, q) == FLS_ERR_INVALID, "another map_cloud_filter_size"); }
    { KdImageParams q = kIcp; q.filter_size[0] = std::nextafter(0.5f, 1.f); CHECK(check(good, nb, q) == FLS_ERR_INVALID, "a filter size one ulp away"); }
    { KdImageParams q = kIcp; q.local_size[0] = 9; q.max_clouds[0] = 9; CHECK(check(good, nb, q) == FLS_ERR_INVALID, "another local_map_size"); }
    { KdImageParams q = kIcp; q.point_search_thres = 2.0; CHECK(check(good, nb, q) == FLS_ERR_INVALID, "another point_search_thres"); }
    CHECK(check(good, nb, kd_image_params(FLS_ICP_OPTIMIZED, icp_params(1))) == FLS_ERR_INVALID, "a mapping image into a localization handle");
    { fls_kd_image_header h = header_of(good); h.is_localization_mode = 1; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "a localization image into a mapping handle"); }
    { fls_kd_image_header h = header_of(good); h.is_localization_mode = 1;
      CHECK(check(with_header(good, h), nb, kd_image_params(FLS_ICP_OPTIMIZED, icp_params(1))) == FLS_ERR_INVALID, "six clouds in a localization image"); }
    { KdImageParams q = kIcp; q.max_clouds[0] = 5; CHECK(check(good, nb, q) == FLS_ERR_INVALID, "six clouds where the deque holds five"); }
    { KdImageParams q = kIcp; q.max_clouds[0] = 6; CHECK(check(good, nb, q) == FLS_OK, "six clouds where the deque holds six"); }
    { fls_kd_image_header h = header_of(good); h.gate_init = 2; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "gate init 2"); }
    { fls_kd_image_header h = header_of(good); h.gate_last_T[5] = std::nan(""); CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "NaN in last_T"); }
    { fls_kd_image_header h = header_of(good); h.gate_last_T[15] = -INFINITY; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "infinity in last_T"); }
    { fls_kd_image_header h = header_of(good); h.gate_init = 0; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "a last_T while init is 0"); }
    { fls_kd_image_header h = header_of(good); h.gate_init = 0; std::memset(h.gate_last_T, 0, sizeof(h.gate_last_T)); CHECK(check(with_header(good, h), nb) == FLS_OK, "an unset gate");
      h.gate_last_T[3] = -0.0; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "a negative zero in an unset gate's last_T"); }
    { fls_kd_image_header h = header_of(good); h.reserved = 1; CHECK(check(with_header(good, h), nb) == FLS_ERR_INVALID, "reserved word set"); }
    // ---- the arrays: six sizes leave 8 bytes of padding in front of the rows ----
    CHECK(L0.rows[0] - (L0.sizes[0] + 4 * L0.n_clouds[0]) == 8, "the scenario has no padding to spoil");
    for (size_t i = L0.sizes[0] + 4 * L0.n_clouds[0]; i < L0.rows[0]; ++i) { std::vector<unsigned char> b = good; b[i] = 1; CHECK(check(b, nb) == FLS_ERR_INVALID, "padding byte %zu set", i); }
    { std::vector<unsigned char> b = good; uint32_t s; std::memcpy(&s, b.data() + L0.sizes[0] + 20, 4); ++s; std::memcpy(b.data() + L0.sizes[0] + 20, &s, 4);
      CHECK(check(b, nb) == FLS_ERR_INVALID, "sizes sum to one more than n_points"); }
    { std::vector<unsigned char> b = good; uint32_t a, c; std::memcpy(&a, b.data() + L0.sizes[0] + 16, 4); std::memcpy(&c, b.data() + L0.sizes[0] + 20, 4); a += 1; c -= 1;
      std::memcpy(b.data() + L0.sizes[0] + 16, &a, 4); std::memcpy(b.data() + L0.sizes[0] + 20, &c, 4);
      CHECK(check(b, nb) == FLS_OK, "one point moved between two clouds is another valid deque"); }
    { std::vector<unsigned char> b = good; for (size_t i = L0.rows[0]; i < nb; ++i) b[i] = 0xff; CHECK(check(b, nb) == FLS_OK, "point values are not checked"); }
    // ---- header only ----
    {
        KdDeque e0, e1;
        const KdDeque* none[2] = {&e0, &e1};
        for (const KdImageParams* q : {&kIcp, &kLoam, &kKd}) {
            KdImageLayout L;
            const std::vector<unsigned char> b = export_deques(*q, KdImageGate(), none, L);
            CHECK(b.size() == 224 && check(b, 224, *q) == FLS_OK && header_of(b).n_clouds[0] == 0 && header_of(b).gate_init == 0, "the image of a handle without a cloud is its header");
            KdDeque back;
            back.push_back(std::vector<PtI>(3));
            kd_deque_from_image(b.data(), L, 0, back);
            CHECK(back.empty(), "an empty image gives an empty deque");
        }
        CHECK(header_of(export_deques(kKd, KdImageGate(), none, L0)).point_search_thres_bits == 0, "P2PlaneKd carries no search gate");
    }
    // ---- deque -> bytes -> deque ----
    int two_maps = 0;
    for (int round = 0; round < 200; ++round) {
        const bool two = (round % 3) == 2;
        const KdImageParams& q = two ? kLoam : (round & 1) ? kKd : kIcp;
        two_maps += two;
        KdDeque a0, a1, b0, b1;
        random_deque(rng, a0, round < 3 ? round : std::uniform_int_distribution<int>(0, 8)(rng));
        if (two) random_deque(rng, a1, std::uniform_int_distribution<int>(0, 6)(rng));
        const KdDeque* maps[2] = {&a0, two ? &a1 : nullptr};
        const KdImageGate g = some_gate(rng, (round & 2) != 0);
        KdImageLayout L;
        const std::vector<unsigned char> img = export_deques(q, g, maps, L);
        fls_kd_image_header h;
        KdImageLayout Lc;
        CHECK(kd_image_check_header(img.data(), img.size(), q, h, Lc) == FLS_OK && kd_image_check_body(img.data(), Lc) == FLS_OK, "round %d: own image refused", round);
        CHECK(Lc.total == img.size() && Lc.total == L.total && Lc.rows[0] == L.rows[0] && Lc.sizes[1] == L.sizes[1] && Lc.rows[1] == L.rows[1], "round %d: layouts", round);
        CHECK(h.n_clouds[0] == a0.size() && h.n_clouds[1] == a1.size() && h.n_maps == (two ? 2u : 1u), "round %d: header counts", round);
        for (int m = 0; m < L.n_maps; ++m) {
            CHECK(L.sizes[m] % 16 == 0 && L.rows[m] % 16 == 0, "round %d: map %d placed at %zu / %zu", round, m, L.sizes[m], L.rows[m]);
            const KdDeque& src = m ? a1 : a0;
            size_t at = L.rows[m];
            for (size_t c = 0; c < src.size(); ++c) {  // oldest first, rows back to back, bit for bit
                uint32_t s;
                std::memcpy(&s, img.data() + L.sizes[m] + 4 * c, 4);
                CHECK(s == src[c].size(), "round %d: map %d cloud %zu holds %u", round, m, c, s);
                CHECK(src[c].empty() || std::memcmp(img.data() + at, src[c].data(), src[c].size() * 16) == 0, "round %d: map %d cloud %zu rows", round, m, c);
                at += src[c].size() * 16;
            }
            CHECK(at == (m + 1 < L.n_maps ? L.sizes[m + 1] : L.total), "round %d: map %d ends at %zu", round, m, at);
        }
        kd_deque_from_image(img.data(), Lc, 0, b0);
        if (two) kd_deque_from_image(img.data(), Lc, 1, b1);
        CHECK(same_deque(a0, b0) && same_deque(a1, b1), "round %d: the deques differ", round);
        const KdImageGate gb = kd_gate_from_header(h);
        CHECK(gb.init == g.init && std::memcmp(gb.last_T, g.last_T, sizeof(g.last_T)) == 0, "round %d: the gate differs", round);
        const KdDeque* back[2] = {&b0, two ? &b1 : nullptr};
        KdImageLayout L2;
        CHECK(export_deques(q, gb, back, L2) == img, "round %d: export(import(x)) != x", round);
        // the device export's two pieces (header + sizes from the host) are the image's own bytes
        std::vector<unsigned char> meta(L.rows[0] + (two ? L.rows[1] - L.sizes[1] : 0), 0xCD);
        unsigned char* const chunk[2] = {meta.data(), meta.data() + L.rows[0]};
        kd_image_write_meta(q, g, L, maps, chunk);
        CHECK(std::memcmp(meta.data(), img.data(), L.rows[0]) == 0 && (!two || std::memcmp(chunk[1], img.data() + L.sizes[1], L.rows[1] - L.sizes[1]) == 0), "round %d: meta pieces", round);
    }
    CHECK(g_nan > 100 && g_negzero > 100 && g_empty > 50 && two_maps > 50, "the random deques missed a case: %d %d %d %d", g_nan, g_negzero, g_empty, two_maps);
    std::printf("kd image model: 200 random deques (%d NaN payloads, %d negative zeros, %d empty clouds, %d images of two maps), mismatches %d\n", g_nan, g_negzero,
                g_empty, two_maps, g_fail);
    return g_fail ? 1 : 0;
}
