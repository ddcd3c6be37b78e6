// The host optimisers of the loop-closure matcher (csrc/loop_optim.hpp) without a device, held against the oracle (oracle/flo_loop.h): the 6x6
// Jacobi SVD solve on seeded systems, the NDT Newton loop with its More-Thuente line search driven by the oracle's derivatives, and the BFGS of
// GICP driven by the oracle's cost function -- each on the sums the oracle itself sees, so every count, pose and solution must equal the
// oracle's bit for bit.  Built by tests/test_loop_optim_model.py with hipcc (the product headers include the HIP headers; no HIP runtime call is
// made), once plain and once with AddressSanitizer and UBSan on the host side.  Arguments: source and target cloud, raw float32 x y z rows.
#include "../../funny_lidar_slam_amd/csrc/loop_optim.hpp"
#include "../../oracle/flo_loop.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

using namespace fls;
namespace fo = flo::loop;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static bool same_bits(const void* a, const void* b, size_t bytes) { return std::memcmp(a, b, bytes) == 0; }
static fo::M4f to_oracle(const LoopMat4f& t) { fo::M4f r; std::memcpy(r.m, t.m, sizeof(r.m)); return r; }
static LoopMat4f to_product(const fo::M4f& t) { LoopMat4f r; std::memcpy(r.m, t.m, sizeof(r.m)); return r; }

static flo::Cloud read_cloud(const char* path) {
    flo::Cloud c;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return c;
    float p[3];
    while (std::fread(p, sizeof(float), 3, f) == 3) c.push_back(flo::P4{p[0], p[1], p[2], 0.f});
    std::fclose(f);
    return c;
}

// translation (m) and rotation (rad) between two poses
static void pose_error(const fo::M4f& a, const fo::M4f& b, double& dt, double& dr) {
    double d2 = 0.0, f2 = 0.0;
    for (int i = 0; i < 3; ++i) { const double d = double(a.m[12 + i]) - double(b.m[12 + i]); d2 += d * d; }
    for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) { const double d = double(a.m[k + 4 * i]) - double(b.m[k + 4 * i]); f2 += d * d; }
    dt = std::sqrt(d2);
    dr = 2.0 * std::asin(std::min(1.0, std::sqrt(f2 / 8.0)));  // |Ra - Rb|_F = 2 sqrt(2) sin(angle / 2): well conditioned at 0, unlike the trace
}

// ---- svd_solve6 == jacobi_svd_solve<6> -------------------------------------------------------------------------------------------------
static int check_solve(const double* A, const double* b, const char* what, int k) {
    double xp[6], xo[6];
    loop::svd_solve6(A, b, xp);
    fo::jacobi_svd_solve<6>(A, b, xo);
    const bool same = same_bits(xp, xo, sizeof(xp));
    CHECK(same, "svd_solve6 %s %d: %.17g %.17g %.17g .. against %.17g %.17g %.17g ..", what, k, xp[0], xp[1], xp[2], xo[0], xo[1], xo[2]);
    return same ? 1 : 0;
}
static void test_svd_solve6() {
    std::mt19937_64 rng(20240607);
    std::normal_distribution<double> nd(0.0, 1.0);
    int same = 0, total = 0;
    for (int k = 0; k < 200; ++k) {
        double B[36], spd[36], indef[36], b[6];
        const double scale = std::pow(10.0, double(k % 9) - 4.0);
        for (double& v : B) v = nd(rng) * scale;
        for (double& v : b) v = nd(rng);
        for (int j = 0; j < 6; ++j)
            for (int i = 0; i < 6; ++i) {
                double s = 0.0;
                for (int q = 0; q < 6; ++q) s += B[q + 6 * i] * B[q + 6 * j];
                spd[i + 6 * j] = s;                           // B^T B
                indef[i + 6 * j] = B[i + 6 * j] + B[j + 6 * i];  // symmetric, eigenvalues of both signs
            }
        same += check_solve(spd, b, "SPD", k); same += check_solve(indef, b, "indefinite", k);
        total += 2;
    }
    {   // rank 2: the singular-value threshold drops four directions
        double A[36], b[6] = {1.0, -2.0, 0.5, 3.0, -1.0, 0.25};
        const double u[6] = {1, 2, -1, 0.5, 3, -2}, v[6] = {-1, 0.5, 2, 1, 0, 4};
        for (int j = 0; j < 6; ++j) for (int i = 0; i < 6; ++i) A[i + 6 * j] = u[i] * u[j] + v[i] * v[j];
        same += check_solve(A, b, "rank-deficient", 0);
        double xp[6];
        loop::svd_solve6(A, b, xp);
        double r = 0.0;  // (the minimum-norm solution lies in span{u, v}: it was not solved as a full-rank system)
        for (int i = 0; i < 6; ++i) r = std::max(r, std::fabs(xp[i]));
        CHECK(r < 1e3, "rank-deficient: |x| = %g", r);
        const double Z[36] = {0}, x0[6] = {0, 0, 0, 0, 0, 0};
        same += check_solve(Z, b, "zero", 0);
        loop::svd_solve6(Z, b, xp);
        CHECK(same_bits(xp, x0, sizeof(xp)), "zero matrix: x != 0");
        total += 2;
    }
    std::printf("svd_solve6: %d of %d systems equal bit for bit\n", same, total);
}

// ---- ndt_align on the oracle's derivatives == Ndt::align -------------------------------------------------------------------------------
static void test_ndt(const flo::Cloud& source, const flo::Cloud& target, const float resolution, fo::M4f& pose) {
    const flo::Cloud src = flo::voxel_grid(source, resolution * 0.2f), tgt = flo::voxel_grid(target, resolution * 0.2f);
    fo::Ndt ref;
    ref.step_size = 0.5; ref.max_iterations = 30; ref.resolution = resolution;
    ref.set_target(tgt);
    const fo::M4f fin_o = ref.align(src, pose);

    fo::Ndt ev;  // the evaluator: the oracle's sums at the poses the product's optimiser asks for
    ev.resolution = resolution;
    ev.set_target(tgt);
    ev.source = &src;
    loop::NdtRun run;
    run.resolution = resolution;
    int evaluations = 0, iterations = 0;
    double score = 0.0;
    const auto eval = [&](const LoopMat4f& T, const double* p, bool hessian, double* grad, double* hess) {
        ++evaluations;
        ev.gauss_d1 = run.pose.gauss_d1; ev.gauss_d2 = run.pose.gauss_d2;
        return ev.derivatives(grad, hess, to_oracle(T), p, hessian);
    };
    const fo::M4f fin_p = to_oracle(loop::ndt_align(run, eval, ev.cells.ok, src.size(), to_product(pose), iterations, score));

    double dt, dr;
    pose_error(fin_p, fin_o, dt, dr);
    const bool bits = same_bits(fin_p.m, fin_o.m, sizeof(fin_o.m)) && same_bits(&score, &ref.stats.score, sizeof(double));
    std::printf("ndt %g m: %zu source points, %zu leaves, oracle %d iterations / %d evaluations, product %d / %d, pose apart %.3g m %.3g rad, %s\n", double(resolution),
                src.size(), ref.cells.searchable.size(), ref.stats.iterations, ref.stats.evaluations, iterations, evaluations, dt, dr, bits ? "equal bits" : "bits differ");
    CHECK(ref.stats.iterations > 0, "ndt %g: the oracle did not iterate", double(resolution));
    CHECK(iterations == ref.stats.iterations && evaluations == ref.stats.evaluations, "ndt %g: counts", double(resolution));
    CHECK(dt <= 1e-4 && dr <= 1e-4, "ndt %g: pose %g m %g rad", double(resolution), dt, dr);
    CHECK(bits, "ndt %g: pose or score differ in bits", double(resolution));
    CHECK(same_bits(&run.pose.gauss_d1, &ref.gauss_d1, sizeof(double)) && same_bits(&run.pose.gauss_d2, &ref.gauss_d2, sizeof(double)), "ndt %g: Gauss constants", double(resolution));
    pose = fin_o;
}

// ---- gicp_estimate / Bfgs on the oracle's cost == Gicp::estimate -----------------------------------------------------------------------
// Gicp::align's outer loop (flo_loop.h) around `estimate(gicp, transformation)`; `each`: called with the state every estimate starts from
template <class Est, class Each>
static fo::M4f gicp_outer(fo::Gicp& g, const flo::Cloud& src, const flo::Cloud& tgt, const fo::M4f& guess, Est&& estimate, Each&& each) {
    g.stats = fo::GicpStats();
    g.target = &tgt;
    g.tgt_tree.Build(&tgt[0].x, tgt.size(), 4);
    fo::Gicp::covariances(tgt, g.k_correspondences, g.gicp_epsilon, g.cov_tgt);
    fo::Gicp::covariances(src, g.k_correspondences, g.gicp_epsilon, g.cov_src);
    const size_t N = src.size();
    g.mahal.assign(N * 9, 0.0);
    for (size_t i = 0; i < N; ++i) g.mahal[9 * i] = g.mahal[9 * i + 4] = g.mahal[9 * i + 8] = 1.0;
    g.moved.resize(N);
    for (size_t i = 0; i < N; ++i) { float o[3]; fo::xform_pt(guess, src[i].x, src[i].y, src[i].z, o); g.moved[i] = flo::P4{o[0], o[1], o[2], src[i].i}; }
    fo::M4f transformation = fo::m4f_identity(), previous = fo::m4f_identity();
    const double dist_threshold = g.corr_dist_threshold * g.corr_dist_threshold;
    int nr = 0;
    for (bool converged = false; !converged;) {
        g.idx_src.clear(); g.idx_tgt.clear();
        double R[9];
        for (int j = 0; j < 3; ++j)
            for (int i = 0; i < 3; ++i) {
                double s = 0.0;
                for (int k = 0; k < 4; ++k) s += double(transformation.m[i + 4 * k]) * double(guess.m[k + 4 * j]);
                R[i + 3 * j] = s;
            }
        for (size_t i = 0; i < N; ++i) {
            float q[3];
            fo::xform_pt(transformation, g.moved[i].x, g.moved[i].y, g.moved[i].z, q);
            flo::KdTree::Hit h;
            if (g.tgt_tree.Knn(q, 1, &h) != 1 || !(double(h.d2) < dist_threshold)) continue;
            double M1[9], Rt[9], tmp[9];
            flo::mat3_mul(R, &g.cov_src[9 * i], M1);
            for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) Rt[r + 3 * c] = R[c + 3 * r];
            flo::mat3_mul(M1, Rt, tmp);
            for (int q9 = 0; q9 < 9; ++q9) tmp[q9] += g.cov_tgt[9 * size_t(h.idx) + q9];
            flo::inverse3(tmp, &g.mahal[9 * i]);
            g.idx_src.push_back(int(i));
            g.idx_tgt.push_back(h.idx);
        }
        g.stats.correspondences = int(g.idx_src.size());
        previous = transformation;
        each(transformation, nr);
        if (!estimate(g, transformation)) { g.stats.failed = true; break; }
        double delta = 0.0;
        for (int k = 0; k < 4; ++k)
            for (int l = 0; l < 4; ++l) {
                const double ratio = (k < 3 && l < 3) ? 1.0 / g.rotation_epsilon : 1.0 / g.transformation_epsilon;
                delta = std::max(delta, ratio * std::fabs(double(previous.m[k + 4 * l]) - double(transformation.m[k + 4 * l])));
            }
        ++nr;
        if (nr >= g.max_iterations || delta < 1) { converged = true; previous = transformation; }
    }
    g.stats.iterations = nr;
    return fo::m4f_mul(previous, guess);
}

static bool product_estimate(fo::Gicp& g, fo::M4f& transformation) {
    LoopMat4f t = to_product(transformation);
    const auto fdf = [&](const double* x, double* f, double* grad) { g.fdf(x, f, grad); };
    const bool ok = loop::gicp_estimate(int(g.idx_src.size()), t, fdf, g.stats.inner_total);
    transformation = to_oracle(t);
    return ok;
}

static void test_gicp(const flo::Cloud& source, const flo::Cloud& target, const fo::M4f& guess) {
    const flo::Cloud src = flo::voxel_grid(source, 0.5f), tgt = flo::voxel_grid(target, 0.4f);
    CHECK(src.size() >= 20 && tgt.size() >= 20, "gicp: %zu / %zu points", src.size(), tgt.size());
    if (src.size() < 20 || tgt.size() < 20) return;
    // the oracle's run; on the way, the product's estimate from the same state on the same correspondences, every outer iteration
    fo::Gicp ref;
    ref.max_iterations = 30; ref.corr_dist_threshold = 2.0;
    int steps = 0, steps_equal = 0;
    const fo::M4f fin_o = gicp_outer(ref, src, tgt, guess, [](fo::Gicp& g, fo::M4f& t) { return g.estimate(t); }, [&](const fo::M4f& start, int nr) {
        fo::Gicp side = ref;  // (a copy: the oracle's counters stay its own)
        side.stats = fo::GicpStats();
        fo::M4f tp = start, to = start;
        const bool okp = product_estimate(side, tp);
        const int inner_p = side.stats.inner_total, evals_p = side.stats.evaluations;
        side.stats = fo::GicpStats();
        const bool oko = side.estimate(to);
        const bool same = okp == oko && inner_p == side.stats.inner_total && evals_p == side.stats.evaluations && same_bits(tp.m, to.m, sizeof(to.m));
        CHECK(same, "gicp estimate, outer iteration %d: product %d inner / %d evaluations ok %d, oracle %d / %d ok %d", nr, inner_p, evals_p, int(okp), side.stats.inner_total,
              side.stats.evaluations, int(oko));
        ++steps;
        steps_equal += same ? 1 : 0;
    });
    const fo::GicpStats so = ref.stats;
    {   // the oracle's own align is what gicp_outer restates
        fo::Gicp own;
        own.max_iterations = 30; own.corr_dist_threshold = 2.0;
        const fo::M4f fin = own.align(src, tgt, guess);
        CHECK(same_bits(fin.m, fin_o.m, sizeof(fin.m)) && own.stats.iterations == so.iterations && own.stats.inner_total == so.inner_total && own.stats.evaluations == so.evaluations,
              "gicp: the restated outer loop is not Gicp::align");
    }
    // the whole alignment on the product's estimate
    fo::Gicp prod;
    prod.max_iterations = 30; prod.corr_dist_threshold = 2.0;
    const fo::M4f fin_p = gicp_outer(prod, src, tgt, guess, product_estimate, [](const fo::M4f&, int) {});
    const fo::GicpStats sp = prod.stats;
    double dt, dr;
    pose_error(fin_p, fin_o, dt, dr);
    const bool same_trace = sp.iterations == so.iterations && sp.inner_total == so.inner_total;
    const bool bits = same_bits(fin_p.m, fin_o.m, sizeof(fin_o.m));
    std::printf("gicp: %zu / %zu points, oracle %d outer / %d inner / %d evaluations / %d correspondences failed %d, product %d / %d / %d / %d failed %d, "
                "%d of %d estimates equal bit for bit, pose apart %.3g m %.3g rad, %s\n", src.size(), tgt.size(), so.iterations, so.inner_total, so.evaluations, so.correspondences,
                int(so.failed), sp.iterations, sp.inner_total, sp.evaluations, sp.correspondences, int(sp.failed), steps_equal, steps, dt, dr, bits ? "equal bits" : "bits differ");
    CHECK(!so.failed && so.iterations > 0, "gicp: the oracle failed");
    CHECK(sp.failed == so.failed && std::abs(sp.iterations - so.iterations) <= 2, "gicp: outer iterations %d against %d", sp.iterations, so.iterations);
    if (same_trace) CHECK(sp.correspondences == so.correspondences, "gicp: correspondences %d against %d", sp.correspondences, so.correspondences);
    CHECK(dt <= (same_trace ? 1e-4 : 2e-3) && dr <= (same_trace ? 1e-4 : 5e-4), "gicp: pose %g m %g rad, same trace %d", dt, dr, int(same_trace));
    CHECK(same_trace && bits && sp.evaluations == so.evaluations, "gicp: trace, evaluations or pose differ from the oracle's");
}

int main(int argc, char** argv) {
    if (argc != 3) { std::printf("usage: %s source.f32 target.f32\n", argv[0]); return 2; }
    const flo::Cloud source = read_cloud(argv[1]), target = read_cloud(argv[2]);
    if (source.empty() || target.empty()) { std::printf("no points read\n"); return 2; }
    test_svd_solve6();
    fo::M4f pose = fo::m4f_identity();
    test_ndt(source, target, 10.0f, pose);
    test_ndt(source, target, 2.0f, pose);
    test_gicp(source, target, pose);
    std::printf("loop optimisers: %d failures\n", g_fail);
    return g_fail ? 1 : 0;
}
