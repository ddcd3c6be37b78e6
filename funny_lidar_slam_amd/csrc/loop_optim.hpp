// loop_optim.hpp -- the host arithmetic of the loop-closure matcher that owns no device state: the float pose algebra, the leaf Gaussian
// of VoxelGridCovariance, P2D-NDT's Newton loop with its 6x6 SVD solve and More-Thuente line search, and GICP's BFGS (algorithms and
// parameters: the head of loop_closure.hpp).  Plain functions and small structs; the two optimisers take their objective as a callable,
// which LoopMatcher binds to its device sums (ndt_eval, gicp_fdf) and tests/host/loop_optim_test.cpp to the oracle's.  No HIP runtime call.
#pragma once
#include "host_math.hpp"
#include "loop_types.hpp"

namespace fls {
namespace loop {

// ---- float pose algebra (Eigen::Transform<float, 3, Affine>) ------------------------------------------------------------
inline LoopMat4f ident() { LoopMat4f r{}; r.m[0] = r.m[5] = r.m[10] = r.m[15] = 1.f; return r; }
inline LoopMat4f mul(const LoopMat4f& a, const LoopMat4f& b) {
    LoopMat4f r;
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i)
            r.m[i + 4 * j] = ((a.m[i] * b.m[4 * j] + a.m[i + 4] * b.m[1 + 4 * j]) + a.m[i + 8] * b.m[2 + 4 * j]) + a.m[i + 12] * b.m[3 + 4 * j];
    return r;
}
inline LoopMat4f rot(int axis, float angle) {  // AngleAxisf(angle, unit axis)
    LoopMat4f r = ident();
    const float c = std::cos(angle), s = std::sin(angle);
    const int a = (axis + 1) % 3, b = (axis + 2) % 3;
    r.m[a + 4 * a] = c; r.m[b + 4 * b] = c; r.m[b + 4 * a] = s; r.m[a + 4 * b] = -s;
    return r;
}
inline LoopMat4f trans(float x, float y, float z) { LoopMat4f r = ident(); r.m[12] = x; r.m[13] = y; r.m[14] = z; return r; }
inline LoopMat4f from_d(const double* T) { LoopMat4f r; for (int i = 0; i < 16; ++i) r.m[i] = float(T[i]); return r; }
// (Translation(p0..2) * AngleAxis(p3, X) * AngleAxis(p4, Y) * AngleAxis(p5, Z)).matrix()   ndt.hpp computeStepLengthMT
inline LoopMat4f pose_xyz(const double* p) {
    return mul(mul(mul(trans(float(p[0]), float(p[1]), float(p[2])), rot(0, float(p[3]))), rot(1, float(p[4]))), rot(2, float(p[5])));
}
// Matrix3f::eulerAngles(0, 1, 2) (Eigen 3.3 EulerAngles.h)
inline void euler012(const LoopMat4f& t, float (&e)[3]) {
    auto at = [&](int i, int j) { return t.m[i + 4 * j]; };
    const float pi = 3.14159265358979323846f;
    e[0] = std::atan2(at(1, 2), at(2, 2));
    const float c2 = std::sqrt(at(0, 0) * at(0, 0) + at(0, 1) * at(0, 1));
    if (e[0] > 0.f) { e[0] -= pi; e[1] = std::atan2(-at(0, 2), -c2); }
    else e[1] = std::atan2(-at(0, 2), c2);
    const float s1 = std::sin(e[0]), c1 = std::cos(e[0]);
    e[2] = std::atan2(s1 * at(2, 0) - c1 * at(1, 0), c1 * at(1, 1) - s1 * at(2, 1));
    e[0] = -e[0]; e[1] = -e[1]; e[2] = -e[2];
}

// ---- leaf Gaussians of VoxelGridCovariance --------------------------------------------------------------------------------
// symmetric 3x3 eigen-decomposition, ascending (SelfAdjointEigenSolver stand-in: Jacobi via hm::svd3)
__host__ __device__ inline void sym_eig3(const double* A, double* ev, double* evec) {
    double U[9], S[3], V[9];
    hm::svd3(A, U, S, V);
    for (int k = 0; k < 3; ++k) {
        const double sgn = (U[3 * k] * V[3 * k] + U[3 * k + 1] * V[3 * k + 1]) + U[3 * k + 2] * V[3 * k + 2];
        const int dst = 2 - k;
        ev[dst] = sgn < 0.0 ? -S[k] : S[k];
        for (int i = 0; i < 3; ++i) evec[i + 3 * dst] = V[i + 3 * k];
    }
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b)
            if (ev[b] < ev[a]) {
                { const double t = ev[a]; ev[a] = ev[b]; ev[b] = t; }
                for (int i = 0; i < 3; ++i) { const double t = evec[i + 3 * a]; evec[i + 3 * a] = evec[i + 3 * b]; evec[i + 3 * b] = t; }
            }
}
// The Gaussian of a leaf of n >= 6 points from its sums (VoxelGridCovariance::applyFilter): the mean, the covariance with the 0.01 * ev[2]
// eigenvalue floor, its inverse -- zero for a leaf with a negative eigenvalue, which stays searchable as in PCL.  One function for
// build_target and the device build (kernels_loop_leaves.hpp): the same IEEE operation sequence on both sides (-ffp-contract=off).
__host__ __device__ inline void leaf_gaussian(const int n, const double* sum, const double* xx, double* mean, double* icov) {
    double cov[9];
    for (int a = 0; a < 9; ++a) icov[a] = 0.0;
    for (int a = 0; a < 3; ++a) mean[a] = sum[a] / n;
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) cov[r + 3 * c] = (xx[r + 3 * c] - 2.0 * (sum[r] * mean[c])) / n + mean[r] * mean[c];
    for (int i = 0; i < 9; ++i) cov[i] *= (n - 1.0) / n;
    double ev[3], evec[9];
    sym_eig3(cov, ev, evec);
    if (ev[0] < 0 || ev[1] < 0 || ev[2] <= 0) return;
    const double floor_ev = 0.01 * ev[2];
    if (ev[0] < floor_ev) {
        ev[0] = floor_ev;
        if (ev[1] < floor_ev) ev[1] = floor_ev;
        double vinv[9], tmp[9];
        hm::inv3(evec, vinv);
        for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) tmp[r + 3 * c] = evec[r + 3 * c] * ev[c];
        hm::mul3(tmp, vinv, cov);
    }
    hm::inv3(cov, icov);
}

// ---- NormalDistributionsTransform ------------------------------------------------------------------------------------------
struct NdtRun {  // one align: the reference's parameters, and what the evaluator reads (pose) and ndt_align leaves (final_transformation)
    float resolution = 1.f;
    double step_size = 0.5, outlier_ratio = 0.55, transformation_epsilon = 0.1;
    int max_iterations = 30;
    NdtP2dPose pose{};
    LoopMat4f final_transformation{};
};
// the Gauss constants d1, d2 of a resolution (Magnusson eq. 6.8; ndt.hpp init) -> r.pose
inline void ndt_gauss(NdtRun& r) {
    const double c1 = 10.0 * (1.0 - r.outlier_ratio), c2 = r.outlier_ratio / std::pow(double(r.resolution), 3), d3 = -std::log(c2);
    r.pose.gauss_d1 = -std::log(c1 + c2) - d3;
    r.pose.gauss_d2 = -2.0 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - d3) / r.pose.gauss_d1);
}

// computeAngleDerivatives: rows of d(Rx Ry Rz)/d(angle) and of the second derivatives (Magnusson eq. 6.19, 6.21)
inline void angle_derivatives(const double* p, NdtP2dPose& o) {
    double cx, cy, cz, sx, sy, sz;
    if (std::fabs(p[3]) < 10e-5) { cx = 1.0; sx = 0.0; } else { cx = std::cos(p[3]); sx = std::sin(p[3]); }
    if (std::fabs(p[4]) < 10e-5) { cy = 1.0; sy = 0.0; } else { cy = std::cos(p[4]); sy = std::sin(p[4]); }
    if (std::fabs(p[5]) < 10e-5) { cz = 1.0; sz = 0.0; } else { cz = std::cos(p[5]); sz = std::sin(p[5]); }
    const double J[8][3] = {{-sx * sz + cx * sy * cz, -sx * cz - cx * sy * sz, -cx * cy}, {cx * sz + sx * sy * cz, cx * cz - sx * sy * sz, -sx * cy},
                            {-sy * cz, sy * sz, cy}, {sx * cy * cz, -sx * cy * sz, sx * sy}, {-cx * cy * cz, cx * cy * sz, -cx * sy},
                            {-cy * sz, -cy * cz, 0.0}, {cx * cz - sx * sy * sz, -cx * sz - sx * sy * cz, 0.0}, {sx * cz + cx * sy * sz, cx * sy * cz - sx * sz, 0.0}};
    const double H[15][3] = {{-cx * sz - sx * sy * cz, -cx * cz + sx * sy * sz, sx * cy}, {-sx * sz + cx * sy * cz, -cx * sy * sz - sx * cz, -cx * cy},
                             {cx * cy * cz, -cx * cy * sz, cx * sy}, {sx * cy * cz, -sx * cy * sz, sx * sy},
                             {-sx * cz - cx * sy * sz, sx * sz - cx * sy * cz, 0.0}, {cx * cz - sx * sy * sz, -sx * sy * cz - cx * sz, 0.0},
                             {-cy * cz, cy * sz, -sy}, {-sx * sy * cz, sx * sy * sz, sx * cy}, {cx * sy * cz, -cx * sy * sz, -cx * cy},
                             {sy * sz, sy * cz, 0.0}, {-sx * cy * sz, -sx * cy * cz, 0.0}, {cx * cy * sz, cx * cy * cz, 0.0},
                             {-cy * cz, cy * sz, 0.0}, {-cx * sz - sx * sy * cz, -cx * cz + sx * sy * sz, 0.0}, {-sx * sz + cx * sy * cz, -cx * sy * sz - sx * cz, 0.0}};
    std::memcpy(o.j_ang, J, sizeof(J));
    std::memcpy(o.h_ang, H, sizeof(H));
}

// JacobiSVD<Matrix6d>(A, ComputeFullU | ComputeFullV).solve(b)
inline void svd_solve6(const double* A, const double* b, double* x) {
    constexpr int N = 6;
    const double precision = 2.0 * std::numeric_limits<double>::epsilon(), tiny = std::numeric_limits<double>::min();
    double scale = 0.0;
    for (int i = 0; i < N * N; ++i) scale = std::max(scale, std::fabs(A[i]));
    if (scale == 0.0) scale = 1.0;
    double W[N * N], U[N * N], V[N * N];
    for (int i = 0; i < N * N; ++i) { W[i] = A[i] / scale; U[i] = V[i] = (i % (N + 1) == 0) ? 1.0 : 0.0; }
    double max_diag = 0.0;
    for (int i = 0; i < N; ++i) max_diag = std::max(max_diag, std::fabs(W[i + N * i]));
    auto jacobi = [&](double x_, double y_, double z_, double& c, double& s) {
        const double deno = 2.0 * std::fabs(y_);
        if (deno < tiny) { c = 1.0; s = 0.0; return; }
        const double tau = (x_ - z_) / deno, w = std::sqrt(tau * tau + 1.0);
        const double t = tau > 0.0 ? 1.0 / (tau + w) : 1.0 / (tau - w);
        const double sign_t = t > 0.0 ? 1.0 : -1.0, nn = 1.0 / std::sqrt(t * t + 1.0);
        s = -sign_t * (y_ / std::fabs(y_)) * std::fabs(t) * nn;
        c = nn;
    };
    bool finished = false;
    for (int sweep = 0; !finished && sweep < 1000; ++sweep) {
        finished = true;
        for (int p = 1; p < N; ++p)
            for (int q = 0; q < p; ++q) {
                const double threshold = std::max(tiny, precision * max_diag);
                if (!(std::fabs(W[p + q * N]) > threshold || std::fabs(W[q + p * N]) > threshold)) continue;
                finished = false;
                const double m00 = W[p + p * N], m01 = W[p + q * N], m10 = W[q + p * N], m11 = W[q + q * N];
                double r1c, r1s;
                const double t = m00 + m11, d = m10 - m01;
                if (std::fabs(d) < tiny) { r1s = 0.0; r1c = 1.0; }
                else { const double u = t / d, tmp = std::sqrt(1.0 + u * u); r1s = 1.0 / tmp; r1c = u / tmp; }
                const double n00 = r1c * m00 + r1s * m10, n01 = r1c * m01 + r1s * m11, n11 = -r1s * m01 + r1c * m11;
                double jc, js;
                jacobi(n00, n01, n11, jc, js);
                const double lc = r1c * jc - r1s * (-js), ls = r1c * (-js) + r1s * jc;  // j_left = rot1 * j_right^T
                for (int k = 0; k < N; ++k) {
                    const double xi = W[p + k * N], yi = W[q + k * N];
                    W[p + k * N] = lc * xi + ls * yi;
                    W[q + k * N] = -ls * xi + lc * yi;
                }
                for (int k = 0; k < N; ++k) {
                    const double xi = U[k + p * N], yi = U[k + q * N];
                    U[k + p * N] = lc * xi + ls * yi;
                    U[k + q * N] = -ls * xi + lc * yi;
                }
                for (int k = 0; k < N; ++k) {
                    double xi = W[k + p * N], yi = W[k + q * N];
                    W[k + p * N] = jc * xi - js * yi;
                    W[k + q * N] = js * xi + jc * yi;
                    xi = V[k + p * N]; yi = V[k + q * N];
                    V[k + p * N] = jc * xi - js * yi;
                    V[k + q * N] = js * xi + jc * yi;
                }
                max_diag = std::max(max_diag, std::max(std::fabs(W[p + p * N]), std::fabs(W[q + q * N])));
            }
    }
    double S[N], smax = 0.0;
    for (int i = 0; i < N; ++i) {
        const double a = W[i + i * N];
        S[i] = std::fabs(a) * scale;
        if (a < 0.0) for (int k = 0; k < N; ++k) U[k + i * N] = -U[k + i * N];
        smax = std::max(smax, S[i]);
    }
    const double thr = std::numeric_limits<double>::epsilon() * N * smax;
    for (int i = 0; i < N; ++i) x[i] = 0.0;
    for (int k = 0; k < N; ++k) {
        if (!(S[k] > thr)) continue;
        double ub = 0.0;
        for (int i = 0; i < N; ++i) ub += U[i + k * N] * b[i];
        const double c = ub / S[k];
        for (int i = 0; i < N; ++i) x[i] += V[i + k * N] * c;
    }
}

// More-Thuente pieces (ndt.hpp): psi, psi', interval update, trial value
inline double mt_psi(double a, double f_a, double f_0, double g_0, double mu) { return f_a - f_0 - mu * g_0 * a; }
inline double mt_dpsi(double g_a, double g_0, double mu) { return g_a - mu * g_0; }
struct MtEnd { double a, f, g; };
inline bool mt_update(MtEnd& l, MtEnd& u, const MtEnd& t) {
    if (t.f > l.f) { u = t; return false; }
    const double s = t.g * (l.a - t.a);
    if (s > 0) { l = t; return false; }
    if (s < 0) { u = l; l = t; return false; }
    return true;
}
inline double mt_cubic_min(const MtEnd& p, const MtEnd& q) {  // minimiser of the cubic through (p.a, p.f, p.g), (q.a, q.f, q.g)
    const double z = 3 * (q.f - p.f) / (q.a - p.a) - q.g - p.g, w = std::sqrt(z * z - q.g * p.g);
    return p.a + (q.a - p.a) * (w - p.g - z) / (q.g - p.g + 2 * w);
}
inline double mt_trial(const MtEnd& l, const MtEnd& u, const MtEnd& t) {
    if (t.f > l.f) {
        const double a_c = mt_cubic_min(l, t), a_q = l.a - 0.5 * (l.a - t.a) * l.g / (l.g - (l.f - t.f) / (l.a - t.a));
        return std::fabs(a_c - l.a) < std::fabs(a_q - l.a) ? a_c : 0.5 * (a_q + a_c);
    }
    if (t.g * l.g < 0) {
        const double a_c = mt_cubic_min(l, t), a_s = l.a - (l.a - t.a) / (l.g - t.g) * l.g;
        return std::fabs(a_c - t.a) >= std::fabs(a_s - t.a) ? a_c : a_s;
    }
    if (std::fabs(t.g) <= std::fabs(l.g)) {
        const double a_c = mt_cubic_min(l, t), a_s = l.a - (l.a - t.a) / (l.g - t.g) * l.g;
        const double nxt = std::fabs(a_c - t.a) < std::fabs(a_s - t.a) ? a_c : a_s;
        return t.a > l.a ? std::min(t.a + 0.66 * (u.a - t.a), nxt) : std::max(t.a + 0.66 * (u.a - t.a), nxt);
    }
    return mt_cubic_min(u, t);
}
inline double dot6(const double* a, const double* b) { double s = 0.0; for (int i = 0; i < 6; ++i) s += a[i] * b[i]; return s; }

// computeStepLengthMT.  eval(T, p, want_hessian, grad, hess) -> score: computeDerivatives (computeHessian where the gradient is unused) at
// the pose vector p, whose matrix is T
template <class Eval>
double step_length_mt(NdtRun& r, Eval&& eval, const double* x, double* dir, double step_init, double step_max, double step_min, double& score, double* grad, double* hess) {
    const double phi_0 = -score;
    double d_phi_0 = -dot6(grad, dir);
    if (d_phi_0 >= 0) {
        if (d_phi_0 == 0) return 0;
        d_phi_0 = -d_phi_0;
        for (int i = 0; i < 6; ++i) dir[i] = -dir[i];
    }
    const double mu = 1.e-4, nu = 0.9;
    MtEnd lo{0.0, mt_psi(0.0, phi_0, phi_0, d_phi_0, mu), mt_dpsi(d_phi_0, d_phi_0, mu)}, up = lo;
    bool interval_converged = (step_max - step_min) < 0, open_interval = true;
    int trials = 0;
    double a_t = std::max(std::min(step_init, step_max), step_min), x_t[6];
    auto evaluate = [&](bool with_hessian) {
        for (int i = 0; i < 6; ++i) x_t[i] = x[i] + dir[i] * a_t;
        r.final_transformation = pose_xyz(x_t);
        score = eval(r.final_transformation, x_t, with_hessian, grad, hess);
    };
    evaluate(true);
    double phi_t = -score, d_phi_t = -dot6(grad, dir);
    double psi_t = mt_psi(a_t, phi_t, phi_0, d_phi_0, mu), d_psi_t = mt_dpsi(d_phi_t, d_phi_0, mu);
    while (!interval_converged && trials < 10 && !(psi_t <= 0 && d_phi_t <= -nu * d_phi_0)) {
        a_t = open_interval ? mt_trial(lo, up, MtEnd{a_t, psi_t, d_psi_t}) : mt_trial(lo, up, MtEnd{a_t, phi_t, d_phi_t});
        a_t = std::max(std::min(a_t, step_max), step_min);
        evaluate(false);
        phi_t = -score;
        d_phi_t = -dot6(grad, dir);
        psi_t = mt_psi(a_t, phi_t, phi_0, d_phi_0, mu);
        d_psi_t = mt_dpsi(d_phi_t, d_phi_0, mu);
        if (open_interval && psi_t <= 0 && d_psi_t >= 0) {  // the interval is closed from here on: psi -> phi at both ends
            open_interval = false;
            lo.f = lo.f + phi_0 - mu * d_phi_0 * lo.a; lo.g = lo.g + mu * d_phi_0;
            up.f = up.f + phi_0 - mu * d_phi_0 * up.a; up.g = up.g + mu * d_phi_0;
        }
        interval_converged = open_interval ? mt_update(lo, up, MtEnd{a_t, psi_t, d_psi_t}) : mt_update(lo, up, MtEnd{a_t, phi_t, d_phi_t});
        ++trials;
    }
    if (trials) {  // computeHessian at the accepted point (score and gradient are current)
        double g_unused[6];
        eval(r.final_transformation, x_t, true, g_unused, hess);
    }
    return a_t;
}

// computeTransformation of n_src source points (0, or no target leaf: the guess comes back)
template <class Eval>
LoopMat4f ndt_align(NdtRun& r, Eval&& eval, const bool have_target, const size_t n_src, const LoopMat4f& guess, int& iterations, double& score_out) {
    ndt_gauss(r);
    r.final_transformation = guess;
    iterations = 0;
    score_out = 0.0;
    if (!have_target || n_src == 0) return r.final_transformation;
    float e[3];
    euler012(guess, e);
    double p[6] = {double(guess.m[12]), double(guess.m[13]), double(guess.m[14]), double(e[0]), double(e[1]), double(e[2])};
    double grad[6], hess[36], delta[6];
    double score = eval(r.final_transformation, p, true, grad, hess);
    for (bool converged = false; !converged;) {
        double neg[6];
        for (int i = 0; i < 6; ++i) neg[i] = -grad[i];
        svd_solve6(hess, neg, delta);
        double nrm = std::sqrt(dot6(delta, delta));
        if (nrm == 0 || nrm != nrm) break;
        for (int i = 0; i < 6; ++i) delta[i] /= nrm;
        nrm = step_length_mt(r, eval, p, delta, nrm, r.step_size, r.transformation_epsilon / 2, score, grad, hess);
        for (int i = 0; i < 6; ++i) { delta[i] *= nrm; p[i] += delta[i]; }
        if (iterations > r.max_iterations || (iterations && std::fabs(nrm) < r.transformation_epsilon)) converged = true;
        ++iterations;
    }
    score_out = score / double(n_src);
    return r.final_transformation;
}

// ---- GeneralizedIterativeClosestPoint --------------------------------------------------------------------------------------
inline void apply_state(LoopMat4f& t, const double* x) {  // gicp.hpp applyState: R = Rz(x5) Ry(x4) Rx(x3) on the left, translation added
    const LoopMat4f R = mul(mul(rot(2, float(x[5])), rot(1, float(x[4]))), rot(0, float(x[3])));
    LoopMat4f o = t;
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) o.m[i + 4 * j] = (R.m[i] * t.m[4 * j] + R.m[i + 4] * t.m[1 + 4 * j]) + R.m[i + 8] * t.m[2 + 4 * j];
    o.m[12] = t.m[12] + float(x[0]); o.m[13] = t.m[13] + float(x[1]); o.m[14] = t.m[14] + float(x[2]);
    t = o;
}
// computeRDerivative: derivatives of Rz(psi) Ry(theta) Rx(phi) at x[3..5]; g[3 + k] = trace(dR_k * Racc)
inline void gicp_rotation_gradient(const double* x, const double* Racc, double* grad) {
    const double cphi = std::cos(x[3]), sphi = std::sin(x[3]), cth = std::cos(x[4]), sth = std::sin(x[4]), cpsi = std::cos(x[5]), spsi = std::sin(x[5]);
    const double dphi[9] = {0.0, 0.0, 0.0,  // column 0
                            sphi * spsi + cphi * cpsi * sth, -cpsi * sphi + cphi * spsi * sth, cphi * cth,
                            cphi * spsi - cpsi * sphi * sth, -cphi * cpsi - sphi * spsi * sth, -cth * sphi};
    const double dth[9] = {-cpsi * sth, -spsi * sth, -cth, cpsi * cth * sphi, cth * sphi * spsi, -sphi * sth, cphi * cpsi * cth, cphi * cth * spsi, -cphi * sth};
    const double dpsi[9] = {-cth * spsi, cpsi * cth, 0.0, -cphi * cpsi - sphi * spsi * sth, -cphi * spsi + cpsi * sphi * sth, 0.0,
                            cpsi * sphi - cphi * spsi * sth, sphi * spsi + cphi * cpsi * sth, 0.0};
    auto tr = [&](const double* d) { double s = 0.0; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) s += d[j + 3 * i] * Racc[i + 3 * j]; return s; };
    grad[3] = tr(dphi); grad[4] = tr(dth); grad[5] = tr(dpsi);
}

// pcl/registration/bfgs.h = GSL vector_bfgs2: direction update + Fletcher's bracketing / sectioning line search with cached evaluations
// fdf(x, f*, grad*): the cost (and, with grad, its gradient) at x
template <class Fdf>
struct Bfgs {
    Fdf& fdf;
    double x0[6], g0[6], p[6], xa[6], ga[6], gradient[6];
    double f = 0, fa = 0, dfa = 0, g0norm = 0, pnorm = 0, fp0 = 0, delta_f = 0, kx = 0, kf = 0, kg = 0, kdf = 0;
    static double nrm(const double* v) { return std::sqrt(dot6(v, v)); }
    void move_to(double a) { if (a == kx) return; for (int i = 0; i < 6; ++i) xa[i] = x0[i] + a * p[i]; kx = a; }
    double eval_f(double a) { if (a == kf) return fa; move_to(a); fdf(xa, &fa, nullptr); kf = a; return fa; }
    double eval_df(double a) {
        if (a == kdf) return dfa;
        move_to(a);
        if (a != kg) { double ft; fdf(xa, &ft, ga); kg = a; }
        dfa = dot6(ga, p); kdf = a;
        return dfa;
    }
    void eval_fdf(double a, double& fv, double& dfv) {
        if (a == kf && a == kdf) { fv = fa; dfv = dfa; return; }
        if (a == kf || a == kdf) { fv = eval_f(a); dfv = eval_df(a); return; }
        move_to(a);
        fdf(xa, &fa, ga);
        kf = a; kg = a; dfa = dot6(ga, p); kdf = a;
        fv = fa; dfv = dfa;
    }
    void new_direction() { for (int i = 0; i < 6; ++i) { xa[i] = x0[i]; ga[i] = g0[i]; } kx = kf = kg = 0; dfa = dot6(ga, p); kdf = 0; }
    void start(const double* x) {
        delta_f = 0;
        fdf(x, &f, gradient);
        for (int i = 0; i < 6; ++i) { x0[i] = x[i]; g0[i] = gradient[i]; }
        g0norm = nrm(g0);
        for (int i = 0; i < 6; ++i) p[i] = gradient[i] * (-1.0 / g0norm);
        pnorm = nrm(p);
        fp0 = -g0norm;
        for (int i = 0; i < 6; ++i) { xa[i] = x0[i]; ga[i] = g0[i]; }
        kx = 0; fa = f; kf = 0; kg = 0; dfa = dot6(ga, p); kdf = 0;
    }
    static double poly3(double c0, double c1, double c2, double c3, double z) { return c0 + z * (c1 + z * (c2 + z * c3)); }
    static int quad_roots(double a, double b, double c, double& r0, double& r1) {  // gsl_poly_solve_quadratic
        const double disc = b * b - 4 * a * c;
        if (a == 0) { if (b == 0) return 0; r0 = -c / b; return 1; }
        if (disc > 0) {
            if (b == 0) { const double r = std::fabs(0.5 * std::sqrt(disc) / a); r0 = -r; r1 = r; }
            else { const double t = -0.5 * (b + (b > 0 ? 1.0 : -1.0) * std::sqrt(disc)), q1 = t / a, q2 = c / t; r0 = std::min(q1, q2); r1 = std::max(q1, q2); }
            return 2;
        }
        if (disc == 0) { r0 = r1 = -0.5 * b / a; return 2; }
        return 0;
    }
    static double min_quad(double f0, double d0, double f1, double zl, double zh) {
        const double k = f1 - f0 - d0, fl = f0 + zl * (d0 + zl * k), fh = f0 + zh * (d0 + zh * k), c = 2 * k;
        double zmin = zl, fmin = fl;
        if (fh < fmin) { zmin = zh; fmin = fh; }
        if (c > 0) { const double z = -d0 / c; if (z > zl && z < zh) { const double fz = f0 + z * (d0 + z * k); if (fz < fmin) { zmin = z; fmin = fz; } } }
        return zmin;
    }
    static double min_cubic(double f0, double d0, double f1, double d1, double zl, double zh) {
        const double c2 = 3 * (f1 - f0) - 2 * d0 - d1, c3 = d0 + d1 - 2 * (f1 - f0);
        double zmin = zl, fmin = poly3(f0, d0, c2, c3, zl), z0 = 0, z1 = 0;
        auto consider = [&](double z) { const double y = poly3(f0, d0, c2, c3, z); if (y < fmin) { zmin = z; fmin = y; } };
        consider(zh);
        const int n = quad_roots(3 * c3, 2 * c2, d0, z0, z1);
        if (n >= 1 && z0 > zl && z0 < zh) consider(z0);
        if (n == 2 && z1 > zl && z1 < zh) consider(z1);
        return zmin;
    }
    static double interpolate(double a, double fa_, double fpa, double b, double fb, double fpb, double xmin, double xmax) {
        double ymin = (xmin - a) / (b - a), ymax = (xmax - a) / (b - a);
        if (ymin > ymax) std::swap(ymin, ymax);
        const bool cubic_ok = !(fpb != fpb) && fpb != std::numeric_limits<double>::infinity();  // order 3
        const double y = cubic_ok ? min_cubic(fa_, fpa * (b - a), fb, fpb * (b - a), ymin, ymax) : min_quad(fa_, fpa * (b - a), fb, ymin, ymax);
        return a + y * (b - a);
    }
    // 0 = Success, 1 = NoProgress
    int line_search(double alpha1, double& alpha_new) {
        const double rho = 0.01, sigma = 0.01, tau1 = 9, tau2 = 0.05, tau3 = 0.5, nan = std::numeric_limits<double>::quiet_NaN();
        double f0v, fp0v;
        eval_fdf(0.0, f0v, fp0v);
        double alpha = alpha1, alpha_prev = 0.0, falpha, fpalpha, falpha_prev = f0v, fpalpha_prev = fp0v;
        double a = 0.0, b = alpha, f_a = f0v, f_b = 0.0, fp_a = fp0v, fp_b = 0.0;
        int i = 0;
        while (i++ < 100) {  // bracketing
            falpha = eval_f(alpha);
            if (falpha > f0v + alpha * rho * fp0v || falpha >= falpha_prev) { a = alpha_prev; f_a = falpha_prev; fp_a = fpalpha_prev; b = alpha; f_b = falpha; fp_b = nan; break; }
            fpalpha = eval_df(alpha);
            if (std::fabs(fpalpha) <= -sigma * fp0v) { alpha_new = alpha; return 0; }
            if (fpalpha >= 0) { a = alpha; f_a = falpha; fp_a = fpalpha; b = alpha_prev; f_b = falpha_prev; fp_b = fpalpha_prev; break; }
            const double delta = alpha - alpha_prev;
            const double next = interpolate(alpha_prev, falpha_prev, fpalpha_prev, alpha, falpha, fpalpha, alpha + delta, alpha + tau1 * delta);
            alpha_prev = alpha; falpha_prev = falpha; fpalpha_prev = fpalpha; alpha = next;
        }
        while (i++ < 100) {  // sectioning
            const double delta = b - a;
            alpha = interpolate(a, f_a, fp_a, b, f_b, fp_b, a + tau2 * delta, b - tau3 * delta);
            falpha = eval_f(alpha);
            if ((a - alpha) * fp_a <= std::numeric_limits<double>::epsilon()) return 1;
            if (falpha > f0v + rho * alpha * fp0v || falpha >= f_a) { b = alpha; f_b = falpha; fp_b = nan; }
            else {
                fpalpha = eval_df(alpha);
                if (std::fabs(fpalpha) <= -sigma * fp0v) { alpha_new = alpha; return 0; }
                if (((b - a) >= 0 && fpalpha >= 0) || ((b - a) <= 0 && fpalpha <= 0)) { b = a; f_b = f_a; fp_b = fp_a; }
                a = alpha; f_a = falpha; fp_a = fpalpha;
            }
        }
        return 0;
    }
    int step(double* x) {
        const double f_before = f;
        if (pnorm == 0.0 || g0norm == 0.0 || fp0 == 0) return 1;
        double alpha1 = 1.0, alpha = 0.0;
        if (delta_f < 0) alpha1 = std::min(1.0, 2.0 * std::max(-delta_f, 10 * std::numeric_limits<double>::epsilon() * std::fabs(f_before)) / (-fp0));
        const int status = line_search(alpha1, alpha);
        if (status != 0) return status;
        eval_fdf(alpha, fa, dfa);
        for (int i = 0; i < 6; ++i) { x[i] = xa[i]; gradient[i] = ga[i]; }
        f = fa;
        delta_f = f - f_before;
        double dx0[6], dg0[6];
        for (int i = 0; i < 6; ++i) { dx0[i] = x[i] - x0[i]; dg0[i] = gradient[i] - g0[i]; }
        const double dxg = dot6(dx0, gradient), dgg = dot6(dg0, gradient), dxdg = dot6(dx0, dg0), dgn = nrm(dg0);
        double A = 0, B = 0;
        if (dxdg != 0) { B = dxg / dxdg; A = -(1.0 + dgn * dgn / dxdg) * B + dgg / dxdg; }
        for (int i = 0; i < 6; ++i) p[i] = (-A * dx0[i] + gradient[i]) + -B * dg0[i];
        for (int i = 0; i < 6; ++i) { g0[i] = gradient[i]; x0[i] = x[i]; }
        g0norm = nrm(g0);
        pnorm = nrm(p);
        const double dir = dot6(p, gradient) > 0 ? -1.0 : 1.0;
        for (int i = 0; i < 6; ++i) p[i] *= dir / pnorm;
        pnorm = nrm(p);
        fp0 = dot6(p, g0);
        new_direction();
        return 0;
    }
};

// estimateRigidTransformationBFGS
template <class Fdf>
bool gicp_estimate(const int n_corr, LoopMat4f& transformation, Fdf&& fdf, int& inner_total) {
    if (n_corr < 4) return false;
    double x[6] = {double(transformation.m[12]), double(transformation.m[13]), double(transformation.m[14]),
                   std::atan2(double(transformation.m[2 + 4 * 1]), double(transformation.m[2 + 4 * 2])), std::asin(-double(transformation.m[2])),
                   std::atan2(double(transformation.m[1]), double(transformation.m[0]))};
    Bfgs<Fdf> b{fdf};
    b.start(x);
    int inner = 0, result;
    do {
        ++inner;
        result = b.step(x);
        if (result) break;
        result = b.nrm(b.gradient) < 1e-2 ? 0 : -1;
    } while (result == -1 && inner < 20);
    inner_total += inner;
    if (!(result == 1 || result == 0 || inner == 20)) return false;
    transformation = ident();
    apply_state(transformation, x);
    return true;
}

}  // namespace loop
}  // namespace fls
