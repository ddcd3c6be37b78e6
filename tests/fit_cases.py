"""Inputs and numpy models of the stages of the fit launch (csrc/kernels_p2plane.hpp, kernels_knn.hpp, kernels_grid_coop.hpp), shared by
tests/test_fit_cases.py (CPU: every family reaches what it is named after, by the oracle and the models alone) and tests/test_gpu_fit_stages.py
(GPU: the routines themselves through include/fls_debug_fit.h).  Deterministic (fixed seeds), every case labelled with its family so that a failure
names it; the arrays are built once per process and handed out read-only, like tests/linalg_cases.py, whose generators the point sets come from.

Neighbours, source points and transformed points are float32 values held in doubles (the kernels take float4 / float)."""
import functools
from fractions import Fraction

import numpy as np

from tests import linalg_cases as LC
from tests.linalg_cases import _Cases, _f32, _freeze, _unit

EPS = LC.EPS
CANARY = 7.0


def gamma(k):
    """gamma_k = k u / (1 - k u), u = 2^-53: the relative error bound of any k roundings in sequence (Higham, Accuracy and Stability, lemma 3.1)"""
    u = 2.0 ** -53
    return k * u / (1.0 - k * u)


def _rotation(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q * np.sign(np.linalg.det(Q))


def _pose(rng, t_scale):
    T = np.eye(4)
    T[:3, :3] = _rotation(rng)
    T[:3, 3] = rng.uniform(-1.0, 1.0, 3) * t_scale
    return T.reshape(-1, order="F")  # column-major


# ---------------------------------------------------------------------------------------------
# plane_residual_dev / line_residual_dev: (nn (n, 5, 3), ps (n, 3), pt (n, 3), T (n, 16), gate (n,), labels)
# ---------------------------------------------------------------------------------------------
def _plane_normal_and_gate(P):
    """from the ORACLE's plane fit of the five points: unit normal n, and max_j |r_j| / nrm as plane_residual forms it, operation by operation"""
    from oracle import oracle as O
    x = O.colpiv_qr_solve_5x3(P, -np.ones(5))
    with np.errstate(all="ignore"):
        nrm = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
        r = ((P[:, 0] * x[0] + P[:, 1] * x[1]) + P[:, 2] * x[2]) + 1.0
        return x / nrm, float(np.max(np.abs(r) / nrm))


def _stack(c):
    nn = np.stack([i[0] for i in c.items]); ps = np.stack([i[1] for i in c.items]); pt = np.stack([i[2] for i in c.items])
    T = np.stack([i[3] for i in c.items]); gate = np.array([i[4] for i in c.items], dtype=np.float64)
    assert np.array_equal(nn, _f32(nn)) and np.array_equal(ps, _f32(ps)) and np.array_equal(pt, _f32(pt))
    return _freeze(nn, ps, pt, T, gate, np.array(c.labels))


@functools.lru_cache(maxsize=None)
def plane_residual_cases():
    from oracle import oracle as O
    rng = np.random.default_rng(6101)
    A, lab = LC.plane_fit_cases()
    planes = A[lab == "noisy_plane"]     # 600, noise 0 .. 0.2 m, |centre| <= 140 m
    far = A[lab == "far_mm"]             # 200, up to 2.5 km
    c = _Cases()

    def src(lo=5.0, hi=60.0):
        return _f32(_unit(rng) * rng.uniform(lo, hi))

    for k in range(300):   # every noise level against the workload's threshold, pt a few centimetres to decimetres off the plane, either side
        P = planes[2 * k]
        c.add("noisy_plane", (P, src(), _f32(P[0] + rng.normal(size=3) * rng.choice([0.02, 0.1, 0.4])), _pose(rng, 100.0), 0.1))
    for k in range(100):   # 2.5 km from the origin; the threshold lets the millimetre clouds through or not
        P = far[k]
        c.add("far_mm", (P, src(100.0, 2500.0), _f32(P[0] + rng.normal(size=3) * 0.05), _pose(rng, 2500.0), 10.0 ** rng.uniform(-4, 0)))
    for k in range(150):   # the threshold exactly the oracle's own max |r| / nrm (not above it: valid), and the next double towards zero (invalid)
        P = planes[2 * k + 1] if k % 3 else far[100 + k // 3]
        _, g = _plane_normal_and_gate(P)
        ps, pt, T = src(30.0, 60.0), _f32(P[0] + rng.normal(size=3) * 0.02), _pose(rng, 100.0)
        c.add("thres_at_gate", (P, ps, pt, T, g))
        c.add("thres_below_gate", (P, ps, pt, T, float(np.nextafter(g, 0.0))))
    for k in range(260):   # range within 1e-6 relative of 81 d^2, either side: |ps| scaled from the oracle's own d
        P = planes[(7 * k) % 600]
        pt, T = _f32(P[0] + rng.normal(size=3) * 0.15), _pose(rng, 100.0)
        _, _, d = O.plane_residual(P[None], np.array([[1e4, 0.0, 0.0]]), pt[None], T[None], np.array([1e9]))
        delta = rng.uniform(1e-7, 1e-6) * (1.0 if k % 2 else -1.0)
        c.add("range_gate", (P, _f32(_unit(rng) * (81.0 * d[0] * d[0]) * (1.0 + delta)), pt, T, 1e9))
    for k in range(60):    # pt is the nearest neighbour itself: d == 0 exactly, not > 0, so s = -1 and d_abs = 0
        P = planes[(11 * k + 3) % 600]
        c.add("d_zero", (P, src(), P[0].copy(), _pose(rng, 100.0), 1e9))
    for k in range(120):   # pt a decimetre off the plane along the fitted normal, below (d < 0) and above
        P = planes[(13 * k + 5) % 600]
        n, _ = _plane_normal_and_gate(P)
        c.add("d_negative" if k % 2 else "d_positive", (P, src(), _f32(P[0] + n * (-0.1 if k % 2 else 0.1)), _pose(rng, 100.0), 1e9))
    for P in A[lab == "identical"]:
        c.add("identical", (P, src(), _f32(P[0] + rng.normal(size=3) * 0.1), _pose(rng, 100.0), 0.1 if len(c.items) % 2 else 1e9))
    for P in A[lab == "collinear"]:
        c.add("collinear", (P, src(), _f32(P[0] + rng.normal(size=3) * 0.1), _pose(rng, 100.0), 0.1 if len(c.items) % 2 else 1e9))
    for k in range(24):    # all-zero neighbours: the fit is (NaN, NaN, inf), every comparison with the NaN norm is false: VALID, with NaN J
        c.add("zeros", (np.zeros((5, 3)) * (-1.0 if k % 2 else 1.0), src(), _f32(rng.normal(size=3)), _pose(rng, 100.0), 0.1))
    for k in range(40):    # the same system under two poses that share the rotation: only the rotation may enter J
        P = planes[(17 * k + 1) % 600]
        ps, pt, T = src(), _f32(P[0] + rng.normal(size=3) * 0.05), _pose(rng, 1.0)
        T2 = T.copy(); T2[12:15] = rng.uniform(-1.0, 1.0, 3) * 1e6
        c.add("pose_a", (P, ps, pt, T, 1e9))
        c.add("pose_b", (P, ps, pt, T2, 1e9))
    return _stack(c)


def _line_points(rng, centre, length, noise):
    d = _unit(rng)
    return _f32(centre + np.linspace(-1.0, 1.0, 5)[:, None] * d * length + rng.normal(size=(5, 3)) * noise)


def _exact_mean_line(rng):
    """five points around an integer centroid c0 whose left-to-right sum / 5.0 is c0 exactly (multiples of 1/64, offsets that cancel)"""
    c0 = rng.integers(-40, 41, 3).astype(np.float64)
    d = rng.integers(-3, 4, 3).astype(np.float64); d[0] += (not d.any())
    a, b, e = (rng.integers(-8, 9, 3) / 64.0 for _ in range(3))
    P = c0 + np.arange(-2.0, 3.0)[:, None] * d + np.stack([a, b, -a - b, e, -e])
    return P, c0


@functools.lru_cache(maxsize=None)
def line_residual_cases():
    from oracle import oracle as O
    rng = np.random.default_rng(6102)
    A, lab = LC.plane_fit_cases()
    c = _Cases()

    def src(lo=5.0, hi=60.0):
        return _f32(_unit(rng) * rng.uniform(lo, hi))

    for k in range(300):   # lines at 1 m .. 2.5 km, noise 1e-4 .. 0.3 of their length, against the workload's ratio
        centre = _unit(rng) * 10.0 ** rng.uniform(0.0, np.log10(2500.0))
        length = rng.uniform(0.1, 2.0)
        P = _line_points(rng, centre, length, length * 10.0 ** rng.uniform(-4.0, 0.5))
        c.add("noisy_line", (P, src(), _f32(P[2] + rng.normal(size=3) * 0.1), _pose(rng, 2500.0), 3.0))
    for k in range(70):    # ratio = S0 / S1 of the oracle's own singular values, and its two neighbours either way: the oracle decides each
        P = _line_points(rng, _unit(rng) * 10.0 ** rng.uniform(0.0, 2.0), 1.0, 10.0 ** rng.uniform(-2.0, -0.7))
        _, S, _ = O.svd3(LC.covariance5(P))
        ps, pt, T = src(), _f32(P[2] + rng.normal(size=3) * 0.1), _pose(rng, 100.0)
        g = S[0] / S[1]
        lo1 = np.nextafter(g, 0.0); lo2 = np.nextafter(lo1, 0.0); hi1 = np.nextafter(g, np.inf); hi2 = np.nextafter(hi1, np.inf)
        for name, v in (("ratio_m2", lo2), ("ratio_m1", lo1), ("ratio_0", g), ("ratio_p1", hi1), ("ratio_p2", hi2)):
            c.add(name, (P, ps, pt, T, float(v)))
    for k in range(30):    # pt at the centroid: a = 0, w = 0, dist = 0, u = 0 / 0: VALID, with NaN J
        P, c0 = _exact_mean_line(rng)
        c.add("dist_zero", (P, src(), c0, _pose(rng, 100.0), 3.0))
    for P in A[lab == "identical"]:   # S = 0: 0 <= ratio * 0, invalid
        c.add("identical", (P, src(), _f32(P[0] + rng.normal(size=3) * 0.1), _pose(rng, 100.0), 3.0))
    for P in A[lab == "collinear"]:   # exact lines
        c.add("collinear", (P, src(), _f32(P[0] + rng.normal(size=3) * 0.1), _pose(rng, 100.0), 3.0))
    for k in range(4):
        c.add("zeros", (np.zeros((5, 3)) * (-1.0 if k % 2 else 1.0), src(), _f32(rng.normal(size=3)), _pose(rng, 100.0), 3.0))
    for k in range(40):
        P = _line_points(rng, _unit(rng) * 30.0, 1.0, 1e-3)
        ps, pt, T = src(), _f32(P[2] + rng.normal(size=3) * 0.1), _pose(rng, 1.0)
        T2 = T.copy(); T2[12:15] = rng.uniform(-1.0, 1.0, 3) * 1e6
        c.add("pose_a", (P, ps, pt, T, 3.0))
        c.add("pose_b", (P, ps, pt, T2, 3.0))
    return _stack(c)


@functools.lru_cache(maxsize=None)
def oracle_plane_residual():
    from oracle import oracle as O
    nn, ps, pt, T, gate, _ = plane_residual_cases()
    with np.errstate(all="ignore"):
        return _freeze(*O.plane_residual(nn, ps, pt, T, gate))


def oracle_plane_residual_far_source():
    """d_abs of the `range_gate` systems with the source point 10 km away (the range gate open): what their |ps| was scaled from"""
    from oracle import oracle as O
    nn, ps, pt, T, gate, lab = plane_residual_cases()
    m = lab == "range_gate"
    far = np.tile([1e4, 0.0, 0.0], (int(m.sum()), 1))
    return O.plane_residual(nn[m], far, pt[m], T[m], gate[m])[2]


@functools.lru_cache(maxsize=None)
def oracle_line_residual():
    from oracle import oracle as O
    nn, ps, pt, T, gate, _ = line_residual_cases()
    with np.errstate(all="ignore"):
        return _freeze(*O.line_residual(nn, ps, pt, T, gate))


# ---------------------------------------------------------------------------------------------
# icp_point_rows: (T (n, 16), p (n, 3), m (n, 3), labels) and the numpy model of the oracle's in-line per-point code
# ---------------------------------------------------------------------------------------------
def xform_f_model(T, p):
    """TransformPointCloud(.., Mat4d) as both sides form it: R and t cast to float, (r0 x + (r1 y + r2 z)) + t in float"""
    Tf = T.astype(np.float32)
    x, y, z = (p[:, k].astype(np.float32) for k in range(3))
    return np.stack([(Tf[:, r] * x + (Tf[:, r + 4] * y + Tf[:, r + 8] * z)) + Tf[:, 12 + r] for r in range(3)], axis=1)


def icp_point_rows_model(T, p, m):
    """flo_oracle.cpp, IcpOptimized::Match, the per-point lines, operation by operation: e = double(T (x) p in float) - double(m); J = [I | -(R hat(p))],
    3 x 6 column-major, the products of R hat(p) summed (a + b) + c with their zero terms kept; res = sqrt((e0 e0 + e1 e1) + e2 e2)"""
    n = T.shape[0]
    q = xform_f_model(T, p)
    assert q.dtype == np.float32
    e = q.astype(np.float64) - m
    o = p
    zero = np.zeros(n)
    hat = np.stack([zero, o[:, 2], -o[:, 1], -o[:, 2], zero, o[:, 0], o[:, 1], -o[:, 0], zero], axis=1)  # column-major
    J = np.zeros((n, 18))
    for j in range(3):
        for r in range(3):
            J[:, r + j * 3] = 1.0 if r == j else 0.0
            J[:, r + (j + 3) * 3] = -((T[:, r] * hat[:, 0 + j * 3] + T[:, r + 4] * hat[:, 1 + j * 3]) + T[:, r + 8] * hat[:, 2 + j * 3])
    res = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    return J, e, res


@functools.lru_cache(maxsize=None)
def icp_point_rows_cases():
    rng = np.random.default_rng(6103)
    c = _Cases()
    for k in range(300):
        p = _f32(_unit(rng) * rng.uniform(1.0, 80.0))
        c.add("random", (_pose(rng, 50.0), p, _f32(rng.normal(size=3) * 50.0)))
    for k in range(20):    # a source point at the origin: hat(p) = 0 with both signs of zero, every product of the right block a zero
        c.add("origin", (_pose(rng, 50.0), np.zeros(3) * (-1.0 if k % 2 else 1.0), _f32(rng.normal(size=3) * 50.0)))
    for k in range(100):   # coordinates up to 2.5 km
        c.add("far", (_pose(rng, 2500.0), _f32(rng.uniform(-2500, 2500, 3)), _f32(rng.uniform(-2500, 2500, 3))))
    for k in range(40):    # the map point is the transformed point itself: e = 0, res = 0 (filled in below)
        c.add("e_zero", (_pose(rng, 50.0), _f32(_unit(rng) * rng.uniform(1.0, 80.0)), np.zeros(3)))
    T = np.stack([i[0] for i in c.items]); p = np.stack([i[1] for i in c.items]); m = np.stack([i[2] for i in c.items])
    lab = np.array(c.labels)
    m[lab == "e_zero"] = xform_f_model(T, p)[lab == "e_zero"].astype(np.float64)
    return _freeze(T, p, m, lab)


# ---------------------------------------------------------------------------------------------
# wave reductions of the rank-1 terms: contrib (n, 64) bool, J (n, 64, 6), r (n, 64); three-row form: J (n, 64, 18), e (n, 64, 3)
# ---------------------------------------------------------------------------------------------
POISON = (np.nan, np.inf, -np.inf, 1e308, -1e308)


def lane_masks():
    """[(name, mask (64,) bool)]: none, all, every lane alone, the first k lanes, alternating, one lane per 16-lane row"""
    out = [("none", np.zeros(64, bool)), ("all", np.ones(64, bool))]
    for l in range(64):
        m = np.zeros(64, bool); m[l] = True
        out.append(("lane%02d" % l, m))
    for k in (1, 7, 8, 9, 31, 32, 33, 63):
        out.append(("first%02d" % k, np.arange(64) < k))
    out.append(("even", np.arange(64) % 2 == 0)); out.append(("odd", np.arange(64) % 2 == 1))
    m = np.zeros(64, bool); m[[3, 16 + 7, 32 + 0, 48 + 15]] = True
    out.append(("one_per_row", m))
    m = np.zeros(64, bool); m[[0, 16 + 8, 32 + 8, 48 + 0]] = True   # (owners of the three-row form)
    out.append(("one_owner_per_row", m))
    return out


def _poison(rng, shape):
    return np.asarray(POISON)[rng.integers(0, len(POISON), shape)]


def _rank1_family(width, res_w, seed):
    """width: J entries per lane (6 / 18), res_w: residual entries per lane (1 / 3).  Returns contrib, J, r (n, 64, res_w), labels, and `twin`:
    for a poisoned case the index of the same case with zeros in the lanes that do not contribute (else -1)."""
    rng = np.random.default_rng(seed)
    owners = (np.arange(64) % 8 == 0) if width == 18 else np.ones(64, bool)
    C, Js, Rs, lab, twin = [], [], [], [], []

    def add(label, mask, J, r, tw=-1):
        C.append(mask.copy()); Js.append(J); Rs.append(r); lab.append(label); twin.append(tw)
        return len(C) - 1

    # exact integers, |.| <= 2^10: every product and partial sum is exact, every summation order gives the same bits
    for name, mask in lane_masks():
        J = rng.integers(-1024, 1025, (64, width)).astype(np.float64)
        r = rng.integers(-1024, 1025, (64, res_w)).astype(np.float64)
        used = mask & owners
        Jc, rc = J * used[:, None], r * used[:, None]
        clean = add("int_" + name, mask, Jc + 0.0, rc + 0.0)
        Jp, rp = Jc.copy(), rc.copy()
        Jp[~used] = _poison(rng, (int((~used).sum()), width)); rp[~used] = _poison(rng, (int((~used).sum()), res_w))
        add("int_poison_" + name, mask, Jp, rp, clean)
    # determinism: one case in every wave slot of two workgroups (the index of a case modulo 4 is its wave slot)
    J = rng.integers(-1024, 1025, (64, width)).astype(np.float64) * np.ldexp(1.0, rng.integers(-20, 21, (64, width)))
    r = rng.normal(size=(64, res_w))
    while len(C) % 4: add("pad", np.zeros(64, bool), np.zeros((64, width)), np.zeros((64, res_w)))
    for k in range(8):
        add("repeat", np.arange(64) % 3 != 0, J, r)
    # magnitudes 2^-40 .. 2^40, mixed signs
    for k in range(24):
        J = np.ldexp(rng.uniform(1.0, 2.0, (64, width)), rng.integers(-40, 41, (64, width))) * rng.choice([-1.0, 1.0], (64, width))
        r = np.ldexp(rng.uniform(1.0, 2.0, (64, res_w)), rng.integers(-40, 41, (64, res_w))) * rng.choice([-1.0, 1.0], (64, res_w))
        add("wide", (rng.uniform(size=64) < 0.8) if k % 2 else np.ones(64, bool), J, r)
    # built to cancel: lanes (or owners) in pairs, the second the first with every other entry negated and moved by 2^-30 relative, so that the
    # off-diagonal sums and the gradient are ~2^-30 of the sum of their terms' magnitudes
    step = 8 if width == 18 else 1
    for k in range(16):
        J = rng.normal(size=(64, width)) * 10.0 ** rng.uniform(-2, 2)
        r = rng.normal(size=(64, res_w))
        sgn = np.where(np.arange(width) % 2 == 0, 1.0, -1.0) if width == 6 else np.where((np.arange(width) // 3) % 2 == 0, 1.0, -1.0)
        for l in range(0, 64, 2 * step):
            J[l + step] = J[l] * sgn * (1.0 + 2.0 ** -30 * rng.integers(-3, 4, width))
            r[l + step] = (-r[l] if width == 6 else r[l]) * (1.0 + 2.0 ** -30 * rng.integers(-3, 4, res_w))
        add("cancel", np.ones(64, bool), J, r)
    return _freeze(np.stack(C), np.stack(Js), np.stack(Rs), np.array(lab), np.array(twin))


@functools.lru_cache(maxsize=None)
def rank1_cases():
    return _rank1_family(6, 1, 6104)


@functools.lru_cache(maxsize=None)
def rank1x3_cases():
    return _rank1_family(18, 3, 6105)


TRI = [(a, b) for a in range(6) for b in range(a, 6)]   # column k of a partial row = H(a, b), a <= b, row-wise upper triangle


def rank1_terms(contrib, J, r):
    """the terms of the 29 sums of ONE case as (64, 29) float arrays of operand pairs (x, y): column c is sum_l x[l, c] * y[l, c]:
    0..20 J_a J_b; 21..26 (-J_a) r; 27 r * 1; 28 1 * 1.  Lanes that do not contribute are zero."""
    z = contrib.astype(np.float64)[:, None]
    Jz = np.where(contrib[:, None], J, 0.0)
    rz = np.where(contrib[:, None], r, 0.0)[:, :1]
    x = np.concatenate([Jz[:, [a for a, _ in TRI]], -Jz, rz, z], axis=1)
    y = np.concatenate([Jz[:, [b for _, b in TRI]], np.repeat(rz, 6, axis=1), z, z], axis=1)
    return x, y


def rank1x3_terms(contrib, J, e):
    """the same for the three-row form, (24, 29) operand pairs: the rows r = 0..2 of the owners (lane % 8 == 0); column 27 is the caller's (all zero
    here), column 28 counts the owners"""
    xs, ys = [], []
    for l in range(0, 64, 8):
        for r in range(3):
            on = bool(contrib[l])
            v = np.array([J[l, r + 3 * a] for a in range(6)]) if on else np.zeros(6)
            er = float(e[l, r]) if on else 0.0
            one = 1.0 if (on and r == 0) else 0.0
            xs.append(np.concatenate([v[[a for a, _ in TRI]], -v, [0.0], [one]]))
            ys.append(np.concatenate([v[[b for _, b in TRI]], np.full(6, er), [0.0], [one]]))
    return np.stack(xs), np.stack(ys)


def exact_sums(x, y):
    """(exact sum of x y, exact sum of |x y|) per column, as Fractions"""
    s, a = [], []
    for c in range(x.shape[1]):
        t = [Fraction(float(x[l, c])) * Fraction(float(y[l, c])) for l in range(x.shape[0]) if x[l, c] != 0.0 and y[l, c] != 0.0]
        s.append(sum(t, Fraction(0))); a.append(sum((abs(v) for v in t), Fraction(0)))
    return s, a


def rank1_dpp_model(contrib, J, r):
    """reduce_rank1_and_store: each product rounded once, then wave_sum_dpp's tree (tests/linalg_cases.py::wave_sum_model); (n, 29)"""
    out = np.zeros((contrib.shape[0], 29))
    with np.errstate(all="ignore"):
        for s in range(contrib.shape[0]):
            x, y = rank1_terms(contrib[s], J[s], r[s])
            prod = x * y
            prod[~contrib[s]] = 0.0   # (`contrib ? J[a] * J[b] : 0.0`: +0.0 whatever the sign of the product of zeros)
            out[s] = LC.wave_sum_model(prod.T.copy())
    return out


# ---------------------------------------------------------------------------------------------
# reduce_partials<NT, SC1, U>: rows (1100, 32), and the model of its fixed order
# ---------------------------------------------------------------------------------------------
REDUCE_VARIANTS = ((256, 32), (512, 16), (512, 32), (1024, 16))   # (NT, U) of variant 0..3 of fls_debug_reduce_partials


def reduce_row_counts(variant):
    NT, U = REDUCE_VARIANTS[variant]
    NG = NT // 32
    # (no caller passes 0 rows: the row count is a launch's grid size)
    n = {1, NG - 1, NG, NG + 1, (U - 4) * NG - 1, (U - 4) * NG, (U - 4) * NG + 1, U * NG - 1, U * NG, U * NG + 1, 2 * U * NG + 3, 205, 225, 457}
    return sorted(v for v in n if 1 <= v <= 1100)


@functools.lru_cache(maxsize=None)
def partial_rows():
    """(wide (1100, 32): magnitudes 2^-40 .. 2^40, mixed signs, in all 32 columns; ints (1100, 32): |.| < 2^20)"""
    rng = np.random.default_rng(6106)
    wide = np.ldexp(rng.uniform(1.0, 2.0, (1100, 32)), rng.integers(-40, 41, (1100, 32))) * rng.choice([-1.0, 1.0], (1100, 32))
    ints = rng.integers(-(1 << 20), 1 << 20, (1100, 32)).astype(np.float64)
    return _freeze(wide, ints)


def reduce_partials_model(rows, nrows, NT, U):
    """add by add: row group g = 0 .. NG - 1 sums rows g, g + NG, g + 2 NG, ... in that order from 0.0, whole trips of U rows with zeros past nrows;
    then tot = ((0 + acc_0) + acc_1) + ... over the groups.  (32,)"""
    NG = NT // 32
    acc = np.zeros((NG, 32))
    trips = 0
    while trips * U * NG < nrows:   # (a group whose first row of the trip is past nrows adds nothing: the same as adding zeros)
        trips += 1
    padded = np.zeros((trips * U * NG, 32))
    padded[:nrows] = rows[:nrows]
    for k in range(trips * U):
        acc = acc + padded[k * NG:(k + 1) * NG]
    tot = np.zeros(32)
    for g in range(NG):
        tot = tot + acc[g]
    return tot


# ---------------------------------------------------------------------------------------------
# fan-in: the rows fls_debug_fanin publishes
# ---------------------------------------------------------------------------------------------
FANIN_BLOCKS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 64, 205, 457)


def fanin_totals(nblocks):
    """(2, 32) exact: launch k, column col: sum_b (k + 1)(b + 1)(col + 1) + 1000 k b"""
    b = np.arange(nblocks, dtype=np.int64)[:, None]; col = np.arange(32, dtype=np.int64)[None, :]
    return np.stack([((k + 1) * (b + 1) * (col + 1) + 1000 * k * b).sum(0) for k in range(2)]).astype(np.float64)
