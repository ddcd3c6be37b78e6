"""Inputs of the device linear-algebra primitives (csrc/linalg_dev.hpp, csrc/wave_solve.hpp), shared by tests/test_oracle_linalg_cases.py
(CPU: the generators reach the branches they name, by the oracle alone), tests/test_gpu_linalg.py and tests/test_gpu_solver.py (GPU: the
device against the oracle).  Deterministic (fixed seeds), a few thousand systems per routine, every system labelled with its family so that a
failure names it.  The arrays are built once per process and handed out read-only.

Plane-fit and covariance entries are float32-representable in every family but `general_f64`: the kernels cast them from float4."""
import functools

import numpy as np

EPS = 2.220446049250313e-16


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


class _Cases:
    def __init__(self):
        self.items, self.labels = [], []

    def add(self, label, item):
        self.items.append(item)
        self.labels.append(label)


def _unit(rng, n=None):
    v = rng.normal(size=3 if n is None else (n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ---------------------------------------------------------------------------------------------
# 6x6 normal equations of the Gauss-Newton tails (moved here from tests/test_gpu_solver.py: both GPU files use them)
# ---------------------------------------------------------------------------------------------
def _systems():
    rng = np.random.default_rng(20241022)
    Hs, gs = [], []

    def add(J, r):
        Hs.append(J.T @ J); gs.append(-J.T @ r)

    for k in range(3000):
        kind = k % 10
        n = int(rng.integers(6, 400))
        J = rng.normal(size=(n, 6)) * rng.choice([1e-3, 1.0, 50.0], size=6)
        if kind == 1: J[:, 3:] = np.outer(rng.normal(size=n), [0.0, 0.0, 1.0])                 # all normals parallel (a single plane): rank 3-4
        if kind == 2: J[:, 5] = 0.0                                                             # an unobserved direction
        if kind == 3: J[:, 4] = J[:, 3] * 2.0                                                   # exactly dependent columns
        if kind == 4: J = J[:2]                                                                 # two residuals only
        if kind == 5: J *= 0.0                                                                  # nothing valid: H = 0
        if kind == 6: J[:, 0] *= 1e-9                                                           # a nearly negligible pivot
        if kind == 7: J = np.round(J)                                                           # small integers: exact ties in the pivot search
        r = rng.normal(size=J.shape[0]) * 0.05
        add(J, r)
    H = np.stack(Hs); g = np.stack(gs)
    H = 0.5 * (H + H.transpose(0, 2, 1))  # exactly symmetric, like the device's upper-triangle assembly
    return H, g


@functools.lru_cache(maxsize=None)
def gn_systems():
    """_systems(), built once, read-only"""
    return _freeze(*_systems())


# ---------------------------------------------------------------------------------------------
# plane fit: A (n, 5, 3), rows = the five neighbours, columns = x y z; the right-hand side is -1
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plane_fit_cases():
    rng = np.random.default_rng(5301)
    c = _Cases()

    def plane_points(centre, normal, spread, noise):
        u = np.cross(normal, [1.0, 0.0, 0.0] if abs(normal[0]) < 0.9 else [0.0, 1.0, 0.0]); u /= np.linalg.norm(u)
        w = np.cross(normal, u)
        return centre + rng.uniform(-spread, spread, (5, 1)) * u + rng.uniform(-spread, spread, (5, 1)) * w + rng.normal(0.0, 1.0, (5, 1)) * noise * normal

    for k in range(600):   # random planes, noise 0 .. 0.2 m
        c.add("noisy_plane", _f32(plane_points(rng.uniform(-80, 80, 3), _unit(rng), 0.4, 0.2 * k / 599.0)))
    for k in range(200):   # coordinates up to 2.5 km, millimetre spread: a float32 ulp there is 0.24 mm, the points nearly coincide
        c.add("far_mm", _f32(rng.uniform(-2500, 2500, 3) + rng.uniform(-1e-3, 1e-3, (5, 3))))
    for k in range(100):   # five collinear points, exact (integers): rank 2, or rank 1 when the line passes through the origin
        p0 = rng.integers(-9, 10, 3).astype(np.float64) * (k % 4 != 0)
        d = rng.integers(-3, 4, 3).astype(np.float64)
        d[0] += (not d.any())
        c.add("collinear", p0 + np.arange(5.0)[:, None] * d * (1.0 if k % 2 else 0.25))
    for k in range(50):    # five identical points: rank 1
        p = _f32(rng.uniform(-50, 50, 3)) if k % 2 else rng.integers(-9, 10, 3).astype(np.float64)
        c.add("identical", np.tile(p, (5, 1)))
    for k in range(4):     # all zeros: rank 0 (Eigen keeps all three pivots there and divides by zero: tests/test_oracle_linalg_cases.py)
        c.add("zeros", np.zeros((5, 3)) * (-1.0 if k % 2 else 1.0))
    for k in range(100):   # a plane through the origin: A x = -1 has no solution there
        if k % 2:
            a, b = rng.integers(-6, 7, 5).astype(np.float64), rng.integers(-6, 7, 5).astype(np.float64)
            c.add("through_origin", np.stack([a, b, a + b], axis=1)[:, rng.permutation(3)])   # x + y - z = 0, exact
        else:
            c.add("through_origin", _f32(plane_points(np.zeros(3), _unit(rng), 5.0, 0.0)))
    for k in range(150):   # axis-aligned planes: one column constant or zero
        P = rng.uniform(-30, 30, (5, 3))
        P[:, k % 3] = 0.0 if k % 2 else float(np.float32(rng.uniform(-20, 20)))
        c.add("axis_zero_column" if k % 2 else "axis_const_column", _f32(P))
    for k in range(200):   # two or three columns of exactly equal norm (sign flips / integer permutations keep the squares): the first wins
        col = _f32(rng.uniform(-10, 10, 5)) if k % 2 else rng.integers(-4, 5, 5).astype(np.float64)
        P = _f32(rng.uniform(-3, 3, (5, 3)))
        cols = [0, 1, 2] if k % 4 < 2 else list(rng.permutation(3)[:2])
        for j in cols:
            P[:, j] = col * rng.choice([-1.0, 1.0], 5)
        if k % 2 == 0 and k % 3 == 0:
            P[:, cols[-1]] = col[rng.permutation(5)]   # integers: a permutation has the same exact sum of squares
        c.add("norm_tie3" if len(cols) == 3 else "norm_tie2", P)
    for k in range(150):   # two nearly parallel columns: after the first reflection the other's norm collapses, the down-date recomputes it
        P = rng.uniform(-10, 10, (5, 3))
        a, b, o = rng.permutation(3)
        P[:, o] *= 0.1   # (the first pivot is one of the pair)
        P[:, b] = P[:, a] * rng.choice([1.0, -1.0, 0.5]) + rng.normal(size=5) * 10.0 ** rng.uniform(-6, -4)
        c.add("near_parallel", _f32(P))
    for k in range(60):    # the pivot column's only non-zero entry is on the diagonal: tail <= DBL_MIN, tau = 0
        P = np.zeros((5, 3))
        o = rng.permutation(3)
        P[0, o[0]] = rng.choice([-1.0, 1.0]) * rng.uniform(20, 30)
        P[0, o[1]], P[1, o[1]] = rng.uniform(-3, 3), rng.choice([-1.0, 1.0]) * rng.uniform(8, 12)   # second step: again only the diagonal below row 0
        P[:, o[2]] = rng.uniform(-2, 2, 5) * (k % 3 != 0)
        if k % 3 == 1: P[3:, o[2]] = 0.0
        c.add("diagonal_only", _f32(P))
    for k in range(300):   # small integers: exact arithmetic for a while, ties everywhere
        c.add("small_int", rng.integers(-3, 4, (5, 3)).astype(np.float64))
    for k in range(300):   # general doubles (not float32-representable)
        c.add("general_f64", rng.normal(size=(5, 3)) * 10.0 ** rng.uniform(-3, 3))
    return _freeze(np.stack(c.items), np.array(c.labels))


# ---------------------------------------------------------------------------------------------
# SVD 3x3: A (n, 3, 3)
# ---------------------------------------------------------------------------------------------
def covariance5(P):
    """covariance of five points as line_residual_dev (csrc/kernels_knn.hpp) forms it, operation by operation: mean by a left-to-right sum / 5.0,
    sum_k D[k][i] * D[k][j] left to right from 0.0, / 5.0"""
    P = np.asarray(P, dtype=np.float64)
    m = ((((P[0] + P[1]) + P[2]) + P[3]) + P[4]) / 5.0
    D = P - m
    C = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(5):
                s += D[k, i] * D[k, j]
            C[i, j] = s / 5.0
    return C


@functools.lru_cache(maxsize=None)
def svd3_cases():
    rng = np.random.default_rng(5302)
    c = _Cases()
    for k in range(600):   # covariances of five float32 points: along a line, on a plane, a blob, far from the origin
        centre = rng.uniform(-80, 80, 3) * (30.0 if k % 5 == 4 else 1.0)
        d = _unit(rng)
        if k % 3 == 0: P = centre + np.linspace(-1, 1, 5)[:, None] * d * rng.uniform(0.1, 2.0) + rng.normal(size=(5, 3)) * 10.0 ** rng.uniform(-4, -1)
        elif k % 3 == 1: P = centre + rng.normal(size=(5, 3)) * rng.uniform(0.05, 1.0)
        else: P = centre + rng.uniform(-1, 1, (5, 1)) * d + rng.uniform(-1, 1, (5, 1)) * _unit(rng)
        c.add("cov5", covariance5(_f32(P)))
    for k in range(100):   # exact rank 1: u u^T of small integers or of float32 values (24-bit products are exact in double)
        u = rng.integers(-4, 5, 3).astype(np.float64) if k % 2 else _f32(rng.normal(size=3))
        u[0] += (not u.any())
        w = u if k % 4 < 2 else (rng.integers(-4, 5, 3).astype(np.float64) if k % 2 else _f32(rng.normal(size=3)))   # u w^T: rank 1, not symmetric
        c.add("rank1", np.outer(u, w))
    for k in range(3):
        c.add("rank0", np.zeros((3, 3)) * (-1.0 if k == 1 else 1.0))
    for k in range(100):   # already diagonal, any order and sign, zeros among the entries: no rotation happens
        dvals = rng.normal(size=3) * 10.0 ** rng.uniform(-3, 3, 3)
        if k % 4 == 1: dvals[rng.integers(3)] = 0.0
        if k % 4 == 2: dvals[rng.permutation(3)[:2]] = 0.0
        c.add("diagonal", np.diag(dvals))
    for k in range(120):   # isotropic s I and two equal singular values, in every position: the sort's first maximum wins
        s, t = float(np.float32(10.0 ** rng.uniform(-3, 3))), float(np.float32(10.0 ** rng.uniform(-3, 3)))
        pat = [(s, s, s), (s, s, t), (t, s, s), (s, t, s), (0.0, s, s), (s, 0.0, s), (s, s, 0.0), (-s, s, s), (s, -s, t), (0.0, 0.0, s)][k % 10]
        c.add("isotropic" if k % 10 == 0 else "two_equal", np.diag(pat))
    for k in range(300):   # scales 2^-900 .. 2^900
        A = rng.normal(size=(3, 3))
        if k % 2: A = A @ A.T
        c.add("scales", np.ldexp(A, int(rng.integers(-900, 901))))
    for k in range(400):   # general non-symmetric doubles: the first rotation has d != 0
        c.add("general", rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-2, 2))
    return _freeze(np.stack(c.items), np.array(c.labels))


# ---------------------------------------------------------------------------------------------
# LU 6x6: H (n, 6, 6), b (n, 6)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lu6_cases():
    rng = np.random.default_rng(5303)
    c = _Cases()
    H, g = gn_systems()
    for s in range(H.shape[0]):
        c.add("gn_kind%d" % (s % 10), (H[s], g[s]))
    for k in range(400):   # general non-symmetric
        c.add("general", (rng.normal(size=(6, 6)) * 10.0 ** rng.uniform(-3, 3), rng.normal(size=6)))
    for k in range(240):   # a permutation of 0..5 transpositions times a diagonal, a little noise on top: sign of det = parity
        t = k % 6
        P = np.eye(6)
        for _ in range(t):
            i, j = rng.permutation(6)[:2]
            P[[i, j]] = P[[j, i]]
        A = P @ np.diag(rng.uniform(1.0, 9.0, 6) * rng.choice([-1.0, 1.0], 6)) + (rng.normal(size=(6, 6)) * 1e-3 if k % 2 else 0.0)
        c.add("perm_t%d" % t, (A, rng.normal(size=6)))
    for k in range(300):   # pivot-column ties: small integers; every other one with the maximum of a column repeated, sign flipped, further down
        A = rng.integers(-2, 3, (6, 6)).astype(np.float64)
        if k % 2:
            j = int(rng.integers(6)); i0, i1 = sorted(rng.permutation(6)[:2])
            A[i0, j], A[i1, j] = 3.0, -3.0
        c.add("pivot_tie", (A, rng.integers(-3, 4, 6).astype(np.float64)))
    for k in range(2):
        c.add("zero", (np.zeros((6, 6)), rng.normal(size=6) * k))
    for k in range(120):   # a zero column in each of the six positions
        A = rng.normal(size=(6, 6)) if k % 2 else rng.integers(-3, 4, (6, 6)).astype(np.float64)
        A[:, k % 6] = 0.0
        c.add("zero_col%d" % (k % 6), (A, rng.normal(size=6)))
    for k in range(100):   # two equal rows of small integers: the second becomes exactly zero when the first is the pivot row, det = 0 exactly
        A = rng.integers(-3, 4, (6, 6)).astype(np.float64)
        i, j = rng.permutation(6)[:2]
        A[j] = A[i]
        c.add("equal_rows", (A, rng.normal(size=6)))
    for k in range(200):   # power-of-two scalings: same mantissas, det = 2^(6 e) det(A) until it overflows (e > 170) or underflows
        A = rng.normal(size=(6, 6)) if k % 2 else rng.integers(-3, 4, (6, 6)).astype(np.float64) + np.eye(6) * 7.0
        e = int(rng.integers(-200, 201))
        c.add("pow2", (np.ldexp(A, e), np.ldexp(rng.normal(size=6), e)))
    return _freeze(np.stack([h for h, _ in c.items]), np.stack([b for _, b in c.items]), np.array(c.labels))


# ---------------------------------------------------------------------------------------------
# SO3: v (n, 3), R (n, 3, 3)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def so3_cases():
    rng = np.random.default_rng(5304)
    c = _Cases()
    nxt = float(np.nextafter(EPS, 1.0))
    c.add("zero", np.zeros(3)); c.add("zero", -np.zeros(3))
    for k in range(20):
        c.add("tiny_1e-17", _unit(rng) * 1e-17)
    for a in range(3):
        for sgn in (1.0, -1.0):
            e = np.zeros(3); e[a] = sgn
            c.add("eps_exact", e * EPS)          # |v| == DBL_EPS exactly: not above it, identity
            c.add("eps_next", e * nxt)           # the next double: Rodrigues
            c.add("subnormal", e * 5e-324); c.add("subnormal", e * 1e-310)
            for ang in (0.5, np.pi / 2, np.pi, 1e-8, 100.0):
                c.add("axis", e * ang)
    for k in range(20):
        c.add("underflow_1e-170", _unit(rng) * 1e-170)   # the square underflows: theta = 0
        c.add("subnormal", rng.uniform(-1, 1, 3) * 1e-310)
    for ang, name in ((np.pi / 4, "pi/4"), (np.pi / 2, "pi/2"), (np.pi, "pi"), (3 * np.pi, "3pi"), (-3 * np.pi, "-3pi")):
        for k in range(40):
            c.add("angle_" + name, _unit(rng) * ang)
    for k in range(1000):  # random, |v| log-uniform up to 1e3
        c.add("random", _unit(rng) * 10.0 ** rng.uniform(-9, 3))
    v = np.stack(c.items)
    R = np.zeros((v.shape[0], 3, 3))
    for s in range(v.shape[0]):
        if s % 5 == 0:
            R[s] = np.eye(3)
        else:
            Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            R[s] = Q * np.sign(np.linalg.det(Q))
    return _freeze(v, R, np.array(c.labels))


def so3_exp_longdouble(v):
    """Rodrigues in numpy.longdouble from the double input: R = c I + (1 - c) a a^T + s hat(a), identity where |v| <= DBL_EPS (math_function.h:74-89)"""
    v = np.asarray(v, dtype=np.longdouble)
    th = np.sqrt((v * v).sum())
    if not th > np.longdouble(EPS):
        return np.eye(3, dtype=np.longdouble)
    a = v / th
    hat = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=np.longdouble)
    return np.cos(th) * np.eye(3, dtype=np.longdouble) + (1 - np.cos(th)) * np.outer(a, a) + np.sin(th) * hat


def so3_max_error(v, Rd):
    """largest elementwise |Rd[s] - longdouble Rodrigues(v[s])| over the systems, and the same per family is the caller's to take"""
    err = np.zeros(v.shape[0])
    for s in range(v.shape[0]):
        err[s] = float(np.abs(np.asarray(Rd[s], dtype=np.longdouble) - so3_exp_longdouble(v[s])).max())
    return err


def mat3_mul_model(A, B):
    """mat3_mul_dev / Eigen's lazy product coefficient order: (A[i,0] B[0,j] + A[i,1] B[1,j]) + A[i,2] B[2,j], batched (n, 3, 3)"""
    return (A[:, :, 0:1] * B[:, 0:1, :] + A[:, :, 1:2] * B[:, 1:2, :]) + A[:, :, 2:3] * B[:, 2:3, :]


# ---------------------------------------------------------------------------------------------
# wave sum: rows (n, 64)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wave_sum_cases():
    rng = np.random.default_rng(5305)
    c = _Cases()
    for k in range(300):   # magnitudes over 2^-40 .. 2^40, mixed signs: the association changes the bits
        c.add("wide", np.ldexp(rng.uniform(1.0, 2.0, 64), rng.integers(-40, 41, 64)) * rng.choice([-1.0, 1.0], 64))
    c.add("zeros", np.zeros(64))
    for l in range(64):    # a single non-zero, in each lane
        r = np.zeros(64); r[l] = rng.normal() * 10.0 ** rng.uniform(-5, 5)
        c.add("single", r)
    return _freeze(np.stack(c.items), np.array(c.labels))


def wave_sum_model(rows):
    """wave_sum_dpp (csrc/wave_solve.hpp) in numpy, add by add: row_shr 1, 2, 4, 8 with zero fill inside rows of 16 lanes, row_bcast15 (lane 15 of
    a row into the next row) into rows 1 and 3, row_bcast31 (lane 31) into rows 2 and 3; disabled rows and shifted-in lanes add +0.0.  Lane 63."""
    v = np.array(rows, dtype=np.float64).reshape(-1, 4, 16)
    for s in (1, 2, 4, 8):
        sh = np.zeros_like(v)
        sh[:, :, s:] = v[:, :, :-s]
        v = v + sh
    b = np.zeros_like(v)
    b[:, 1, :] = v[:, 0, 15:16]
    b[:, 3, :] = v[:, 2, 15:16]
    v = v + b
    b = np.zeros_like(v)
    b[:, 2, :] = v[:, 1, 15:16]
    b[:, 3, :] = v[:, 1, 15:16]
    v = v + b
    return v[:, 3, 15].copy()


# ---------------------------------------------------------------------------------------------
# the oracle over a whole set (one ctypes call per system; cached: the CPU and the GPU tests of one process share the results)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_plane_fit():
    from oracle import oracle as O
    A, _ = plane_fit_cases()
    b = -np.ones(5)
    return _freeze(np.stack([O.colpiv_qr_solve_5x3(A[s], b) for s in range(A.shape[0])]))


@functools.lru_cache(maxsize=None)
def oracle_svd3():
    from oracle import oracle as O
    A, _ = svd3_cases()
    out = [O.svd3(A[s]) for s in range(A.shape[0])]
    return _freeze(np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]))


@functools.lru_cache(maxsize=None)
def oracle_lu6():
    """(inv (n, 6, 6), det (n,), x (n, 6)); x is the tail's own product over the oracle's inverse: s = 0; s += inv[i, q] * b[q], q = 0..5"""
    from oracle import oracle as O
    H, b, _ = lu6_cases()
    with np.errstate(all="ignore"):
        out = [O.lu_inverse_6(H[s]) for s in range(H.shape[0])]
        inv = np.stack([o[0] for o in out]); det = np.array([o[1] for o in out])
        x = np.zeros((H.shape[0], 6))
        for q in range(6):
            x = x + inv[:, :, q] * b[:, q:q + 1]
    return _freeze(inv, det, x)


@functools.lru_cache(maxsize=None)
def oracle_so3():
    from oracle import oracle as O
    v, _, _ = so3_cases()
    return _freeze(np.stack([O.so3_exp(v[s]) for s in range(v.shape[0])]))


def same_bits(a, b, zero_sign_free=False, nan_free=False):
    """elementwise: the same 64 bits; optionally +0 == -0 and NaN == NaN (any payload, any sign)"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    same = a.view(np.uint64) == b.view(np.uint64)
    if zero_sign_free:
        same |= (a == 0.0) & (b == 0.0)
    if nan_free:
        same |= np.isnan(a) & np.isnan(b)
    return same
