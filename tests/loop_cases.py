"""Inputs, hook wrappers and numpy models for tests/test_gpu_loop_stages.py (include/fls_debug_loop.h): small clouds that reach the branches
of csrc/kernels_loop.hpp and kernels_knn.hpp which the synthetic sub-maps of test_gpu_loop.py never or hardly reach.  Every cached array is
read-only: the tests share it."""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np

from funny_lidar_slam_amd import _lib
from oracle import oracle as O
from tests import loopdata

FP, DP, IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
F32 = np.float32

# prefixes of the source cloud: 1, 7, 8, 9 and 18 partial rows of 256 points, with and without a ragged last row
SIZES = (1, 255, 256, 257, 7 * 256, 8 * 256, 8 * 256 + 1, 17 * 256 + 5)
P_MOVED = np.array([0.3, -0.2, 0.05, 0.02, -0.015, 0.04])
X_MOVED = np.array([0.05, -0.03, 0.01, 0.004, -0.006, 0.008])
STRAY = np.array([[3000.0, 2000.0, 40.0], [-2500.0, 1800.0, -30.0], [2999.0, 2001.0, 41.0]], F32)  # (test_gpu_loop.py's stray points)


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def base_pair():
    src, tgt, _ = loopdata.make_pair(job=3, n_az=120, n_t=2, n_s=2)
    return _ro(src), _ro(tgt)


@functools.lru_cache(maxsize=None)
def filtered(leaf_src, leaf_tgt):
    """the base pair after VoxelGridCloud, xyz only: (0.6, 0.6) for the NDT stages, (0.5, 0.4) as GICP takes them"""
    src, tgt = base_pair()
    return _ro(O.voxel_grid(src, leaf_src)[:, :3]), _ro(O.voxel_grid(tgt, leaf_tgt)[:, :3])


# ---- hooks ----------------------------------------------------------------------------------------------------------------------------
def _f(a):
    a = np.ascontiguousarray(a, F32)
    assert a.ndim == 2 and a.shape[1] >= 3
    return a, a.ctypes.data_as(FP), a.shape[0], a.shape[1]


def _ok(rc, what):
    assert rc == _lib.FLS_OK, (what, rc, _lib.status_string(rc))


def ndt(src, tgt, resolution, p, want_hessian=True):
    s, ps, ns, st = _f(src)
    t, pt, nt, st2 = _f(tgt)
    assert st == st2
    p = np.ascontiguousarray(p, np.float64)
    score, pairs, leaves, sparse = C.c_double(7.0), C.c_int64(-7), C.c_int32(-7), C.c_int32(-7)
    g, H = np.full(6, 7.0), np.full(36, 7.0)
    _ok(_lib.lib().fls_debug_loop_ndt(0, ps, ns, pt, nt, st, resolution, p.ctypes.data_as(DP), 1 if want_hessian else 0, C.byref(score), g.ctypes.data_as(DP),
                                      H.ctypes.data_as(DP), C.byref(pairs), C.byref(leaves), C.byref(sparse)), "fls_debug_loop_ndt")
    return {"score": score.value, "grad": g, "hess": H.reshape(6, 6, order="F"), "pairs": pairs.value, "leaves": leaves.value, "sparse": sparse.value}


def gicp_cov(cloud, cell=1.5, eps=0.001, host_grid=0):
    c, pc, n, st = _f(cloud)
    out = np.full((n, 9), np.nan)
    _ok(_lib.lib().fls_debug_loop_gicp_cov(0, pc, n, st, cell, eps, host_grid, out.ctypes.data_as(DP)), "fls_debug_loop_gicp_cov")
    return out.reshape(n, 3, 3).transpose(0, 2, 1)


def _colmajor(M):
    """(n, 3, 3) matrices -> (n, 9) column-major rows"""
    return np.ascontiguousarray(np.asarray(M, np.float64).transpose(0, 2, 1).reshape(-1, 9))


def gicp_corr(moved, tgt, T, R, cov_src, cov_tgt, corr_dist, host_grid=0):
    s, ps, ns, st = _f(moved)
    t, pt, nt, st2 = _f(tgt)
    assert st == st2
    Tf = np.ascontiguousarray(np.asarray(T, F32).T).reshape(-1).copy()
    Rd = np.ascontiguousarray(np.asarray(R, np.float64).T).reshape(-1).copy()
    c1, c2 = _colmajor(cov_src), _colmajor(cov_tgt)
    assert c1.shape == (ns, 9) and c2.shape == (nt, 9)
    corr, mahal = np.full(ns, -7, np.int32), np.full((ns, 9), 7.0)
    _ok(_lib.lib().fls_debug_loop_gicp_corr(0, ps, ns, pt, nt, st, Tf.ctypes.data_as(FP), Rd.ctypes.data_as(DP), c1.ctypes.data_as(DP), c2.ctypes.data_as(DP), corr_dist,
                                            host_grid, corr.ctypes.data_as(IP), mahal.ctypes.data_as(DP)), "fls_debug_loop_gicp_corr")
    return corr, mahal.reshape(ns, 3, 3).transpose(0, 2, 1)


def gicp_fdf(moved, tgt, x, corr, mahal, want_grad=True):
    s, ps, ns, st = _f(moved)
    t, pt, nt, st2 = _f(tgt)
    assert st == st2
    x = np.ascontiguousarray(x, np.float64)
    corr = np.ascontiguousarray(corr, np.int32)
    m = _colmajor(mahal) if ns else np.zeros((1, 9))
    v = np.full(14 if want_grad else 2, 7.0)
    _ok(_lib.lib().fls_debug_loop_gicp_fdf(0, ps, ns, pt, nt, st, x.ctypes.data_as(DP), corr.ctypes.data_as(IP), m.ctypes.data_as(DP), 1 if want_grad else 0,
                                           v.ctypes.data_as(DP)), "fls_debug_loop_gicp_fdf")
    return v


def fitness(src, tgt, T, host_grid=0):
    s, ps, ns, st = _f(src)
    t, pt, nt, st2 = _f(tgt)
    assert st == st2
    Tf = np.ascontiguousarray(np.asarray(T, F32).T).reshape(-1).copy()
    total, count = C.c_double(7.0), C.c_int64(-7)
    _ok(_lib.lib().fls_debug_loop_fitness(0, ps, ns, pt, nt, st, Tf.ctypes.data_as(FP), host_grid, C.byref(total), C.byref(count)), "fls_debug_loop_fitness")
    return total.value, count.value


# ---- float models of the host's pose algebra (LoopMatcher::rot / mul / apply_state) ------------------------------------------------------
_libm = C.CDLL("libm.so.6")
_libm.cosf.restype = _libm.sinf.restype = C.c_float
_libm.cosf.argtypes = _libm.sinf.argtypes = [C.c_float]


def _rot(axis, angle):
    """AngleAxisf(angle, unit axis) as LoopMatcher::rot: the C library's cosf / sinf of float(angle)"""
    r = np.eye(4, dtype=F32)
    a = F32(angle)
    c, s = F32(_libm.cosf(a)), F32(_libm.sinf(a))
    i, j = (axis + 1) % 3, (axis + 2) % 3
    r[i, i] = c; r[j, j] = c; r[j, i] = s; r[i, j] = -s
    return r


def _mul(a, b):
    """LoopMatcher::mul: ((a0 b0 + a1 b1) + a2 b2) + a3 b3 in float"""
    r = np.zeros((4, 4), F32)
    for j in range(4):
        for i in range(4):
            r[i, j] = F32(F32(F32(a[i, 0] * b[0, j]) + F32(a[i, 1] * b[1, j])) + F32(a[i, 2] * b[2, j])) + F32(a[i, 3] * b[3, j])
    return r


def apply_state(x):
    """LoopMatcher::apply_state(identity, x): R = Rz(x5) Ry(x4) Rx(x3), translation float(x0..2)"""
    R = _mul(_mul(_rot(2, x[5]), _rot(1, x[4])), _rot(0, x[3]))
    t = np.eye(4, dtype=F32)
    o = np.eye(4, dtype=F32)
    for j in range(3):
        for i in range(3):
            o[i, j] = F32(F32(R[i, 0] * t[0, j]) + F32(R[i, 1] * t[1, j])) + F32(R[i, 2] * t[2, j])
    for a in range(3):
        o[a, 3] = t[a, 3] + F32(x[a])
    return o


def xform(T, c):
    """loop_xform: c0 * x + (c1 * y + (c2 * z + c3)) in float"""
    T = np.asarray(T, F32)
    c = np.asarray(c, F32)
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    return np.stack([T[i, 0] * x + (T[i, 1] * y + (T[i, 2] * z + T[i, 3])) for i in range(3)], axis=1)


# ---- numpy models ---------------------------------------------------------------------------------------------------------------------
def nearest(q, tgt, chunk=512):
    """1-NN by brute force: float ((dx*dx + dy*dy) + dz*dz), lowest (d2, index) -> (index, d2)"""
    q, tgt = np.asarray(q, F32), np.asarray(tgt, F32)
    idx, d2 = np.zeros(len(q), np.int64), np.zeros(len(q), F32)
    for a in range(0, len(q), chunk):
        b = q[a:a + chunk]
        dx, dy, dz = (b[:, None, k] - tgt[None, :, k] for k in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == F32
        i = np.argmin(d, axis=1)  # (the first minimum: the lowest index among equal distances)
        idx[a:a + chunk] = i
        d2[a:a + chunk] = d[np.arange(len(b)), i]
    return idx, d2


def corr_model(moved, tgt, T, corr_dist):
    idx, d2 = nearest(xform(T, moved), tgt)
    return np.where(d2.astype(np.float64) < corr_dist * corr_dist, idx, -1).astype(np.int32)


def mahal_model(corr, R, cov_src, cov_tgt):
    R = np.asarray(R, np.float64)
    M = np.full((len(corr), 3, 3), np.nan)
    k = np.flatnonzero(corr >= 0)
    M[k] = np.linalg.inv(cov_tgt[corr[k]] + R @ cov_src[k] @ R.T)
    return M


def fdf_model(moved, tgt, x, corr, mahal):
    """the terms of gicp_fdf_kernel in its arithmetic, added exactly: (sums[14], sums of |term|[14], m)"""
    k = np.flatnonzero(np.asarray(corr) >= 0)
    moved, tgt = np.asarray(moved, F32), np.asarray(tgt, F32)
    sums, mags = np.zeros(14), np.zeros(14)
    if len(k) == 0:
        return sums, mags, 0
    pp = xform(apply_state(x), moved[k])
    res = (pp - tgt[np.asarray(corr)[k], :3]).astype(np.float64)  # (float subtraction)
    assert pp.dtype == F32
    M = np.asarray(mahal, np.float64)[k]
    tmp = np.stack([(M[:, r, 0] * res[:, 0] + M[:, r, 1] * res[:, 1]) + M[:, r, 2] * res[:, 2] for r in range(3)], axis=1)
    p3 = moved[k, :3].astype(np.float64)
    cols = [(res[:, 0] * tmp[:, 0] + res[:, 1] * tmp[:, 1]) + res[:, 2] * tmp[:, 2]] + [tmp[:, a] for a in range(3)]
    cols += [p3[:, q % 3] * tmp[:, q // 3] for q in range(9)]  # Racc[rr + 3 cc] = p[rr] * tmp[cc]
    cols.append(np.ones(len(k)))
    for c, col in enumerate(cols):
        sums[c] = math.fsum(col)
        mags[c] = math.fsum(np.abs(col))
    return sums, mags, len(k)


def f_and_g(v, x):
    """f and the gradient from the reduced row as LoopMatcher::gicp_fdf forms them"""
    m = v[13]
    f = v[0] / m
    g = np.zeros(6)
    g[:3] = v[1:4] * (2.0 / m)
    Racc = (v[4:13] * (2.0 / m)).reshape(3, 3, order="F")
    cphi, sphi, cth, sth, cpsi, spsi = math.cos(x[3]), math.sin(x[3]), math.cos(x[4]), math.sin(x[4]), math.cos(x[5]), math.sin(x[5])
    dphi = np.array([0.0, 0.0, 0.0, sphi * spsi + cphi * cpsi * sth, -cpsi * sphi + cphi * spsi * sth, cphi * cth,
                     cphi * spsi - cpsi * sphi * sth, -cphi * cpsi - sphi * spsi * sth, -cth * sphi]).reshape(3, 3, order="F")
    dth = np.array([-cpsi * sth, -spsi * sth, -cth, cpsi * cth * sphi, cth * sphi * spsi, -sphi * sth, cphi * cpsi * cth, cphi * cth * spsi,
                    -cphi * sth]).reshape(3, 3, order="F")
    dpsi = np.array([-cth * spsi, cpsi * cth, 0.0, -cphi * cpsi - sphi * spsi * sth, -cphi * spsi + cpsi * sphi * sth, 0.0,
                     cpsi * sphi - cphi * spsi * sth, sphi * spsi + cphi * cpsi * sth, 0.0]).reshape(3, 3, order="F")
    for a, d in enumerate((dphi, dth, dpsi)):
        g[3 + a] = np.trace(d @ Racc)
    return f, g


def cov_numpy(cloud):
    """20-NN covariances in float64 numpy, independent of the oracle: brute-force neighbours in (d2, index) order, np.cov, numpy's SVD.
    -> (C (n, 3, 3) with singular values (1, 1, 0.001), mask of the points whose normal is separated: S1 - S2 > 1e-3 S0)"""
    c = np.asarray(cloud, F32)
    n = len(c)
    Cn, sep = np.zeros((n, 3, 3)), np.zeros(n, bool)
    for a in range(0, n, 256):
        b = c[a:a + 256]
        dx, dy, dz = (b[:, None, k] - c[None, :, k] for k in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        nn = np.argsort(d, axis=1, kind="stable")[:, :20]
        for r in range(len(b)):
            P = c[nn[r]].astype(np.float64)
            U, S, _ = np.linalg.svd(np.cov(P.T, bias=True))
            Cn[a + r] = U @ np.diag([1.0, 1.0, 0.001]) @ U.T
            sep[a + r] = S[1] - S[2] > 1e-3 * S[0]
    return Cn, sep


# ---- covariance clouds -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cov_cloud(name):
    rng = np.random.default_rng(20)
    if name == "submap":      # the first 1500 points in voxel order, a thin slice: 20th neighbours 1 .. 50 m away, rho = 1 .. 19 and beyond
        c = filtered(0.5, 0.4)[0][:1500]
    elif name == "patch":     # the 1500 points around the middle of the same cloud: the ordinary case, rho = 1 certifies 85 %, rho = 2 the rest
        full = filtered(0.5, 0.4)[0]
        near = np.argsort(((full - np.median(full, axis=0)) ** 2).sum(axis=1), kind="stable")[:1500]
        c = full[np.sort(near)]
    elif name == "lattice":   # exact distance ties at the 20th / 21st neighbour throughout
        g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
        c = (g * 0.25).astype(F32)
    elif name == "crowded":   # one 1.5 m cell with 1100 points: total > kCovMaxCand, lane 0's serial search
        c = np.concatenate([rng.uniform(0.0, 1.5, (1100, 3)), rng.uniform(-6.0, 6.0, (300, 3))]).astype(F32)
    elif name == "isolated":  # two points 50 - 60 m from a slab: rho grows 4, 6, 9, 13 .. until the block is the whole window
        slab = rng.uniform(-3.0, 3.0, (400, 3)) * [1.0, 1.0, 0.05]
        c = np.concatenate([slab, [[50.0, 5.0, 1.0], [-8.0, 60.0, -2.0]]]).astype(F32)
    elif name in ("20", "21"):
        c = (rng.uniform(-1.0, 1.0, (int(name), 3)) * [1.0, 1.0, 0.1]).astype(F32)
    else:
        raise KeyError(name)
    return _ro(c)


@functools.lru_cache(maxsize=None)
def cov_reference(name):
    """(oracle covariances, numpy covariances, separated-normal mask) of a covariance cloud"""
    c = cov_cloud(name)
    Co = O.gicp_covariances(c, 20, 0.001)
    Cn, sep = cov_numpy(c)
    return _ro(Co), _ro(Cn), _ro(sep)


@functools.lru_cache(maxsize=None)
def gicp_covs():
    """oracle covariances of the GICP pair (inputs of the correspondence stage)"""
    s, t = filtered(0.5, 0.4)
    return _ro(O.gicp_covariances(s, 20, 0.001)), _ro(O.gicp_covariances(t, 20, 0.001))


# ---- sparse leaf table -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chained_leaves():
    """(source, target, strays) at resolution 3: 500 leaves of 7 points each in cells scattered over 192 x 192 x 24 m, so that nearly every occupied
    cell is a leaf and their cell indices are spread: in the 2048 slots of the sparse form's open-addressing table probe chains form, which the 311
    leaves of the sub-map in 4096 slots do not"""
    rng = np.random.default_rng(77)
    cells = np.unique(rng.integers(0, [64, 64, 8], (500, 3)), axis=0)
    tgt = (cells[:, None, :] * 3.0 + rng.uniform(0.1, 2.9, (len(cells), 7, 3))).reshape(-1, 3).astype(F32)
    src = (tgt[rng.integers(0, len(tgt), 1500)] + rng.uniform(-1.5, 1.5, (1500, 3))).astype(F32)
    return _ro(src), _ro(tgt), _ro(STRAY * F32(2.0))


def leaf_table_displaced(tgt, resolution):
    """model of LoopMatcher::build_target's sparse table: (slots, leaves that do not sit in their home slot)"""
    tgt = np.asarray(tgt, F32)
    inv = F32(1.0) / F32(resolution)
    lo = np.floor(tgt.min(axis=0) * inv)
    div = (np.floor(tgt.max(axis=0) * inv) - lo + 1).astype(np.int64)
    c = (np.floor(tgt * inv) - lo).astype(np.int64)
    cell, count = np.unique(c[:, 0] + c[:, 1] * div[0] + c[:, 2] * div[0] * div[1], return_counts=True)
    leaves = [int(v) for v in cell[count >= 6]]
    assert leaves == [int(v) for v in O.ndt_leaves(tgt, resolution)[0]], "the cell index of this model is the oracle's"
    slots = 1024
    while slots < 2 * len(cell) + 2:
        slots <<= 1
    table, displaced = {}, 0
    for v in leaves:  # ascending cell index, linear probing
        h = home = (v * 2654435761) & 0xffffffff & (slots - 1)
        while h in table:
            h = (h + 1) & (slots - 1)
        table[h] = v
        displaced += h != home
    return slots, displaced
