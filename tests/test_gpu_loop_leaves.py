"""GPU: the leaf Gaussians of an NDT stage's target built on the device (csrc/kernels_loop_leaves.hpp) against LoopMatcher::build_target, through
fls_debug_loop_leaves (include/fls_debug_loop_leaves.h): every array on bits, n_leaves and sparse equal; cell and n_points also against the CPU
oracle's flo_ndt_leaves, as integers.  Then ndt_p2d_kernel on the tables the device build filled (fls_debug_loop_ndt_device) against the same kernel
on build_target's tables (fls_debug_loop_ndt), on bits.  Constructed targets: the smallest at which the build can go wrong."""
import ctypes as C

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib
from oracle import oracle as O
from tests import loop_cases as LC

pytestmark = pytest.mark.gpu

F32 = np.float32
FP, DP, IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"


def leaves(tgt, resolution, on_device):
    t = np.ascontiguousarray(tgt, F32)
    assert t.ndim == 2 and t.shape[1] == 3
    cap = max(t.shape[0] // 6 + 1, 1)
    cell, npts = np.full(cap, -7, np.int32), np.full(cap, -7, np.int32)
    mean, icov, cen = np.full((cap, 3), 7.0), np.full((cap, 9), 7.0), np.full((cap, 3), 7.0, F32)
    nl, sp = C.c_int32(-7), C.c_int32(-7)
    rc = _lib.lib().fls_debug_loop_leaves(0, t.ctypes.data_as(FP), t.shape[0], 3, resolution, on_device, cell.ctypes.data_as(IP), npts.ctypes.data_as(IP),
                                          mean.ctypes.data_as(DP), icov.ctypes.data_as(DP), cen.ctypes.data_as(FP), cap, C.byref(nl), C.byref(sp))
    assert rc == _lib.FLS_OK, (rc, _lib.status_string(rc))
    n = nl.value
    return {"n": n, "sparse": sp.value, "cell": cell[:n], "n_points": npts[:n], "mean": mean[:n], "icov": icov[:n], "centroid": cen[:n]}


def same_bits(a, b):
    if a["n"] != b["n"] or a["sparse"] != b["sparse"]:
        return False
    return (np.array_equal(a["cell"], b["cell"]) and np.array_equal(a["n_points"], b["n_points"]) and
            np.array_equal(a["mean"].view(np.uint64), b["mean"].view(np.uint64)) and np.array_equal(a["icov"].view(np.uint64), b["icov"].view(np.uint64)) and
            np.array_equal(a["centroid"].view(np.uint32), b["centroid"].view(np.uint32)))


def check(tgt, resolution, label, want_leaves=None, want_sparse=0):
    """device == host on bits, cell / n_points == the oracle's; the device build itself ran (counter 3), nothing was declined (counter 4)"""
    L = _lib.lib()
    before = [L.fls_loop_device_stat(0, 3), L.fls_loop_device_stat(0, 4)]
    host, dev = leaves(tgt, resolution, 0), leaves(tgt, resolution, 1)
    assert [L.fls_loop_device_stat(0, 3), L.fls_loop_device_stat(0, 4)] == [before[0] + 1, before[1]], label
    assert dev["n"] == host["n"] and dev["sparse"] == host["sparse"] == want_sparse, (label, dev["n"], host["n"], dev["sparse"], host["sparse"])
    assert same_bits(host, dev), label
    idx, nr = O.ndt_leaves(np.ascontiguousarray(tgt, F32), resolution)[:2]
    assert np.array_equal(idx.astype(np.int64), dev["cell"].astype(np.int64)), label
    # (the oracle keeps PCL's flag nr = -1 on a leaf whose covariance has a non-positive eigenvalue: such a leaf has a zero inverse covariance here)
    flagged = nr < 0
    assert np.array_equal(nr[~flagged].astype(np.int64), dev["n_points"][~flagged].astype(np.int64)), label
    assert (dev["icov"][flagged] == 0.0).all() and (dev["n_points"][flagged] >= 6).all(), label
    if want_leaves is not None:
        assert dev["n"] == want_leaves, (label, dev["n"])
    return dev


def in_cell(rng, cell, n, res=2.0):
    return ((np.asarray(cell, np.float64) + rng.uniform(0.05, 0.95, (n, 3))) * res).astype(F32)


def box_cloud(n, seed):
    """n points in a 40 m box: half of them uniform, half in clusters of 0.6 m, so that leaves of six points form at 2 m as well as at 10 m"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-18.0, 18.0, (max(n // 24, 1), 3))
    a = rng.uniform(-20.0, 20.0, (n // 2, 3))
    b = centres[rng.integers(0, len(centres), n - n // 2)] + rng.normal(0.0, 0.6, (n - n // 2, 3))
    c = np.clip(np.concatenate([a, b]), -20.0, 20.0).astype(F32)
    return c[rng.permutation(n)]


def test_one_point():
    check(np.array([[1.0, 2.0, 3.0]], F32), 2.0, "one point", want_leaves=0)
    check(np.array([[-1.0, 2.0, 3.0]], F32), 10.0, "one point, 10 m", want_leaves=0)


def test_cells_of_five_six_and_seven_points():
    rng = np.random.default_rng(1)
    t = np.concatenate([in_cell(rng, (0, 0, 0), 5), in_cell(rng, (1, 0, 0), 6), in_cell(rng, (2, 0, 0), 7)])
    d = check(t[rng.permutation(len(t))], 2.0, "5 | 6 | 7", want_leaves=2)
    assert list(d["n_points"]) == [6, 7] and list(d["cell"]) == [1, 2]


def test_coplanar_and_collinear_cells():
    """the eigenvalue floor: one eigenvalue clamped (a plane), two clamped (a line)"""
    rng = np.random.default_rng(2)
    plane = in_cell(rng, (0, 0, 0), 12)
    plane[:, 2] = F32(0.75)
    u = rng.uniform(0.1, 0.9, 9)
    line = (np.array([4.0, 4.0, 4.0]) + u[:, None] * np.array([1.5, 1.0, 0.5])).astype(F32)
    d = check(np.concatenate([plane, line]), 2.0, "plane + line", want_leaves=2)
    assert np.isfinite(d["icov"]).all() and np.abs(d["icov"][0]).max() > 0


def test_six_identical_points():
    """ev[2] <= 0: the leaf is searchable with a zero inverse covariance"""
    t = np.tile(np.array([[0.7, 1.1, -0.4]], F32), (6, 1))
    d = check(np.concatenate([t, np.array([[3.0, 3.0, 3.0]], F32)]), 2.0, "six identical", want_leaves=1)
    assert (d["icov"] == 0.0).all() and d["n_points"][0] == 6


def test_points_on_cell_faces():
    """coordinates that are whole multiples of the resolution, negative and positive: floorf decides the cell"""
    g = np.arange(-4.0, 5.0)
    x, y, z = np.meshgrid(g, g, np.array([-2.0, -1.5, -1.0, 0.0, 0.5, 1.0]), indexing="ij")
    t = np.stack([x, y, z], -1).reshape(-1, 3).astype(F32)
    d = check(t, 2.0, "faces, 2 m")
    assert d["n"] >= 16
    check(t * F32(5.0), 10.0, "faces, 10 m")


def test_non_finite_rows_are_skipped():
    t = box_cloud(257, 6).copy()
    clean = check(t, 10.0, "clean")
    bad = np.insert(t, [3, 100, 200], np.array([[np.nan, 0.0, 0.0], [1.0, np.inf, 2.0], [0.0, 1.0, -np.inf]], F32), axis=0)
    d = check(bad, 10.0, "NaN / Inf rows")
    assert same_bits(clean, d), "a non-finite row changes nothing"
    check(np.full((7, 3), np.nan, F32), 2.0, "no finite point", want_leaves=0)


@pytest.mark.parametrize("n", [63, 64, 65, 257, 4097])
def test_box_clouds(n):
    for res in (10.0, 2.0):
        d = check(box_cloud(n, n), res, f"{n} points at {res} m")
        if n >= 257:
            assert d["n"] > 0, (n, res)


def test_extent_beyond_int_max_cells():
    rng = np.random.default_rng(8)
    t = np.concatenate([in_cell(rng, (0, 0, 0), 8), np.array([[4000.0, 4000.0, 4000.0]], F32)])  # 2001^3 cells at 2 m
    check(t, 2.0, "dx dy dz > INT_MAX", want_leaves=0)
    check(t, 10.0, "the same cloud at 10 m: 401^3 cells, sparse", want_leaves=1, want_sparse=1)


def sparse_targets():
    _, t, _ = LC.chained_leaves()
    return (np.concatenate([t, np.array([[4000.0, 4000.0, 10.0]], F32)]), 2.0), (np.concatenate([t, np.array([[8000.0, 8000.0, 10.0]], F32)]), 3.0)


def test_sparse_leaf_table():
    """the open-addressing {cell, row} table is built on the device, not declined (check() asserts that counter 4 does not move)"""
    _, t, _ = LC.chained_leaves()
    for tgt, res in sparse_targets():
        dense = check(t, res, f"dense {res}")
        sparse = check(tgt, res, f"sparse {res}", want_sparse=1)
        assert sparse["n"] == dense["n"] > 0 and np.array_equal(sparse["n_points"], dense["n_points"])
        for k in ("mean", "icov", "centroid"):  # the stray point forms no leaf and does not change a sum
            assert np.array_equal(sparse[k], dense[k]), k


def test_sums_follow_cloud_order():
    """one target shuffled two ways: the device's bits differ where the host's differ and are equal where the host's are equal"""
    t = box_cloud(4097, 10)
    rng = np.random.default_rng(10)
    a, b = t[rng.permutation(len(t))], t[rng.permutation(len(t))]
    ha, hb, da, db = leaves(a, 10.0, 0), leaves(b, 10.0, 0), leaves(a, 10.0, 1), leaves(b, 10.0, 1)
    assert same_bits(ha, da) and same_bits(hb, db)
    assert np.array_equal(ha["cell"], hb["cell"]) and np.array_equal(da["cell"], db["cell"]) and np.array_equal(da["n_points"], db["n_points"])
    differs = 0
    for k, u in (("mean", np.uint64), ("icov", np.uint64), ("centroid", np.uint32)):
        host_eq, dev_eq = ha[k].view(u) == hb[k].view(u), da[k].view(u) == db[k].view(u)
        assert np.array_equal(host_eq, dev_eq), k
        differs += int((~host_eq).sum())
    assert differs > 0, "leaves of dozens of points: some sum depends on the order"


def _ndt(fn, src, tgt, resolution, p, want_hessian):
    s, t = np.ascontiguousarray(src, F32), np.ascontiguousarray(tgt, F32)
    p = np.ascontiguousarray(p, np.float64)
    score, pairs, lv, sp = C.c_double(7.0), C.c_int64(-7), C.c_int32(-7), C.c_int32(-7)
    g, H = np.full(6, 7.0), np.full(36, 7.0)
    rc = fn(0, s.ctypes.data_as(FP), s.shape[0], t.ctypes.data_as(FP), t.shape[0], 3, resolution, p.ctypes.data_as(DP), 1 if want_hessian else 0, C.byref(score),
            g.ctypes.data_as(DP), H.ctypes.data_as(DP), C.byref(pairs), C.byref(lv), C.byref(sp))
    assert rc == _lib.FLS_OK, rc
    return score.value, pairs.value, lv.value, sp.value, g.tobytes(), H.tobytes()


POSES = (np.zeros(6), LC.P_MOVED, -2.0 * LC.P_MOVED)


def test_ndt_kernel_reads_the_device_built_tables():
    """ndt_p2d_kernel over leaves built on the device == over build_target's leaves, on bits: the dense table (a box cloud at 10 and 2 m) and the
    sparse one, whose slots may differ while every look-up returns the same row"""
    L = _lib.lib()
    t = box_cloud(4097, 11)
    rng = np.random.default_rng(11)
    s = (t[rng.integers(0, len(t), 1500)] + rng.normal(0.0, 0.3, (1500, 3))).astype(F32)
    cs, ct, _ = LC.chained_leaves()
    cases = [(s, t, 10.0, 0), (s, t, 2.0, 0)] + [(cs, tgt, res, 1) for tgt, res in sparse_targets()]
    for src, tgt, res, sparse in cases:
        most = 0
        for p in POSES:
            for hess in (True, False):
                a, b = _ndt(L.fls_debug_loop_ndt, src, tgt, res, p, hess), _ndt(L.fls_debug_loop_ndt_device, src, tgt, res, p, hess)
                assert a == b, (res, sparse, hess, a[:4], b[:4])
                assert a[2] > 0 and a[3] == sparse, (res, a[2], a[3])
                most = max(most, a[1])
        assert most > 0, (res, "some (point, leaf) pair contributes at some pose")
