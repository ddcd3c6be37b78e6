"""The integer bookkeeping around the iVox kNN candidate scan (csrc/kernels_ivox_coop.hpp: the two-run candidate window, the packed
probe offsets, the predicated voxel-table build, the ungated / 32-bit-offset form) against the CPU oracle on small hand-built maps.

Every case runs PointToPlane_IVOX with max_iterations 1, 2 and 3 on the same inputs as the oracle, with the brick image and with the
hash-table fall-back (FLS_IVOX_DENSE=0), with the product kernel and with its counting variant: counts, valid flags and neighbour ids
through tests/util.assert_same_registration with NO tie budget, the three traffic counters exactly.  The coordinates are jittered so
that the reference side has no exact distance tie; test_cases_have_no_distance_tie checks that on the CPU for every case."""
import functools

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg
from tests import util

MODE = "PointToPlane_IVOX"
ITERS = (1, 2, 3)


def _pose(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4); T[:3, :3] = Rz @ Ry @ Rx; T[:3, 3] = t
    return T


T_GT = _pose(0.004, -0.003, 0.006, [0.04, -0.03, 0.02])  # the scan is the scene seen from T_GT; every Match starts from the identity


def _to_scan(world):
    """world points -> the body frame of T_GT (float32, as the matcher receives them)"""
    R, t = T_GT[:3, :3], T_GT[:3, 3]
    return np.ascontiguousarray(((np.asarray(world, np.float64) - t) @ R).astype(np.float32))


def _scene(rng, dens, peak):
    """Floor z = 0 over [-4, 4]^2 and two walls (x = 4, y = -4; 3 m high) sampled at dens(u, v) points per m^2 (u, v: the plane's own
    coordinates in [-4, 4] x ...), 5 mm of noise along the normal: three plane orientations, negative and positive coordinates, voxels on
    brick faces, edges and corners (the 4 m bricks meet at the origin, the floor is the z-face of its bricks)."""
    def plane(lo, hi):
        n = int(rng.poisson(peak * (hi[0] - lo[0]) * (hi[1] - lo[1])))
        uv = rng.uniform(lo, hi, (n, 2))
        keep = rng.uniform(0.0, peak, n) < np.array([dens(u, v) for u, v in uv])
        return uv[keep], rng.normal(0.0, 0.005, int(keep.sum()))
    out = []
    uv, w = plane((-4.0, -4.0), (4.0, 4.0)); out.append(np.c_[uv[:, 0], uv[:, 1], w])
    uv, w = plane((-4.0, 0.3), (4.0, 3.0)); out.append(np.c_[4.0 + w, uv[:, 0], uv[:, 1]])
    uv, w = plane((-4.0, 0.3), (4.0, 3.0)); out.append(np.c_[uv[:, 0], -4.0 + w, uv[:, 1]])
    return np.vstack(out)


def _case_sparse_runs(n_scan=700, seed=11):
    """1.5 points per voxel on average: neighbouring voxels hold 1, 1, 2, 1, 3 ... points, a quad of candidates spans three to five runs
    (the two-run cut ends nearly every trip early); candidate totals from 1 up to about 30, none a multiple of anything in particular."""
    rng = np.random.default_rng(seed)
    m = _scene(rng, lambda u, v: 6.0, 6.0)
    s = _scene(rng, lambda u, v: 6.0, 6.0)
    s = s[rng.permutation(len(s))[:n_scan]]
    return dict(map=m.astype(np.float32), scans=[_to_scan(s)])


def _case_density_ramp():
    """2 to 160 points per m^2 across the scene: runs of 1 next to runs of 40, totals from a handful to several hundred"""
    rng = np.random.default_rng(12)
    m = _scene(rng, lambda u, v: 2.0 + 158.0 * ((u + 4.0) / 8.0) ** 3, 160.0)
    s = _scene(rng, lambda u, v: 9.0, 9.0)
    return dict(map=m.astype(np.float32), scans=[_to_scan(s[:1601])])


def _case_all19_dense():
    """A 3 m cube filled at 400 points per m^3 (50 per voxel, every voxel above 20) below the floor at negative coordinates: queries
    in its middle hit all 19 voxels, more than 400 candidates each; the scene around it keeps the registration well posed."""
    rng = np.random.default_rng(13)
    blob = rng.uniform([-3.5, -3.5, -3.6], [-0.5, -0.5, -0.6], (10800, 3))
    m = np.vstack([_scene(rng, lambda u, v: 12.0, 12.0), blob])
    q = rng.uniform([-2.6, -2.6, -2.7], [-1.4, -1.4, -1.5], (150, 3))
    s = np.vstack([_scene(rng, lambda u, v: 5.0, 5.0)[:900], q])
    return dict(map=m.astype(np.float32), scans=[_to_scan(s[rng.permutation(len(s))])])


def _case_few_none_far():
    """Islands of 1, 2, 3 and 4 map points in one voxel with queries next to them (count < 5), queries with no candidate at all, one query
    beyond the key range -- and a second Match on the same handle in which a third of the points has moved away from the map: their
    previous lists must survive (Q15)."""
    rng = np.random.default_rng(14)
    isl, qs = [], []
    for j in range(1, 5):
        c = np.array([20.0 + 5.0 * j, 20.0, 1.0])
        isl.append(c + rng.uniform(-0.12, 0.12, (j, 3)))
        qs.append(c + rng.uniform(-0.2, 0.2, (5, 3)))
    m = np.vstack([_scene(rng, lambda u, v: 10.0, 10.0)] + isl)
    far = np.array([100.0, 50.0, 3.0]) + rng.uniform(-5.0, 5.0, (12, 3))
    beyond = np.array([[6.0e5, 1.0, 2.0]])  # |key| = 1.2e6 > 2^20 - 2
    s = np.vstack([_scene(rng, lambda u, v: 5.0, 5.0)[:800]] + qs + [far])
    s = np.vstack([s[rng.permutation(len(s))], beyond])
    s1 = _to_scan(s)
    s2 = s1.copy()
    s2[::3, 1] += np.float32(200.0)
    return dict(map=m.astype(np.float32), scans=[s1, s2])


CASES = {
    "sparse_runs": _case_sparse_runs,
    "density_ramp": _case_density_ramp,
    "all19_dense": _case_all19_dense,
    "few_none_far": _case_few_none_far,
    "scan_of_1": functools.partial(_case_sparse_runs, 1, 21),
    "scan_of_63": functools.partial(_case_sparse_runs, 63, 22),
    "scan_of_65": functools.partial(_case_sparse_runs, 65, 23),
}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return CASES[name]()


def _yaml(iters):
    return dict(reg.YAML_NCLT_IVOX, optimization_iter_num=iters)


class _Snap:
    """what assert_same_registration reads from an oracle, frozen after one Match (the oracle goes on to the next Match of the sequence)"""

    def __init__(self, o, ok, T):
        self.ok, self.T = ok, T
        self.stats = type(o.stats)()
        for f, _ in o.stats._fields_:
            setattr(self.stats, f, getattr(o.stats, f))
        self._log, self._corr, self._tie = o.iteration_log(), o.correspondences(0), o.tie_rows()
        c = o.counters()
        self.traffic = (int(c.probes), int(c.hit_voxels), int(c.cand_points))
        self.tie_queries = int(c.tie_queries)

    def iteration_log(self):
        return self._log

    def correspondences(self, slot=0):
        return self._corr

    def tie_rows(self):
        return self._tie


@functools.lru_cache(maxsize=None)
def _reference(name, iters):
    """the oracle's Matches of a case (computed once, shared by the brick-image and hash-table runs; never modified)"""
    inp = _inputs(name)
    o = util.oracle_for(MODE, _yaml(iters))
    o.AddCloudToLocalMap(inp["map"])
    out = []
    for scan in inp["scans"]:
        ok, T = o.Match(scan, np.eye(4), update_map=False)
        out.append(_Snap(o, ok, T))
    o.close()
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_have_no_distance_tie(name):
    """no GPU needed: the oracle marks no row of any case as decided by an exact distance tie (the GPU comparisons carry no tie budget)"""
    inp = _inputs(name)
    for iters in ITERS:
        for k, snap in enumerate(_reference(name, iters)):
            assert snap.tie_queries == 0, (name, iters, k, snap.tie_queries)
            assert snap._tie is None or not snap._tie.any(), (name, iters, k, int(snap._tie.sum()))
            assert snap.stats.n_source == inp["scans"][k].shape[0]
    # the case is what its name says (counts from the oracle's last run: 3 iterations, first Match)
    cnt = _reference(name, 3)[0].correspondences(0)[1]
    if name == "few_none_far":
        assert set(np.unique(cnt)) >= {0, 1, 2, 3, 4, 5}
    if name.startswith("scan_of_"):
        assert len(cnt) == int(name.rsplit("_", 1)[1])


@pytest.fixture(scope="module")
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"


@pytest.mark.gpu
@pytest.mark.parametrize("dense", [True, False], ids=["bricks", "hash"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_knn_bookkeeping_equals_the_oracle(_need_gpu, monkeypatch, name, dense):
    if not dense:
        monkeypatch.setenv("FLS_IVOX_DENSE", "0")
    inp = _inputs(name)
    for iters in ITERS:
        ref = _reference(name, iters)
        for counting in (False, True):  # the product kernel, then its counting variant
            m = reg.make_matcher(MODE, _yaml(iters))
            try:
                m.AddCloudToLocalMap([inp["map"]])
                m.set_profiling(False, counters=counting)
                for k, scan in enumerate(inp["scans"]):
                    T = np.eye(4)
                    ok = m.Match(reg.PointcloudCluster(planar_cloud_=scan), T, update_map=False)
                    util.assert_same_registration(m, ref[k], ok, T, ref[k].ok, ref[k].T, sets_only_tail=True, max_tie_rows=0)
                    if counting:
                        assert m.traffic_counters() == ref[k].traffic, (name, iters, k, m.traffic_counters(), ref[k].traffic)
            finally:
                m.close()
