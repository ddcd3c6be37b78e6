"""fls_match_batch_shared_ivox (include/fls_batch_ivox.h): groups of PointToPlane_IVOX jobs in shared launches, one ivox_knn_jobs_kernel launch and
one p2plane_fit_solve_jobs_kernel launch per fit class and iteration.  Every comparison is against a FRESH handle's Match(..., update_map=False) on
the same map (never the shared path against itself): the return value, the pose bits, stats.iterations and stats.n_valid.
Shapes: synth.make_config(1, job=j, scale=0.05) -- a 64 x 90 = 5,760-point scan (128 kNN workgroups, 23 fit rows) and a 50k-point map."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg, synth
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODE, Y = "PointToPlane_IVOX", reg.YAML_NCLT_IVOX


def knn_blocks(n):
    """csrc/matcher_p2plane_ivox.hpp knn_grid_blocks: ceil(n / 64) rounded up to a multiple of 8 * kIvoxXcdChunk = 64"""
    return ((n + 63) // 64 + 63) // 64 * 64


def fit_class(n):
    """threads of a fit workgroup, as match_prepare chooses them"""
    return 256 if n <= 65536 else 512


def yaw_pose(dx, dy, yaw):
    T = np.eye(4)
    c, s = np.cos(yaw), np.sin(yaw)
    T[:2, :2] = [[c, -s], [s, c]]
    T[0, 3], T[1, 3] = dx, dy
    return T


class World:
    """The map, the scans and the fresh-handle results, computed once for the module and never changed."""

    def __init__(self):
        cfg0 = synth.make_config(1, job=0, scale=0.05)
        self.map = cfg0["map"]
        self.scans = [cfg0["scan"]] + [synth.make_config(1, job=j, scale=0.05, with_map=False)["scan"] for j in range(1, 5)]
        self._fresh = {}

    def owner(self, **kw):
        m = reg.make_matcher(MODE, Y, **kw)
        m.AddCloudToLocalMap([self.map])
        return m

    def fresh(self, scan, T0):
        """(ok, pose bytes, iterations, n_valid, n_source) of a fresh handle's Match(scan, T0, update_map=False)"""
        key = (scan.tobytes(), np.asarray(T0, np.float64).tobytes())
        if key not in self._fresh:
            f = self.owner()
            T = np.array(T0, dtype=np.float64)
            ok = f.Match(util.cluster_for(MODE, scan), T, update_map=False)
            self._fresh[key] = (ok, T.tobytes(), f.stats.iterations, f.stats.n_valid, f.stats.n_source)
            f.close()
        return self._fresh[key]


@pytest.fixture(scope="module")
def world(built):
    return World()


def table(oks, Ts, stats):
    return [(bool(oks[j]), np.ascontiguousarray(Ts[j]).tobytes(), stats[j].iterations, stats[j].n_valid) for j in range(len(oks))]


def clusters_of(scans):
    return [util.cluster_for(MODE, s) for s in scans]


def assert_equal_fresh(world, got, scans, T_inits, skip=()):
    for j, (s, T0) in enumerate(zip(scans, T_inits)):
        if j not in skip:
            assert got[j] == world.fresh(s, T0)[:4], j


def ivox_stats(m):
    return [m.BatchIvoxStat(k) for k in range(5)]


def test_groups_equal_fresh_matchers(world):
    """5 jobs on 3 slots = groups of 3 and 2: every job equals its fresh handle and MatchBatch(lanes=1), all five ran in shared launches, and the kNN
    launches queued are fewer than the jobs' iterations (a group costs its longest job, not the sum); one fit class = one fit launch per kNN launch."""
    scans, T0 = world.scans[:5], [np.eye(4)] * 5
    m = world.owner()
    got = table(*m.MatchBatchSharedIvox(clusters_of(scans), T0, slots=3))
    assert m.batch_rc >= 0 and all(s >= 0 for s in m.batch_status)
    counters = ivox_stats(m)
    back_to_back = table(*m.MatchBatch(clusters_of(scans), T0, lanes=1))
    assert_equal_fresh(world, got, scans, T0)
    assert got == back_to_back
    total_iterations = sum(r[2] for r in got)
    print("counters", counters, "iterations", [r[2] for r in got])
    assert counters[2] == 5 and counters[3] == 0 and counters[4] == 2
    assert 0 < counters[0] < total_iterations
    assert counters[1] == counters[0]
    assert all(m.BatchStat(k) == 0 for k in range(4))  # the fused batch's counters are not this entry point's
    assert m.BatchIvoxStat(5) == 0 and m.BatchIvoxStat(-1) == 0
    m.close()


def test_mixed_grids_and_iteration_counts_in_one_group(world):
    """One group holds the full scan (128 kNN workgroups, 23 fit rows), every second point of it (64 and 12), the full scan from the fresh handle's own
    result (stops at once) and from a pose the fresh handle cannot register within optimization_iter_num.  That pose was chosen on the CPU oracle: 29 m
    along x and y and 2 rad of yaw from the result leave about 30 valid points after all ten iterations (n_valid < 50: FLS_NOT_CONVERGED)."""
    full, half = world.scans[0], world.scans[0][::2].copy()
    found = np.frombuffer(world.fresh(full, np.eye(4))[1], np.float64).reshape(4, 4)
    far = found @ yaw_pose(29.0, 29.0, 2.0)
    scans = [full, half, full, full]
    T0 = [np.eye(4), np.eye(4), found, far]
    ref = [world.fresh(s, T) for s, T in zip(scans, T0)]
    print("fresh: ok, iterations, n_valid, n_source", [(r[0], r[2], r[3], r[4]) for r in ref])
    # without these the group would not mix anything
    assert ref[0][4] == 5760 and ref[1][4] == 2880
    assert {knn_blocks(r[4]) for r in ref} == {128, 64}
    assert len({r[2] for r in ref}) >= 3
    assert ref[2][2] <= 2
    assert ref[3][2] == Y["optimization_iter_num"] and not ref[3][0]
    m = world.owner()
    got = table(*m.MatchBatchSharedIvox(clusters_of(scans), T0, slots=4))
    assert ivox_stats(m)[2:] == [4, 0, 1]  # all four shared their launches
    assert m.BatchIvoxStat(0) >= Y["optimization_iter_num"]
    assert_equal_fresh(world, got, scans, T0)
    assert m.batch_status[3] == _lib.FLS_NOT_CONVERGED and m.batch_rc == _lib.FLS_OK
    m.close()


def test_both_fit_classes_in_one_group(world):
    """A 69,120-point job (twelve copies of the scan, each shifted by a few millimetres: 512-thread fit workgroups) beside two 5,760-point jobs
    (256-thread ones): two fit launches per iteration, each job with the workgroup size and therefore the bits of its single-job Match."""
    base = world.scans[0]
    step = np.zeros(base.shape[1], base.dtype)
    step[:3] = (0.002, -0.003, 0.001)
    big = np.concatenate([base + k * step for k in range(12)]).astype(base.dtype)
    scans = [world.scans[1], big, world.scans[2]]
    T0 = [np.eye(4)] * 3
    ref = [world.fresh(s, T) for s, T in zip(scans, T0)]
    print("fresh: ok, iterations, n_valid, n_source", [(r[0], r[2], r[3], r[4]) for r in ref])
    assert [fit_class(r[4]) for r in ref] == [256, 512, 256] and ref[1][4] == 69120
    m = world.owner()
    got = table(*m.MatchBatchSharedIvox(clusters_of(scans), T0, slots=3))
    assert_equal_fresh(world, got, scans, T0)
    c = ivox_stats(m)
    print("counters", c)
    assert c[2:] == [3, 0, 1]
    assert 0 < c[0] < c[1] <= 2 * c[0]
    m.close()


def test_job_below_the_n_valid_floor_and_an_empty_job(world):
    """A 40-point scan (n_valid < 50: FLS_NOT_CONVERGED) in the middle of a group, and in another call an empty scan, which the host answers: the
    other jobs equal their fresh handles either way."""
    tiny = world.scans[1][:40].copy()
    scans = [world.scans[0], tiny, world.scans[2]]
    T0 = [np.eye(4)] * 3
    ref = world.fresh(tiny, np.eye(4))
    assert not ref[0] and ref[3] < 50 and ref[4] == 40
    m = world.owner()
    got = table(*m.MatchBatchSharedIvox(clusters_of(scans), T0, slots=3))
    assert m.batch_rc == _lib.FLS_OK and m.batch_status[1] == _lib.FLS_NOT_CONVERGED
    assert m.batch_status[0] == _lib.FLS_OK and m.batch_status[2] == _lib.FLS_OK
    assert_equal_fresh(world, got, scans, T0)
    assert ivox_stats(m)[2:] == [3, 0, 1]

    empty = world.scans[1][:0].copy()
    scans = [world.scans[0], empty, world.scans[2]]
    ref = world.fresh(empty, np.eye(4))
    assert not ref[0] and ref[2] == 1 and ref[3] == 0 and ref[4] == 0
    got = table(*m.MatchBatchSharedIvox(clusters_of(scans), T0, slots=3))
    assert m.batch_rc == _lib.FLS_OK and m.batch_status == [_lib.FLS_OK, _lib.FLS_NOT_CONVERGED, _lib.FLS_OK]
    assert_equal_fresh(world, got, scans, T0)
    assert ivox_stats(m)[2:] == [5, 1, 2]  # the empty job ran outside the shared launches
    m.close()


@pytest.mark.parametrize("n_jobs,slots", [(1, 8), (2, 16)])
def test_one_job_and_more_slots_than_jobs(world, n_jobs, slots):
    scans, T0 = world.scans[:n_jobs], [np.eye(4)] * n_jobs
    m = world.owner()
    got = table(*m.MatchBatchSharedIvox(clusters_of(scans), T0, slots=slots))
    assert_equal_fresh(world, got, scans, T0)
    assert ivox_stats(m)[2:] == [n_jobs, 0, 1]
    m.close()


def test_three_calls_on_one_handle_and_the_owner_state(world):
    """The ticket words return to zero and no neighbour list carries over: three calls give one table, with a Match of the owner between the second and
    the third; the owner's own sequence of Matches is what an owner that never ran a batch computes.  (Localization-mode owners: their Match leaves the
    map as it is, so the third table is that of the same map.)"""
    scans, T0 = world.scans[:3], [np.eye(4)] * 3
    cl = clusters_of(world.scans)

    def owner_match(h, k):
        T = np.eye(4)
        ok = h.Match(cl[k], T, update_map=True)
        return ok, T.tobytes(), h.stats.iterations, h.stats.n_valid

    m, plain = world.owner(is_localization_mode=True), world.owner(is_localization_mode=True)
    first = table(*m.MatchBatchSharedIvox(clusters_of(scans), T0, slots=2))
    second = table(*m.MatchBatchSharedIvox(clusters_of(scans), T0, slots=2))
    between = owner_match(m, 3)
    third = table(*m.MatchBatchSharedIvox(clusters_of(scans), T0, slots=2))
    after = owner_match(m, 4)
    assert_equal_fresh(world, first, scans, T0)
    assert first == second == third
    assert between == owner_match(plain, 3) and after == owner_match(plain, 4)
    assert ivox_stats(m)[2:] == [9, 0, 6]
    m.close()
    plain.close()


def test_calls_around_a_map_update_of_the_owner(world):
    """Mapping mode: the owner's Match(update_map=True) changes the map between two calls.  The call before it equals the fresh handles, the call after
    it equals MatchBatch(lanes=1) of an owner with the same history that never ran a shared batch, and both owners' Matches agree."""
    scans, T0 = world.scans[:3], [np.eye(4)] * 3
    cl = clusters_of(world.scans)

    def owner_match(h, k):
        T = np.eye(4)
        ok = h.Match(cl[k], T, update_map=True)
        return ok, T.tobytes(), h.stats.iterations, h.stats.n_valid, h.map_size(0)

    m, plain = world.owner(), world.owner()
    before = table(*m.MatchBatchSharedIvox(clusters_of(scans), T0, slots=3))
    assert_equal_fresh(world, before, scans, T0)
    assert owner_match(m, 3) == owner_match(plain, 3)
    after = table(*m.MatchBatchSharedIvox(clusters_of(scans), T0, slots=3))
    assert after == table(*plain.MatchBatch(clusters_of(scans), T0, lanes=1))
    assert owner_match(m, 4) == owner_match(plain, 4)
    m.close()
    plain.close()


WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["FLS_ROOT"])
import numpy as np
from funny_lidar_slam_amd import registration as reg, synth
cfg0 = synth.make_config(1, job=0, scale=0.05)
scans = [cfg0["scan"]] + [synth.make_config(1, job=j, scale=0.05, with_map=False)["scan"] for j in range(1, 5)]
def owner():
    m = reg.make_matcher("PointToPlane_IVOX", reg.YAML_NCLT_IVOX)
    m.AddCloudToLocalMap([cfg0["map"]])
    return m
fresh = []
for s in scans:
    f = owner()
    T = np.eye(4)
    ok = f.Match(reg.PointcloudCluster(planar_cloud_=s), T, update_map=False)
    fresh.append([bool(ok), T.tobytes().hex(), int(f.stats.iterations), int(f.stats.n_valid)])
    f.close()
m = owner()
oks, Ts, st = m.MatchBatchSharedIvox([reg.PointcloudCluster(planar_cloud_=s) for s in scans], [np.eye(4)] * 5, slots=3)
got = [[bool(oks[j]), np.ascontiguousarray(Ts[j]).tobytes().hex(), int(st[j].iterations), int(st[j].n_valid)] for j in range(5)]
print("RESULT " + json.dumps({"fresh": fresh, "got": got, "over_budget": int(m.map_size(132)), "stats": [m.BatchIvoxStat(k) for k in range(5)]}))
m.close()
'''


def test_hash_table_image(built):
    """The DENSE = false kernels: a process whose brick budget is 1 MB builds the per-voxel hash-table image (the budget is read once per process), and
    the call of the first test equals the fresh handles of that same process."""
    assert _lib.device_count() >= 1
    env = dict(os.environ, FLS_ROOT=ROOT, FLS_IVOX_BRICK_BUDGET_MB="1")
    r = subprocess.run([sys.executable, "-c", WORKER], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    assert out["over_budget"] == 1
    assert out["got"] == out["fresh"]
    assert out["stats"][2:] == [5, 0, 2] and 0 < out["stats"][0] == out["stats"][1]


def test_other_kinds_run_as_the_fused_batch(built):
    cfg0 = synth.make_config(0, job=0)
    scans = [cfg0["scan"], synth.make_config(0, job=1, with_map=False)["scan"]]
    clusters = [reg.PointcloudCluster(ordered_cloud_=s) for s in scans]
    m = reg.make_matcher("IcpOptimized", reg.YAML_NCLT_ICP, is_localization_mode=True)
    m.AddCloudToLocalMap([cfg0["map"]])
    fused = table(*m.MatchBatchFused(clusters, [np.eye(4)] * 2, slots=2))
    shared = table(*m.MatchBatchSharedIvox(clusters, [np.eye(4)] * 2, slots=2))
    assert shared == fused
    assert ivox_stats(m) == [0] * 5
    assert m.BatchStat(1) == 4 and m.BatchStat(3) == 2  # both calls took the fused form
    m.close()
