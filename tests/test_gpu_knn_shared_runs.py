"""The shared-run path of the iVox kNN kernel (csrc/kernels_ivox_coop.hpp: run detection per wave, the wave-uniform gate, the staging of a run's
19 voxels in LDS and the scan from there) against the CPU oracle on small hand-built maps, built like tests/test_gpu_knn_bookkeeping.py.

Every case runs PointToPlane_IVOX with max_iterations 1, 2 and 3 on the same inputs as the oracle, with the brick image and with the hash-table
fall-back (FLS_IVOX_DENSE=0, which never shares), with the product kernel and with its counting variant: counts, valid flags and neighbour ids
through tests/util.assert_same_registration with NO tie budget, the three traffic counters exactly, and the number of waves that took the shared
path equal to what tools/knn_run_stats.predict_waves says from the oracle's per-iteration poses.  The scans are ORDERED (a wave is 16 consecutive
queries), so that waves share; the gate's limits come from fls_debug_ivox_knn_limits, not from a copy."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg
from tests import util
from tests import test_gpu_knn_bookkeeping as bk

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import knn_run_stats as krs  # noqa: E402

MODE = bk.MODE
ITERS = bk.ITERS
RES = 0.5
DENS = 18.0  # map points per m^2: the 3 x 3 in-plane voxels of a query's 19 hold about 40


@functools.lru_cache(maxsize=None)
def _limits():
    r, c = C.c_int(0), C.c_int(0)
    assert _lib.lib().fls_debug_ivox_knn_limits(C.byref(r), C.byref(c)) == _lib.FLS_OK
    assert 1 <= r.value <= 16 and c.value >= 64
    return r.value, c.value


@functools.lru_cache(maxsize=None)
def _base_map():
    """bk._scene: floor z = 0 over [-4, 4]^2, walls x = 4 and y = -4 (0.3 .. 3 m high), 5 mm of noise along the normal"""
    return bk._scene(np.random.default_rng(31), lambda u, v: DENS, DENS)


# voxel keys on the three planes: the floor's voxels are (kx, ky, 0), the walls' (8, ky, kz) and (kx, -8, kz) with kz >= 1
def floor(kx, ky):
    return (kx, ky, 0)


def wall_x(ky, kz):
    return (8, ky, kz)


def wall_y(kx, kz):
    return (kx, -8, kz)


def _pts(rng, key, n, inner=0.14):
    """n world points in voxel `key`, within `inner` of its centre on every axis (the scan sees them from T_GT and the Match starts at the identity:
    they move by less than 0.1 m between the iterations and stay in the voxel); on a plane of the scene where the voxel holds one"""
    c = np.asarray(key, np.float64) * RES
    p = c + rng.uniform(-inner, inner, (n, 3))
    if key[2] == 0:
        p[:, 2] = rng.normal(0.0, 0.005, n)
    elif key[0] == 8:
        p[:, 0] = 4.0 + rng.normal(0.0, 0.005, n)
    elif key[1] == -8:
        p[:, 1] = -4.0 + rng.normal(0.0, 0.005, n)
    return p


def _wave(rng, runs):
    """16 queries: runs = [(key, length), ...] in order"""
    assert sum(n for _, n in runs) == 16
    return np.vstack([_pts(rng, k, n) for k, n in runs])


def _patches(rng, per_voxel):
    """well-posed backbone whose waves share: `per_voxel` queries in each of 8 floor, 6 + 6 wall voxels"""
    keys = [floor(-6, -5), floor(-3, 5), floor(2, -6), floor(5, 3), floor(-5, 1), floor(1, 1), floor(6, -3), floor(-2, -3),
            wall_x(-6, 2), wall_x(-2, 4), wall_x(3, 1), wall_x(6, 3), wall_x(0, 5), wall_x(-4, 1),
            wall_y(-6, 3), wall_y(-1, 1), wall_y(2, 4), wall_y(5, 2), wall_y(-3, 5), wall_y(6, 1)]
    return np.vstack([_pts(rng, k, per_voxel) for k in keys])


def _lines(rng):
    """backbone waves that do NOT share: 16 queries in 16 different voxels along the floor (x and y direction) and up the walls' length"""
    out = [np.vstack([_pts(rng, floor(kx, 4), 1) for kx in range(-7, 8)] + [_pts(rng, floor(-7, 5), 1)]),
           np.vstack([_pts(rng, floor(-4, ky), 1) for ky in range(-7, 8)] + [_pts(rng, floor(-3, 7), 1)]),
           np.vstack([_pts(rng, wall_x(ky, 2), 1) for ky in range(-7, 8)] + [_pts(rng, wall_x(-7, 3), 1)]),
           np.vstack([_pts(rng, wall_y(kx, 3), 1) for kx in range(-7, 8)] + [_pts(rng, wall_y(-7, 4), 1)])]
    return np.vstack(out)


def _case_one_voxel():
    """48 consecutive queries inside one floor voxel (about 40 candidates), then 16 per voxel on all three planes: one run in every wave"""
    rng = np.random.default_rng(41)
    s = np.vstack([_pts(rng, floor(2, 2), 48), _patches(rng, 16)])
    return dict(map=_base_map().astype(np.float32), scans=[bk._to_scan(s)])


def _case_runs_1_to_6():
    """Lines of queries crossing voxel faces: waves with exactly 1 .. R_MAX + 2 runs on every plane, run boundaries between lanes 15 | 16, 31 | 32 and
    47 | 48 (queries 3 | 4, 7 | 8, 11 | 12: the row boundaries of the lane shifts), runs of one query, a run that returns to an earlier key"""
    rng = np.random.default_rng(42)
    r_max = _limits()[0]
    f = lambda j: floor(-6 + j, -2)  # noqa: E731
    wx = lambda j: wall_x(-5 + j, 3)  # noqa: E731
    wy = lambda j: wall_y(-4 + j, 2)  # noqa: E731
    waves = []
    for vox in (f, wx, wy):
        for nr in range(1, r_max + 3):  # nr runs as even as they go
            cut = [16 // nr + (1 if j < 16 % nr else 0) for j in range(nr)]
            waves.append(_wave(rng, [(vox(j), c) for j, c in enumerate(cut)]))
        waves.append(_wave(rng, [(vox(0), 4), (vox(1), 12)]))
        waves.append(_wave(rng, [(vox(2), 8), (vox(3), 8)]))
        waves.append(_wave(rng, [(vox(4), 12), (vox(5), 4)]))
        waves.append(_wave(rng, [(vox(1), 4), (vox(2), 4), (vox(3), 8)]))
        waves.append(_wave(rng, [(vox(0), 1), (vox(1), 14), (vox(2), 1)]))
        waves.append(_wave(rng, [(vox(3), 7), (vox(4), 2), (vox(3), 7)]))
        waves.append(_wave(rng, [(vox(j), 4) for j in range(4)]))
    return dict(map=_base_map().astype(np.float32), scans=[bk._to_scan(np.vstack(waves))])


# islands in the air over the floor (z = 2 m, nothing of the scene within two voxels): exact neighbourhood totals
def _island(rng, key, n_centre, n_faces):
    """n_centre map points in voxel `key` and n_faces dealt over its six face neighbours"""
    k = np.asarray(key)
    out = [np.asarray(key, np.float64) * RES + rng.uniform(-0.2, 0.2, (n_centre, 3))]
    for j in range(n_faces):
        d = np.zeros(3, np.int64)
        d[j % 3] = 1 if (j // 3) % 2 == 0 else -1
        out.append((k + d) * RES + rng.uniform(-0.2, 0.2, (1, 3)))
    return np.vstack(out)


def _case_cap_edge():
    """one-run waves whose 19 voxels hold CAP - 1, CAP and CAP + 1 points, and one whose single voxel holds more than CAP"""
    rng = np.random.default_rng(43)
    cap = _limits()[1]
    isl = [((-4, -4, 4), cap - 1 - 60, 60), ((4, -4, 4), cap - 60, 60), ((-4, 4, 4), cap + 1 - 60, 60), ((4, 4, 4), cap + 40, 0)]
    m = np.vstack([_base_map()] + [_island(rng, k, a, b) for k, a, b in isl])
    s = np.vstack([_pts(rng, k, 16) for k, _, _ in isl] + [_patches(rng, 8), _lines(rng)])
    return dict(map=m.astype(np.float32), scans=[bk._to_scan(s)], islands=[(k, a + b) for k, a, b in isl])


def _case_aba():
    """first Match: keys A B A B ... in every wave (16 runs: nothing shares); second Match on the same handle: 8 x A then 8 x B (two runs), A B A (three
    runs, the third returns to the first key) and the A B A B waves again"""
    rng = np.random.default_rng(44)
    pairs = [(floor(-5, -5), floor(-4, -5)), (floor(3, 2), floor(3, 3)), (floor(-1, 0), floor(0, 0)), (wall_x(-3, 2), wall_x(-3, 3)), (wall_x(4, 4), wall_x(5, 4)),
             (wall_y(-5, 2), wall_y(-4, 2)), (wall_y(3, 3), wall_y(3, 4))]
    abab = np.vstack([_wave(rng, [((a, b)[j & 1], 1) for j in range(16)]) for a, b in pairs])
    halves = np.vstack([_wave(rng, [(a, 8), (b, 8)]) for a, b in pairs] + [_wave(rng, [(a, 5), (b, 6), (a, 5)]) for a, b in pairs])
    return dict(map=_base_map().astype(np.float32), scans=[bk._to_scan(abab), bk._to_scan(np.vstack([halves, abab]))])


def _case_mixed_validity():
    """Inside waves that share: a query beyond the key range, queries in a missing brick, islands with 1 - 4 candidates, queries without a candidate in
    an existing brick; then a second Match on the same handle with every third point of the first waves and the upper half of every later wave moved
    200 m away (into missing bricks: their previous lists must survive, Q15 -- in waves that do not share and in waves that do)."""
    rng = np.random.default_rng(45)
    isl_keys = [(-5, 3, 4), (-1, 3, 4), (3, 3, 4), (-3, -2, 4)]
    isl = [np.asarray(k, np.float64) * RES + rng.uniform(-0.12, 0.12, (j + 1, 3)) for j, k in enumerate(isl_keys)]
    m = np.vstack([_base_map()] + isl)
    a, b = floor(1, -5), wall_x(2, 3)
    beyond = np.array([[6.0e5, 1.0, 2.0]])  # |key| = 1.2e6 > 2^20 - 2
    far = np.array([1.0, 1.0, 9.0]) + rng.uniform(-0.1, 0.1, (8, 3))  # one voxel of a brick the image does not hold (9 m over the floor)
    none = _pts(rng, (2, 2, 2), 6)  # 1 m over the floor: the brick exists, none of the 19 voxels holds a point
    waves = [np.vstack([_pts(rng, a, 8), beyond, _pts(rng, a, 7)]),
             np.vstack([_pts(rng, b, 8), far]),
             np.vstack([_pts(rng, a, 5), none, _pts(rng, b, 5)]),
             np.vstack([_pts(rng, b, 9), beyond, far[:6]])]
    waves += [_pts(rng, k, 16, inner=0.18) for k in isl_keys]
    s1 = bk._to_scan(np.vstack(waves + [_patches(rng, 8), _lines(rng)]))
    s2 = s1.copy()
    s2[:128:3, 1] += np.float32(200.0)
    for w in range(8, len(s2) // 16):
        s2[16 * w + 8:16 * w + 16, 1] += np.float32(200.0)
    return dict(map=m.astype(np.float32), scans=[s1, s2])


def _case_brick_faces():
    """runs in voxels on brick faces, edges and corners (the bricks of 8 voxels meet at keys -8, 0 and 8; the floor is the z-face of its bricks, the
    wall x = 4 the x-face of the next brick) at negative and positive coordinates: their neighbours are halo cells"""
    rng = np.random.default_rng(46)
    waves = [_wave(rng, [(floor(-1, -1), 5), (floor(0, -1), 5), (floor(0, 0), 6)]),
             _wave(rng, [(floor(-1, 0), 8), (floor(-1, -1), 8)]),
             _wave(rng, [(floor(7, 3), 6), (floor(7, 7), 10)]),
             _wave(rng, [(floor(-8, -8), 4), (floor(-8, -7), 4), (floor(-7, -8), 8)]),
             _wave(rng, [(floor(-8, 0), 16)]),
             _wave(rng, [(floor(0, 7), 3), (floor(-1, 7), 13)]),
             _wave(rng, [(wall_x(-1, 1), 8), (wall_x(0, 1), 8)]),
             _wave(rng, [(wall_x(7, 5), 4), (wall_x(-8, 5), 4), (wall_x(0, 5), 8)]),
             _wave(rng, [(wall_y(-1, 1), 6), (wall_y(0, 1), 5), (wall_y(0, 2), 5)]),
             _wave(rng, [(wall_y(7, 4), 16)]),
             _wave(rng, [(wall_y(-8, 1), 8), (wall_x(-8, 1), 8)]),
             _wave(rng, [(floor(-1, -1), 4), (floor(0, -1), 4), (floor(0, 0), 4), (floor(-1, 0), 4)]),
             _wave(rng, [((floor(0, 0), floor(-1, 0), floor(-1, -1), floor(0, -1))[j & 3], 1) for j in range(16)])]
    return dict(map=_base_map().astype(np.float32), scans=[bk._to_scan(np.vstack(waves + [_lines(rng)]))])


def _case_ragged_n():
    """ordered scans of 1, 15, 17, 63, 65 and 129 points on one handle (the lanes past the end form a run of their own): the first n points of
    a scan whose waves alternate between one that shares (two voxels) and one that does not (16 voxels)"""
    rng = np.random.default_rng(47)
    share, lines = _patches(rng, 8), _lines(rng)
    lines = np.vstack([lines, lines[::-1] + rng.uniform(-0.01, 0.01, lines.shape) * [1, 1, 0]])
    src = np.vstack([np.vstack([share[16 * w:16 * w + 16], lines[16 * w:16 * w + 16]]) for w in range(5)])
    s = bk._to_scan(src)
    return dict(map=_base_map().astype(np.float32), scans=[np.ascontiguousarray(s[:n]) for n in (1, 15, 17, 63, 65, 129)])


CASES = {
    "one_voxel": _case_one_voxel,
    "runs_1_to_6": _case_runs_1_to_6,
    "cap_edge": _case_cap_edge,
    "aba": _case_aba,
    "mixed_validity": _case_mixed_validity,
    "brick_faces": _case_brick_faces,
    "ragged_n": _case_ragged_n,
}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def _vmap(name):
    return krs.VoxelMap(_inputs(name)["map"])


@functools.lru_cache(maxsize=None)
def _reference(name, iters):
    """the oracle's Matches of a case (computed once, shared by every run; never modified)"""
    inp = _inputs(name)
    o = util.oracle_for(MODE, bk._yaml(iters))
    o.AddCloudToLocalMap(inp["map"])
    out = []
    for scan in inp["scans"]:
        ok, T = o.Match(scan, np.eye(4), update_map=False)
        out.append(bk._Snap(o, ok, T))
    o.close()
    return out


@functools.lru_cache(maxsize=None)
def _predicted(name, iters):
    """per Match: a list over the oracle's iterations of (shared bool per wave, the wave table).  The iteration log holds the pose AFTER each
    iteration: the search of iteration i runs at the initial pose (the identity here) for i = 0 and at row i - 1 of the log after that."""
    r_max, cap = _limits()
    out = []
    for scan, snap in zip(_inputs(name)["scans"], _reference(name, iters)):
        per_it = []
        for T in [np.eye(4)] + list(snap._log[0][:-1]):
            w = krs.wave_table(scan, T, _vmap(name))
            per_it.append(((w["runs"] <= r_max) & (w["entries"] <= cap), w))
            assert np.array_equal(per_it[-1][0], krs.predict_waves(scan, T, _vmap(name), r_max, cap))
        out.append(per_it)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_have_no_distance_tie_and_stand_on_both_sides_of_the_gate(built, name):
    """no GPU needed: the oracle marks no row of any case as decided by an exact distance tie; the predictor's candidate, hit-voxel and probe sums over
    the oracle's per-iteration poses are the oracle's own traffic counters (so its model of map and keys is the oracle's); and the predictor puts at
    least two waves on each side of the gate in every case -- except one_voxel (every wave shares, one run each) and aba's first Match (none does)"""
    r_max, cap = _limits()
    inp = _inputs(name)
    for iters in ITERS:
        shared = unshared = 0
        for k, (snap, per_it) in enumerate(zip(_reference(name, iters), _predicted(name, iters))):
            assert snap.tie_queries == 0, (name, iters, k, snap.tie_queries)
            assert snap._tie is None or not snap._tie.any(), (name, iters, k, int(snap._tie.sum()))
            n = inp["scans"][k].shape[0]
            assert snap.stats.n_source == n and len(per_it) == snap.stats.iterations >= 1
            assert snap.traffic == (19 * n * len(per_it), sum(int(w["hits"].sum()) for _, w in per_it), sum(int(w["cand"].sum()) for _, w in per_it)), (name, iters, k)
            for sh, w in per_it:
                assert len(sh) == (n + 15) // 16
                if name == "one_voxel":
                    assert sh.all() and (w["runs"] == 1).all() and 25 <= w["cand"][:48].min() and w["cand"][:48].max() <= 60, (w["runs"], w["cand"][:48])
                if name == "aba" and k == 0:
                    assert not sh.any() and (w["runs"] == 16).all()
                if name == "aba" and k == 1:
                    assert (w["runs"][:7] == 2).all() and (w["runs"][7:14] == 3).all() and sh[:14].all() and not sh[14:].any()
                if name == "runs_1_to_6":
                    assert set(w["runs"]) == set(range(1, r_max + 3)) and np.array_equal(sh, w["runs"] <= r_max)
                if name == "cap_edge":
                    assert list(w["entries"][:4]) == [cap - 1, cap, cap + 1, cap + 40] and (w["runs"][:4] == 1).all() and list(sh[:4]) == [True, True, False, False]
                if name == "brick_faces":
                    assert sh[:11].all() and sh[11] == (r_max >= 4) and not sh[12:].any()
                if name != "aba" or k == 1:
                    shared += int(sh.sum()); unshared += int((~sh).sum())
        if name == "one_voxel":
            assert unshared == 0 and shared >= 11
        else:
            assert shared >= 2 and unshared >= 2, (name, iters, shared, unshared)
    cnt = _reference(name, 3)[0].correspondences(0)[1]
    if name == "mixed_validity":
        assert set(np.unique(cnt)) >= {0, 1, 2, 3, 4, 5}
        sh0 = _predicted(name, 3)[0][0][0]
        assert sh0[:8].all()  # the waves with the query beyond the range, the missing brick, the empty neighbourhood and the islands all share
        cnt2 = _reference(name, 3)[1].correspondences(0)[1]
        moved = np.zeros(len(cnt2), bool); moved[:128:3] = True
        for w in range(8, len(cnt2) // 16):
            moved[16 * w + 8:16 * w + 16] = True
        assert np.array_equal(cnt2[moved], cnt[moved]) and cnt[moved].max() == 5  # Q15: the lists of the first Match survive
        sh1 = _predicted(name, 3)[1][0][0]
        assert sh1[8:].any() and not sh1[:8].all()


@pytest.fixture(scope="module")
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"


@pytest.mark.gpu
@pytest.mark.parametrize("dense", [True, False], ids=["bricks", "hash"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_shared_runs_equal_the_oracle(_need_gpu, monkeypatch, name, dense):
    """lists, flags, counts and poses of every Match equal the oracle's without a tie budget; the counting run's three traffic counters are the oracle's
    and its shared-wave count is the predictor's, per Match (0 with the hash-table image)"""
    if not dense:
        monkeypatch.setenv("FLS_IVOX_DENSE", "0")
    inp = _inputs(name)
    for iters in ITERS:
        ref, pred = _reference(name, iters), _predicted(name, iters)
        for counting in (False, True):  # the product kernel, then its counting variant
            m = reg.make_matcher(MODE, bk._yaml(iters))
            try:
                m.AddCloudToLocalMap([inp["map"]])
                m.set_profiling(False, counters=counting)
                for k, scan in enumerate(inp["scans"]):
                    T = np.eye(4)
                    ok = m.Match(reg.PointcloudCluster(planar_cloud_=scan), T, update_map=False)
                    util.assert_same_registration(m, ref[k], ok, T, ref[k].ok, ref[k].T, sets_only_tail=True, max_tie_rows=0)
                    if counting:
                        assert m.traffic_counters() == ref[k].traffic, (name, iters, k, m.traffic_counters(), ref[k].traffic)
                        want = sum(int(sh.sum()) for sh, _ in pred[k]) if dense else 0
                        print(name, "iters", iters, "match", k, "shared waves", m.knn_shared_waves(), "predicted", want, "of", sum(len(sh) for sh, _ in pred[k]))
                        assert m.knn_shared_waves() == want, (name, iters, k, m.knn_shared_waves(), want)
                    else:
                        assert m.knn_shared_waves() == 0  # (no counting run on this handle yet)
            finally:
                m.close()


@pytest.mark.gpu
def test_jobs_kernel_on_ordered_scans(_need_gpu):
    """ivox_knn_jobs_kernel runs the same body: a group of three jobs with ordered scans (their waves share, by the predictor) in shared launches
    equals three fresh handles' Matches, which the test above holds against the oracle"""
    r_max, cap = _limits()
    names = ("one_voxel", "runs_1_to_6", "brick_faces")
    scans = [_inputs(n)["scans"][0] for n in names]
    amap = _inputs(names[0])["map"]
    assert all(np.array_equal(_inputs(n)["map"], amap) for n in names)
    for s in scans:
        assert krs.predict_waves(s, np.eye(4), _vmap(names[0]), r_max, cap).sum() >= 8
    y = bk._yaml(3)
    fresh = []
    for s in scans:
        f = reg.make_matcher(MODE, y)
        f.AddCloudToLocalMap([amap])
        T = np.eye(4)
        ok = f.Match(reg.PointcloudCluster(planar_cloud_=s), T, update_map=False)
        fresh.append((bool(ok), T.tobytes(), f.stats.iterations, f.stats.n_valid))
        f.close()
    m = reg.make_matcher(MODE, y)
    try:
        m.AddCloudToLocalMap([amap])
        oks, Ts, stats = m.MatchBatchSharedIvox([reg.PointcloudCluster(planar_cloud_=s) for s in scans], [np.eye(4)] * 3, slots=3)
        assert m.batch_rc >= 0 and all(s >= 0 for s in m.batch_status)
        got = [(bool(oks[j]), np.ascontiguousarray(Ts[j]).tobytes(), stats[j].iterations, stats[j].n_valid) for j in range(3)]
        assert got == fresh
        assert m.BatchIvoxStat(2) == 3 and m.BatchIvoxStat(3) == 0  # all three ran in shared launches
    finally:
        m.close()
