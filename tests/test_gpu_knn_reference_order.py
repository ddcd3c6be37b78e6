"""The reference neighbour order of the iVox kind (include/fls_knn_order.h, csrc/kernels_ivox_knn_reforder.hpp) on a GPU against the CPU oracle with its
tie switch OFF: the oracle then leaves candidates at equal distance, and slots 1..4 of every list, to libstdc++'s std::nth_element exactly as the
reference does, and a reference-order handle has to return the same lists element for element.

Constructed inputs state what they construct as an assertion on the oracle (every query meets a tie; the tails are not ascending).  The default order is
what tests/util.py's tie budget and gpu_scenarios.TIE_SCENARIOS describe; nothing here changes it (test_switching compares against it bit for bit)."""
import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg, synth
from oracle import oracle as O
from tests import gpu_scenarios, util

pytestmark = pytest.mark.gpu

NEARBY18 = np.array([(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (1, 1, 0), (-1, 1, 0), (1, -1, 0), (-1, -1, 0),
                     (1, 0, 1), (-1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 1), (0, -1, 1), (0, 1, -1), (0, -1, -1)])


def lattice_room(s: float) -> np.ndarray:
    """three orthogonal planar lattices, floor z = 0 and walls x = -4, y = -4, coordinates s / 2 + s i over +-4 m"""
    c = (s / 2 + s * np.arange(-int(round(4 / s)), int(round(4 / s)))).astype(np.float32)
    u, v = [a.reshape(-1) for a in np.meshgrid(c, c, indexing="ij")]
    z, w = np.zeros_like(u), np.full_like(u, -4.0)
    return np.concatenate([np.stack([u, v, z], 1), np.stack([w, u, v], 1), np.stack([u, w, v], 1)]).astype(np.float32)


def centre_queries() -> np.ndarray:
    """363 queries at voxel centres (0.5 m voxels) on the three planes"""
    c = (0.5 * np.arange(-5, 6)).astype(np.float32)
    u, v = [a.reshape(-1) for a in np.meshgrid(c, c, indexing="ij")]
    z, w = np.zeros_like(u), np.full_like(u, -4.0)
    return np.concatenate([np.stack([u, v, z], 1), np.stack([w, u, v], 1), np.stack([u, w, v], 1)]).astype(np.float32)


def random_room(seed: int = 5):
    """44,000 map points on a floor and two walls with 5 mm noise, 1,700 queries on the same surfaces (1,700 is no multiple of 64)"""
    rng = np.random.default_rng(seed)

    def surfaces(n, lo, hi):
        k = rng.integers(0, 3, n)
        a, b = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
        h = rng.uniform(0.0, hi - lo, n) * 0.5  # walls: half as high as the floor is wide
        noise = rng.normal(0.0, 0.005, n)
        p = np.where((k == 0)[:, None], np.stack([a, b, noise], 1), np.where((k == 1)[:, None], np.stack([-6.0 + noise, a, h], 1), np.stack([a, -6.0 + noise, h], 1)))
        return p.astype(np.float32)
    return surfaces(44000, -6.0, 6.0), surfaces(1700, -4.5, 4.5)


def ivox_pair(y, order="reference", loc=True):
    m = reg.make_matcher("PointToPlane_IVOX", y, is_localization_mode=loc)
    m.SetKnnOrder(order)
    assert m.KnnOrder() == order
    return m, util.oracle_for("PointToPlane_IVOX", y, loc)


def small_pose(dx=0.03, dy=-0.02, dz=0.01, yaw=0.004):
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = [dx, dy, dz]
    return T


@pytest.fixture(scope="module")
def room():
    return random_room()


def run_lattice(s, extra=None):
    """one iteration from the identity on the lattice room (+ extra map points behind it); returns (m, o, ok, T, ok_ref, T_ref): close both"""
    y = dict(reg.YAML_NCLT_IVOX, optimization_iter_num=1)
    m, o = ivox_pair(y)
    cloud = lattice_room(s) if extra is None else np.concatenate([lattice_room(s), extra]).astype(np.float32)
    q = centre_queries()
    m.AddCloudToLocalMap([cloud]); o.AddCloudToLocalMap(cloud)
    T = np.eye(4)
    ok = m.Match(reg.PointcloudCluster(planar_cloud_=q), T, update_map=False)
    ok_ref, T_ref = o.Match(q, np.eye(4), update_map=False)
    return m, o, ok, T, ok_ref, T_ref, cloud, q


def assert_lattice_equal(s):
    O.set_tie_break_by_id(False)
    m, o, ok, T, ok_ref, T_ref, cloud, q = run_lattice(s)
    try:
        assert cloud.shape[0] == (3072 if s == 0.25 else 12288) and q.shape[0] == 363
        assert int(o.counters().tie_queries) == 363  # the input condition: every query's list is decided by an exact distance tie
        ids, cnt, valid = m.correspondences()
        ids_r, cnt_r, valid_r = o.correspondences()
        print("lattice", s, "rows equal", int((ids == ids_r).all(1).sum()), "of", ids.shape[0], "n_valid", m.stats.n_valid, o.stats.n_valid,
              "sum_res", m.stats.sum_res, o.stats.sum_res, "slot 177/178", m.map_size(177), m.map_size(178))
        assert np.array_equal(ids, ids_r), np.flatnonzero((ids != ids_r).any(1))[:8]  # all five slots, element for element
        assert np.array_equal(cnt, cnt_r) and np.array_equal(valid, valid_r)
        assert ok == ok_ref and m.stats.n_valid == o.stats.n_valid and m.stats.iterations == o.stats.iterations == 1
        (_, nvg, srg), (_, nvo, sro) = m.iteration_log(), o.iteration_log()
        assert np.array_equal(nvg, nvo) and abs(srg[0] - sro[0]) <= 1e-9 * max(1.0, abs(sro[0])), (srg, sro)
        assert m.map_size(177) >= 1 and m.map_size(178) == 0
    finally:
        m.close(); o.close()


@pytest.mark.parametrize("s", [0.25, 0.125])
def test_lattice_ties_equal_the_reference_order(s, built):
    """1. every one of the 363 queries sits at equal distance from several lattice points; at s = 0.125 a voxel holds 16 points, so the per-voxel
    truncation (nth_element on a sub-range) runs as well."""
    assert _lib.device_count() >= 1
    assert_lattice_equal(s)


def test_lattice_ties_on_the_hash_table_image(built, monkeypatch):
    """5. the same through the hash-table look-up (FLS_IVOX_DENSE=0)"""
    assert _lib.device_count() >= 1
    monkeypatch.setenv("FLS_IVOX_DENSE", "0")
    assert_lattice_equal(0.25)


def test_order_without_ties(room, built):
    """2. no ties: slots 1..4 of a list are in introselect order in the reference, ascending in the default order"""
    assert _lib.device_count() >= 1
    O.set_tie_break_by_id(False)
    cloud, q = room
    y = dict(reg.YAML_NCLT_IVOX, optimization_iter_num=3, position_converge_thres=1e-9, rotation_converge_thres=1e-9)  # (all three iterations run)
    m, o = ivox_pair(y)
    try:
        m.AddCloudToLocalMap([cloud]); o.AddCloudToLocalMap(cloud)
        guess = small_pose()
        T = guess.copy()
        ok = m.Match(reg.PointcloudCluster(planar_cloud_=q), T, update_map=False)
        ok_ref, T_ref = o.Match(q, guess.copy(), update_map=False)
        ids_r, cnt_r, _ = o.correspondences()
        # the input condition, on the oracle's own lists: the tail is not ascending by distance in at least 100 rows
        To = o.iteration_log()[0]
        it = int(o.stats.iterations)
        Tq = To[it - 2] if it >= 2 else guess  # the pose the last iteration searched with
        qw = q.astype(np.float64) @ Tq[:3, :3].T + Tq[:3, 3]
        full = cnt_r == 5
        d = np.linalg.norm(cloud[np.where(ids_r >= 0, ids_r, 0)].astype(np.float64) - qw[:, None, :], axis=2)
        unsorted_rows = int((full & (np.diff(d[:, 1:], axis=1) < 0).any(1)).sum())
        print("rows whose tail is not ascending:", unsorted_rows, "of", q.shape[0], "iterations", it)
        assert unsorted_rows >= 100 and it == 3
        ids, _, _ = m.correspondences()
        assert np.array_equal(ids, ids_r), np.flatnonzero((ids != ids_r).any(1))[:8]
        util.assert_same_registration(m, o, ok, T, ok_ref, T_ref, sets_only_tail=False, max_tie_rows=0)
    finally:
        m.close(); o.close()


@pytest.mark.parametrize("name", gpu_scenarios.TIE_SCENARIOS)
def test_tie_scenarios_are_plain_equality(name, built, monkeypatch):
    """3. the two pinned scenarios with a distance tie, which the default order can only explain (test_gpu_fuzz_replay.py), are equal in this mode"""
    assert _lib.device_count() >= 1
    monkeypatch.setenv("FLS_IVOX_KNN_ORDER", "reference")
    hist = gpu_scenarios.run_scenario(name)  # (the oracle's tie switch off)
    assert len(hist) >= 2


@pytest.mark.parametrize("name", ["fuzz3", "fuzz7", "fuzz23", "lfuzz2", "lfuzz6", "deg_ivox_empty", "deg_ivox_tiny", "deg_ivox_far"])
def test_ordinary_scenarios_in_the_mode(name, built, monkeypatch):
    """4. mapping-mode replays with map updates between the frames and LRU capacities of 1,500, 6,000 and 300 voxels, localization runs, the
    degenerate inputs (the untouched-list quirk, the empty scan)"""
    assert _lib.device_count() >= 1
    sc = gpu_scenarios.refpin.make_scenario(name)
    assert sc["mode"] == "PointToPlane_IVOX"
    monkeypatch.setenv("FLS_IVOX_KNN_ORDER", "reference")
    hist = gpu_scenarios.run_scenario(name, sc)
    assert len(hist) == len(sc["frames"])


def snapshot(m):
    ids, cnt, valid = m.correspondences()
    Tl, nv, sr = m.iteration_log()
    return dict(ids=ids.copy(), cnt=cnt.copy(), valid=valid.copy(), Tl=np.array(Tl), nv=np.array(nv), sr=np.array(sr), it=int(m.stats.iterations),
                n_valid=int(m.stats.n_valid), sum_res=float(m.stats.sum_res))


def assert_bit_identical(a, b):
    assert a["it"] == b["it"] and a["n_valid"] == b["n_valid"] and a["sum_res"] == b["sum_res"]
    for k in ("ids", "cnt", "valid", "Tl", "nv", "sr"):
        assert np.array_equal(a[k], b[k]), k


def test_switching(room, built):
    """6. reference, Match, default, Match on one handle: the second Match is a fresh default handle's, bit for bit"""
    assert _lib.device_count() >= 1
    cloud, q = room
    y = dict(reg.YAML_NCLT_IVOX, optimization_iter_num=4)
    m = reg.make_matcher("PointToPlane_IVOX", y, is_localization_mode=True)
    f = reg.make_matcher("PointToPlane_IVOX", y, is_localization_mode=True)
    try:
        assert m.KnnOrder() == "default" and m.map_size(177) == 0
        m.AddCloudToLocalMap([cloud]); f.AddCloudToLocalMap([cloud])
        cl = reg.PointcloudCluster(planar_cloud_=q)
        m.SetKnnOrder("reference")
        T1 = small_pose()
        m.Match(cl, T1, update_map=False)
        launches = m.map_size(177)
        assert launches >= m.stats.iterations >= 1
        m.SetKnnOrder("default")
        assert m.KnnOrder() == "default"
        T2, Tf = small_pose(), small_pose()
        ok2 = m.Match(cl, T2, update_map=False)
        okf = f.Match(cl, Tf, update_map=False)
        assert ok2 == okf and np.array_equal(T2, Tf)
        assert_bit_identical(snapshot(m), snapshot(f))
        assert m.map_size(177) == launches and f.map_size(177) == 0
    finally:
        m.close(); f.close()


def test_batch(built):
    """7. MatchBatch on a reference-order handle: every row is a fresh reference-order handle's Match; MatchBatchSharedIvox answers the same"""
    assert _lib.device_count() >= 1
    cfgs = [synth.make_config(1, job=j, scale=0.02) for j in range(4)]
    y = reg.YAML_NCLT_IVOX
    m = reg.make_matcher("PointToPlane_IVOX", y, is_localization_mode=True)
    try:
        m.SetKnnOrder("reference")
        m.AddCloudToLocalMap([cfgs[0]["map"]])
        clusters = [reg.PointcloudCluster(planar_cloud_=c["scan"]) for c in cfgs]
        inits = [c["T_init"] for c in cfgs]
        ok_b, T_b, st_b = m.MatchBatch(clusters, inits, lanes=2)
        after_batch = m.map_size(177)
        assert after_batch >= sum(int(s.iterations) for s in st_b)  # the lanes ran in reference order
        ok_s, T_s, st_s = m.MatchBatchSharedIvox(clusters, inits, slots=4)
        assert m.BatchIvoxStat(0) == 0 and m.map_size(177) > after_batch  # no shared kNN launch: the jobs ran on the lanes again
        for j in range(4):
            f = reg.make_matcher("PointToPlane_IVOX", y, is_localization_mode=True)
            try:
                f.SetKnnOrder("reference")
                f.AddCloudToLocalMap([cfgs[0]["map"]])
                Tf = np.array(inits[j], dtype=np.float64).copy()
                okf = f.Match(clusters[j], Tf, update_map=False)
                for ok_x, T_x, st_x in ((ok_b, T_b, st_b), (ok_s, T_s, st_s)):
                    assert ok_x[j] == okf and np.array_equal(T_x[j], Tf), j
                    assert (st_x[j].iterations, st_x[j].n_valid, st_x[j].sum_res) == (f.stats.iterations, f.stats.n_valid, f.stats.sum_res), j
            finally:
                f.close()
    finally:
        m.close()


def test_the_w_limit(built):
    """8. a voxel of W - 90 + 1 points: the queries that probe it keep the default list and are counted, every other row is the reference's"""
    assert _lib.device_count() >= 1
    O.set_tie_break_by_id(False)
    w = _lib.knn_order_limit()
    rng = np.random.default_rng(11)
    big_key = np.array([2, 2, 0])  # the voxel around (1, 1, 0): four lattice points at s = 0.25
    n_extra = w - 90 + 1 - 4
    extra = (big_key * 0.5 + rng.uniform(-0.24, 0.24, (n_extra, 3)) * np.array([1.0, 1.0, 0.1])).astype(np.float32)
    m, o, ok, T, ok_ref, T_ref, cloud, q = run_lattice(0.25, extra)
    y = dict(reg.YAML_NCLT_IVOX, optimization_iter_num=1)
    d = reg.make_matcher("PointToPlane_IVOX", y, is_localization_mode=True)
    try:
        keys = np.round(cloud * np.float32(2.0)).astype(int)
        assert int((keys == big_key).all(1).sum()) == w - 90 + 1  # the input condition: that voxel holds one point more than a query can take
        qk = np.round(q * np.float32(2.0)).astype(int)
        probes = ((qk[:, None, :] + NEARBY18[None, :, :]) == big_key).all(2).any(1)
        assert 1 <= int(probes.sum()) < q.shape[0]
        assert m.map_size(178) == int(probes.sum()), (m.map_size(178), int(probes.sum()))
        d.AddCloudToLocalMap([cloud])
        Td = np.eye(4)
        d.Match(reg.PointcloudCluster(planar_cloud_=q), Td, update_map=False)
        ids, cnt, valid = m.correspondences()
        ids_d, cnt_d, _ = d.correspondences()
        ids_r, cnt_r, _ = o.correspondences()
        assert np.array_equal(cnt, cnt_r) and np.array_equal(cnt, cnt_d)
        assert np.array_equal(ids[probes], ids_d[probes])      # the default (d2, slot) list
        assert np.array_equal(ids[~probes], ids_r[~probes])    # the reference's order
    finally:
        m.close(); o.close(); d.close()


@pytest.mark.parametrize("mode,y,cid,scale", [("IcpOptimized", reg.YAML_NCLT_ICP, 0, 0.3), ("IncrementalNDT", reg.YAML_NCLT_NDT, 2, 0.03)])
def test_wrong_kind(mode, y, cid, scale, built):
    """9. the reference order exists for the iVox kind alone: FLS_ERR_STATE, and the handle goes on working"""
    assert _lib.device_count() >= 1
    m = reg.make_matcher(mode, y, is_localization_mode=(mode == "IcpOptimized"))
    try:
        with pytest.raises(_lib.FlsError) as e:
            m.SetKnnOrder("reference")
        assert e.value.status == _lib.FLS_ERR_STATE
        assert m.KnnOrder() == "default"
        m.SetKnnOrder("default")
        cfg = synth.make_config(cid, scale=scale)
        m.AddCloudToLocalMap([cfg["map"]])
        T = cfg["T_init"].copy()
        m.Match(reg.PointcloudCluster(ordered_cloud_=cfg["scan"]), T, update_map=False)
        assert m.stats.iterations >= 1 and np.all(np.isfinite(T))
    finally:
        m.close()
