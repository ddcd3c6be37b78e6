"""The iVox map built from a whole cloud on the device (IvoxMap::bulk_build, kernels_ivox_build.hpp): the first AddCloudToLocalMap of a
mapping handle and every reload of a localization handle.  Two handles per test: A created with FLS_IVOX_DEVICE_BUILD=0 (the sequential host
insert + full flatten, the path every handle took before), B with the default.  B must be indistinguishable from A -- exported maps byte for
byte (voxels in LRU order, points with ids, next_id, is_first), correspondences and iteration logs bit for bit where exact distance ties make
the slot order visible -- and equal to the CPU oracle where the existing parity tests compare against it."""
import functools

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg, synth
from tests import util

pytestmark = pytest.mark.gpu

MODE, Y = "PointToPlane_IVOX", reg.YAML_NCLT_IVOX


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"


def handles(monkeypatch, loc=False, y=Y):
    """(A, B): the switch is read when the handle is created"""
    monkeypatch.setenv("FLS_IVOX_DEVICE_BUILD", "0")
    a = reg.make_matcher(MODE, y, is_localization_mode=loc)
    monkeypatch.delenv("FLS_IVOX_DEVICE_BUILD")
    b = reg.make_matcher(MODE, y, is_localization_mode=loc)
    return a, b


def at_voxels(keys, jitter=0.0):
    return (0.5 * np.asarray(keys, np.float64) + jitter).astype(np.float32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def cfg20k():
    return synth.make_config(1, scale=0.02)  # a 20,000-point map of configs[1]'s density


@functools.lru_cache(maxsize=None)
def cloud300k():
    return synth.sample_map(synth.make_scene(), 300000, synth.rng_for(1, 0, 31), radius=60.0)


def hand_made():
    rng = np.random.default_rng(7)
    out = {"one point": np.array([[1.0, 2.0, 3.0]], np.float32)}
    for n in (1, 4, 5, 37):  # the cap_for steps
        out[f"{n} in one voxel"] = at_voxels([[3, -2, 1]] * n) + (0.001 * np.arange(n, dtype=np.float32))[:, None]
    edge = (7, 8, -1, 0)  # brick faces, edges and a corner
    b = at_voxels([(a, c, d) for a in edge for c in edge for d in edge] * 2)
    b[64:] += np.float32(0.01)
    out["brick boundaries"] = b[rng.permutation(len(b))]
    h = (0.25, -0.25, 0.75, -0.75)  # round half away from zero
    out["half-way coordinates"] = np.array([(a, c, d) for a in h for c in h for d in h], np.float32)
    A, B = (1, 1, 1), (20, 1, 1)  # LRU by last member
    out["ABAAB"] = at_voxels([A, B, A, A, B])
    # an extent of 2^20 voxels per axis: the sort key is wider than 32 bits (two stable rounds), bricks of negative and positive coordinates
    far = [(sx * 1000001, sy * 999983, sz * 1000003) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    f = at_voxels((far + [(0, 0, 0), (1, 0, 0)]) * 3)
    out["far corners"] = f[rng.permutation(len(f))]
    return out


def host_flattens(m):
    """full re-flattens of the image from the host mirror.  Slot 101 counts every full build of the image -- the existing replay tests pin it
    to 1 for "only the initial build" -- so a build on the device counts there too; slot 140 says how many of them the device did."""
    return m.map_size(101) - m.map_size(140)


def same_export(a, b):
    ea, eb = a.ExportMap(), b.ExportMap()
    return ea.shape == eb.shape and np.array_equal(ea, eb)


def test_counters(monkeypatch):
    a, b = handles(monkeypatch)
    cloud = cfg20k()["map"]
    assert len(cloud) == 20000
    a.AddCloudToLocalMap([cloud]); b.AddCloudToLocalMap([cloud])
    assert (b.map_size(140), b.map_size(141), host_flattens(b)) == (1, 0, 0)
    assert (a.map_size(140), host_flattens(a)) == (0, 1)
    assert a.map_size(101) == b.map_size(101) == 1  # one full build of the image either way
    assert b.map_size(147) == 0 and b.map_size(102) == a.map_size(102) and b.map_size() == a.map_size() == 20000  # (counts without a mirror)
    a.close(); b.close()


@pytest.mark.parametrize("loc", [False, True])
def test_map_equality(loc, monkeypatch):
    clouds = dict(hand_made())
    clouds["20k"] = cfg20k()["map"]
    clouds["300k"] = cloud300k()  # beyond the update chain's 262,144 points, several radix tiles
    a, b = handles(monkeypatch, loc)
    for k, (name, cloud) in enumerate(clouds.items()):
        if not loc and k > 0:  # a mapping handle takes a whole cloud once: a fresh pair per cloud (a localization pair reloads)
            a.close(); b.close()
            a, b = handles(monkeypatch, loc)
        a.AddCloudToLocalMap([cloud]); b.AddCloudToLocalMap([cloud])
        n140 = k + 1 if loc else 1
        assert b.map_size(140) == n140 and b.map_size(141) == 0, name
        assert (b.map_size(), b.map_size(102)) == (a.map_size(), a.map_size(102)), name
        before = b.map_size(147)
        assert same_export(a, b), name
        assert b.map_size(147) == before + 1, name  # the export built the mirror, once
        assert same_export(a, b) and b.map_size(147) == before + 1, name
    # both handles still match identically
    cfg = cfg20k()
    if loc:
        a.AddCloudToLocalMap([cfg["map"]]); b.AddCloudToLocalMap([cfg["map"]])
    else:
        a.close(); b.close()
        a, b = handles(monkeypatch, loc)
        a.AddCloudToLocalMap([cfg["map"]]); b.AddCloudToLocalMap([cfg["map"]])
        assert same_export(a, b)
    Ta, Tb = np.eye(4), np.eye(4)
    oka = a.Match(reg.PointcloudCluster(planar_cloud_=cfg["scan"]), Ta, update_map=not loc)
    okb = b.Match(reg.PointcloudCluster(planar_cloud_=cfg["scan"]), Tb, update_map=not loc)
    assert oka and okb and np.array_equal(Ta, Tb)
    for u, v in zip(a.correspondences(), b.correspondences()):
        assert np.array_equal(u, v)
    assert same_export(a, b)
    a.close(); b.close()


def test_slot_layout_under_exact_ties(monkeypatch):
    """A lattice map (every point of a 0.125 m grid in a 3 m cube, random insertion order) and queries at cell centres: many exactly equal d2
    across different voxels, so the neighbours chosen depend on the slot order of the image ((d2 bits, map slot) tie order)."""
    y = dict(Y, optimization_iter_num=1)
    g = np.arange(0.0, 3.0, 0.125)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    lattice = lattice[np.random.default_rng(3).permutation(len(lattice))]
    c = np.arange(0.25, 3.0, 0.25)
    queries = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    a, b = handles(monkeypatch, y=y)
    a.AddCloudToLocalMap([lattice]); b.AddCloudToLocalMap([lattice])
    assert b.map_size(140) == 1
    res = []
    for m in (a, b):
        T = np.eye(4)
        m.Match(reg.PointcloudCluster(planar_cloud_=queries), T, update_map=False)
        res.append((T, m.correspondences(), m.iteration_log()))
    assert np.array_equal(res[0][0], res[1][0])
    ids, cnt, valid = res[0][1]
    assert cnt.min() == 5  # every query has its five neighbours: ties are in play
    for u, v in zip(res[0][1], res[1][1]):
        assert np.array_equal(u, v)
    for u, v in zip(res[0][2], res[1][2]):
        assert np.array_equal(np.asarray(u), np.asarray(v))
    a.close(); b.close()


def test_localization_reloads_against_the_oracle():
    """Two successive reloads with different clouds on one localization handle: registration and fitness equal the oracle's."""
    cfgs = [synth.make_config(1, scale=0.05), synth.make_config(1, job=1, scale=0.05)]
    maps = [cfgs[0]["map"], cfgs[0]["map"][::2].copy()]  # the second reload: another cloud (every other point)
    b = reg.make_matcher(MODE, Y, is_localization_mode=True)
    o = util.oracle_for(MODE, Y, loc=True)
    for k in range(2):
        b.AddCloudToLocalMap([maps[k]]); o.AddCloudToLocalMap(maps[k])
        assert b.map_size(140) == k + 1 and host_flattens(b) == 0
        assert b.map_size() == o.map_size() and b.map_size(102) == o.map_voxels()
        T = np.eye(4)
        ok = b.Match(reg.PointcloudCluster(planar_cloud_=cfgs[k]["scan"]), T, update_map=False)
        ok_ref, T_ref = o.Match(cfgs[k]["scan"], np.eye(4), update_map=False)
        util.assert_same_registration(b, o, ok, T, ok_ref, T_ref, sets_only_tail=True, max_tie_rows=int(o.counters().tie_queries))
        fb, fo = b.GetFitnessScore(2.0), o.GetFitnessScore(2.0)
        print(f"reload {k}: fitness {fb!r} oracle {fo!r}")
        assert fb == fo
    assert b.map_size(147) == 0, "nothing here needs the mirror"
    b.close(); o.close()


def test_mapping_continues_on_the_device_from_the_bulk_built_image():
    from tests.test_gpu_parity import _replay
    m, o = _replay(6)  # every scan equals the oracle: ids, flags, n_valid, poses, map sizes
    assert m.map_size(140) == 1 and host_flattens(m) == 0
    assert m.map_size(103) > 0 and m.map_size(104) == 0
    assert m.map_size(147) == 0, "the device AddPoints continues from the image: no mirror"
    m.close(); o.close()


def test_later_evictions_follow_the_bulk_built_stamps(monkeypatch):
    """LRU capacity = first cloud's voxels + 50, then scans that create more: the device evicts by the stamps the bulk build wrote, and
    they must order the voxels as the mirror's list does."""
    scene = synth.make_scene()
    mp = synth.sample_map(scene, 20000, synth.rng_for(1, 0, 5), radius=18.0)
    probe = util.oracle_for(MODE, Y)
    probe.AddCloudToLocalMap(mp)
    V = probe.map_voxels()
    probe.close()
    monkeypatch.setenv("FLS_IVOX_CAPACITY", str(V + 50))
    a, b = handles(monkeypatch)
    a.AddCloudToLocalMap([mp]); b.AddCloudToLocalMap([mp])
    assert b.map_size(140) == 1 and b.map_size(102) == V
    rng = synth.rng_for(1, 12)
    Tgt, guess, created = np.eye(4), np.eye(4), 0
    for k in range(4):
        Tgt = Tgt @ synth.random_pose(rng, 1.0, 0.6)
        scan = synth.cast_scan(scene, Tgt, rng=rng, max_range=30.0, **dict(synth.VELODYNE_64, n_az=60))
        Ta, Tb = guess.copy(), guess.copy()
        oka = a.Match(reg.PointcloudCluster(planar_cloud_=scan), Ta, update_map=True)
        okb = b.Match(reg.PointcloudCluster(planar_cloud_=scan), Tb, update_map=True)
        assert oka and okb and np.array_equal(Ta, Tb), k
        assert same_export(a, b), k
        guess = Ta
    evicted = b.map_size(117)
    print(f"capacity {V + 50}: {evicted} voxels evicted on the device, {b.map_size(103)} device batches, {b.map_size(104)} host fallbacks")
    assert b.map_size(102) == V + 49 and evicted > 50, (b.map_size(102), evicted)
    a.close(); b.close()


def test_declines(monkeypatch):
    # as many voxels as the capacity: the sequential insert evicts
    monkeypatch.setenv("FLS_IVOX_CAPACITY", "64")
    a, b = handles(monkeypatch)
    monkeypatch.delenv("FLS_IVOX_CAPACITY")
    cloud = at_voxels([(v, v % 7, 0) for v in range(100)] * 2)
    a.AddCloudToLocalMap([cloud]); b.AddCloudToLocalMap([cloud])
    assert (b.map_size(140), b.map_size(141), b.map_size(143), host_flattens(b)) == (0, 1, 1, 1)
    assert b.map_size(102) == 63 and same_export(a, b)
    a.close(); b.close()
    # a NaN: FLS_ERR_RANGE from both, nothing inserted; the next valid cloud builds on the device
    for loc in (False, True):
        a, b = handles(monkeypatch, loc)
        bad = cfg20k()["map"][:1000].copy()
        bad[500, 1] = np.nan
        for m in (a, b):
            with pytest.raises(_lib.FlsError) as e:
                m.AddCloudToLocalMap([bad])
            assert e.value.status == _lib.FLS_ERR_RANGE
            assert m.map_size(0) == 0 and m.map_size(102) == 0
        assert (b.map_size(140), b.map_size(141), b.map_size(144)) == (0, 1, 1)
        a.AddCloudToLocalMap([cfg20k()["map"]]); b.AddCloudToLocalMap([cfg20k()["map"]])
        assert (b.map_size(140), b.map_size(141)) == (1, 1) and same_export(a, b)
        a.close(); b.close()
    # a point at the key limit
    a, b = handles(monkeypatch)
    far = cfg20k()["map"][:100].copy()
    far[7, 0] = np.float32(((1 << 20) - 2) * 0.5)
    for m in (a, b):
        with pytest.raises(_lib.FlsError) as e:
            m.AddCloudToLocalMap([far])
        assert e.value.status == _lib.FLS_ERR_RANGE and m.map_size(0) == 0
    assert (b.map_size(141), b.map_size(144)) == (1, 1)
    a.close(); b.close()
    # the hash-table form
    monkeypatch.setenv("FLS_IVOX_DENSE", "0")
    a, b = handles(monkeypatch)
    monkeypatch.delenv("FLS_IVOX_DENSE")
    cfg = cfg20k()
    a.AddCloudToLocalMap([cfg["map"]]); b.AddCloudToLocalMap([cfg["map"]])
    assert (b.map_size(140), b.map_size(141), b.map_size(146)) == (0, 1, 1)
    Ta, Tb = np.eye(4), np.eye(4)
    a.Match(reg.PointcloudCluster(planar_cloud_=cfg["scan"]), Ta, update_map=False)
    b.Match(reg.PointcloudCluster(planar_cloud_=cfg["scan"]), Tb, update_map=False)
    assert np.array_equal(Ta, Tb) and same_export(a, b)
    for u, v in zip(a.correspondences(), b.correspondences()):
        assert np.array_equal(u, v)
    a.close(); b.close()
    # an empty cloud: FLS_OK, counted nowhere
    b = reg.make_matcher(MODE, Y)
    b.AddCloudToLocalMap([np.zeros((0, 3), np.float32)])
    assert [b.map_size(s) for s in range(140, 148)] == [0] * 8 and b.map_size(0) == 0
    b.close()


def test_batch_and_replica_paths_read_a_complete_image_without_a_mirror(monkeypatch):
    n_jobs = 6
    cfgs = [synth.make_config(1, job=j, scale=0.05) for j in range(n_jobs)]
    b = reg.make_matcher(MODE, Y, is_localization_mode=True)
    b.AddCloudToLocalMap([cfgs[0]["map"]])
    assert b.map_size(140) == 1
    clusters = [reg.PointcloudCluster(planar_cloud_=c["scan"]) for c in cfgs]
    oks, Ts, stats = b.MatchBatch(clusters, [np.eye(4)] * n_jobs, lanes=3)
    rs = b.Replicas([0])
    oks_r, Ts_r, stats_r = rs.MatchBatch(clusters, [np.eye(4)] * n_jobs, lanes=3)
    monkeypatch.setenv("FLS_IVOX_DEVICE_BUILD", "0")
    for j, c in enumerate(cfgs):
        f = reg.make_matcher(MODE, Y, is_localization_mode=True)  # a fresh handle on the host-built map
        f.AddCloudToLocalMap([cfgs[0]["map"]])
        assert f.map_size(140) == 0
        T = np.eye(4)
        ok = f.Match(clusters[j], T, update_map=False)
        for okx, Tx, sx in ((oks[j], Ts[j], stats[j]), (oks_r[j], Ts_r[j], stats_r[j])):
            assert okx == ok and np.array_equal(Tx, T), j
            assert (sx.iterations, sx.n_valid) == (f.stats.iterations, f.stats.n_valid), j
        f.close()
    assert b.map_size(147) == 0, "read-only borrowers see a complete image: no mirror was built"
    rs.close(); b.close()
