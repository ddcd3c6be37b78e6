"""The NDT voxel map built from a whole cloud on the device (NdtMatcher::add_cloud_build -> NdtMap::build, ndt_upd_voxel_first in kernels_ndt_update.hpp): the
first AddCloudToLocalMap of every handle and every reload of a localization handle.  Two handles per test: A created with
FLS_NDT_DEVICE_BUILD=0 (host VoxelGrid, sequential insert, UpdateVoxel on one thread: the path every handle took before), B with the default.
B must be indistinguishable from A: every array of ndt_voxels() (include/fls_debug_ndt.h) equal, LRU order included, and Matches bit for bit;
and equal to the CPU oracle where the existing parity tests compare against it."""
import ctypes as C
import functools

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg, synth
from tests import replay, util

pytestmark = pytest.mark.gpu

MODE, Y = "IncrementalNDT", reg.YAML_NCLT_NDT
VOXEL, LEAF = Y["ndt_voxel_size"], Y["source_cloud_filter_size"]
KVG_TILE, KVG_SCAN_BLOCK = 256 * 4, 1024  # csrc/kernels_voxelgrid.hpp: keys per block of a radix pass, threads of a scan block
KNDT_CARRY = 8                            # csrc/kernels_ndt_update.hpp
KEY_LIMIT = (1 << 20) - 2                 # csrc/device_common.hpp
BUILD_SLOTS = range(150, 156)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"


def handles(monkeypatch, loc=False, y=Y):
    """(A, B): the switch is read when the handle is created"""
    monkeypatch.setenv("FLS_NDT_DEVICE_BUILD", "0")
    a = reg.make_matcher(MODE, y, is_localization_mode=loc)
    monkeypatch.delenv("FLS_NDT_DEVICE_BUILD")
    b = reg.make_matcher(MODE, y, is_localization_mode=loc)
    return a, b


def build_counts(m):
    return tuple(m.map_size(s) for s in BUILD_SLOTS)


def same_dump(a, b):
    da, db = a.ndt_voxels(), b.ndt_voxels()
    return [k for k in da if da[k].shape != db[k].shape or not np.array_equal(da[k], db[k])]


def filtered(cloud):
    return reg.VoxelGridCloud(cloud, LEAF, on_device=False)  # the reference's filter on the host


def n_voxels(cloud):
    f = filtered(cloud)[:, :3].astype(np.float64) * (1.0 / VOXEL)
    return len(np.unique(np.trunc(f).astype(np.int64), axis=0))


def axis_slots(k):
    """coordinates inside voxel k of one axis, more than one leaf apart (cast<int> truncates toward zero: voxel 0 is (-1, 1))"""
    if k == 0:
        return [-0.9 + 0.25 * i for i in range(8)]
    s = [abs(k) + 0.05 + 0.25 * i for i in range(4)]
    return s if k > 0 else [-v for v in s]


def in_voxel(key, n, rng):
    """n points of voxel `key`, each in a leaf cell of its own, in a random order"""
    g = np.array([(a, b, c) for c in axis_slots(key[2]) for b in axis_slots(key[1]) for a in axis_slots(key[0])], np.float32)
    assert n <= len(g)
    return g[rng.permutation(len(g))[:n]]


@functools.lru_cache(maxsize=None)
def cfg20k():
    return synth.make_config(2, scale=0.02)  # the 20,000-point cut of configs[2]


@functools.lru_cache(maxsize=None)
def cfg5pct():
    return synth.make_config(2, scale=0.05)


def hand_made():
    rng = np.random.default_rng(11)
    out = {"one point": np.array([[1.3, 2.4, 3.6]], np.float32)}
    for n in (1, 2, 3):
        out[f"{n} in one voxel"] = in_voxel((3, -2, 1), n, rng)
    out["200 in one voxel"] = in_voxel((0, 0, 0), 200, rng)  # a long serial segment: many trips of the batched loads, a short last one
    h = (0.3, -0.3, 0.9, -0.9, 1.3, -1.3)  # -0.3 and +0.3 share key 0
    out["truncation toward zero"] = np.array([(a, b, c) for a in h for b in h for c in h], np.float32)
    # the LRU pattern A B A A B: the filter hands the points on in ascending leaf index, z first
    zs = [1.02, 1.23, 1.44, 1.65, 1.86]
    out["ABAAB"] = np.array([(x, 1.5, z) for x, z in zip((1.5, 20.5, 1.5, 1.5, 20.5), zs)], np.float32)
    far = [(sx * 1000001.5, sy * 999983.5, sz * 1000003.5) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    f = np.array((far + [(0.5, 0.5, 0.5)]) * 1, np.float32)  # (an extent of > INT_MAX leaves: the filter hands the cloud on unfiltered)
    out["far corners"] = f[rng.permutation(len(f))]
    # several radix tiles and scan blocks, no multiple of either: a lattice with one point per leaf cell
    n_big = 3 * max(KVG_TILE, KVG_SCAN_BLOCK) + 17
    g = 0.25 * np.stack(np.meshgrid(np.arange(15), np.arange(15), np.arange(14), indexing="ij"), -1).reshape(-1, 3) - 1.6
    out["beyond one tile"] = g[rng.permutation(len(g))[:n_big]].astype(np.float32)
    for name, c in out.items():
        if name != "far corners":
            assert len(filtered(c)) == len(c), name  # every point survives the filter as itself
    assert len(out["beyond one tile"]) > KVG_TILE and len(out["beyond one tile"]) > KVG_SCAN_BLOCK
    return out


def test_counters(monkeypatch):
    a, b = handles(monkeypatch)
    cloud = cfg20k()["map"]
    assert len(cloud) == 20000
    a.AddCloudToLocalMap([cloud]); b.AddCloudToLocalMap([cloud])
    assert (b.map_size(150), b.map_size(151)) == (1, 0)
    assert (a.map_size(150), a.map_size(151)) == (0, 1) and build_counts(a)[2:] == (0, 0, 0, 0)  # the switch counts in no reason slot
    assert a.map_size() == b.map_size() > 0
    assert (b.map_size(109), b.map_size(110)) == (0, 0) and b.map_size(107) == 1  # a build is no incremental batch; one full build of the image
    a.close(); b.close()


@pytest.mark.parametrize("loc", [False, True])
def test_map_equality(loc, monkeypatch):
    clouds = dict(hand_made())
    clouds["20k"] = cfg20k()["map"]
    a, b = handles(monkeypatch, loc)
    for k, (name, cloud) in enumerate(clouds.items()):
        if not loc and k > 0:  # a mapping handle takes a whole cloud once: a fresh pair per cloud (a localization pair reloads)
            a.close(); b.close()
            a, b = handles(monkeypatch, loc)
        a.AddCloudToLocalMap([cloud]); b.AddCloudToLocalMap([cloud])
        assert (b.map_size(150), b.map_size(151)) == (k + 1 if loc else 1, 0), name
        assert (a.map_size(150), a.map_size(151)) == (0, k + 1 if loc else 1), name
        assert (b.map_size(109), b.map_size(110)) == (0, 0), name
        assert a.map_size() == b.map_size(), name
        assert same_dump(a, b) == [], name
        d = b.ndt_voxels()
        assert d["estimated"].all() and not d["pending"].any(), name
        if name == "200 in one voxel":
            assert len(d["vid"]) >= 1 and (np.abs(d["keys"][0]) == 0).all()
    cfg = cfg20k()
    Ta, Tb = cfg["T_init"].copy(), cfg["T_init"].copy()
    oka = a.Match(util.cluster_for(MODE, cfg["scan"]), Ta, update_map=not loc)
    okb = b.Match(util.cluster_for(MODE, cfg["scan"]), Tb, update_map=not loc)
    assert oka == okb and np.array_equal(Ta, Tb)
    for u, v in zip(a.correspondences(), b.correspondences()):
        assert np.array_equal(u, v)
    for u, v in zip(a.iteration_log(), b.iteration_log()):
        assert np.array_equal(u, v)
    assert same_dump(a, b) == []
    a.close(); b.close()


def _by_key(keys):
    return np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))


def test_localization_reloads_against_the_oracle():
    """Three reloads on one handle: existing voxels are overwritten from the new points alone; some get a single point, which leaves
    info = 100 I and the previous sigma."""
    cfg = cfg5pct()
    maps = [cfg["map"], cfg["map"][::2].copy(), (cfg["map"] + np.float32(0.37)).astype(np.float32)]
    b = reg.make_matcher(MODE, Y, is_localization_mode=True)
    o = util.oracle_for(MODE, Y, loc=True)
    single_with_history = 0
    for k, mp in enumerate(maps):
        b.AddCloudToLocalMap([mp]); o.AddCloudToLocalMap(mp)
        assert b.map_size(150) == k + 1 and b.map_size(151) == 0
        assert b.map_size() == o.map_size()
        d = b.ndt_voxels()
        ok_, omu, oinfo, oest, onp = o.ndt_dump()
        i, j = _by_key(d["keys"]), _by_key(ok_)
        assert np.array_equal(d["keys"][i], ok_[j])
        assert np.array_equal(d["mu"][i], omu[j])
        assert np.array_equal(d["info"].reshape(-1, 3, 3).transpose(0, 2, 1)[i], oinfo[j])
        assert np.array_equal(d["estimated"][i], oest[j]) and np.array_equal(d["num_points"][i], onp[j])
        hundred = (d["info"] == (100.0 * np.eye(3)).reshape(-1)).all(1)
        single_with_history += int((hundred & (d["sigma"] != 0.0).any(1)).sum())
        T = cfg["T_init"].copy()
        ok = b.Match(util.cluster_for(MODE, cfg["scan"]), T, update_map=False)
        ok_ref, T_ref = o.Match(cfg["scan"], cfg["T_init"], update_map=False)
        util.assert_same_registration(b, o, ok, T, ok_ref, T_ref, sets_only_tail=False, max_tie_rows=int(o.counters().tie_queries))
        fb, fo = b.GetFitnessScore(2.0), o.GetFitnessScore(2.0)
        print(f"reload {k}: {b.map_size()} voxels, fitness {fb!r} oracle {fo!r}")
        assert fb == fo
    assert single_with_history > 0, "a reload must leave a single point in a voxel that had an estimate"
    assert b.map_size(150) == len(maps) and b.map_size(109) == b.map_size(110) == 0
    b.close(); o.close()


def test_mapping_continues_on_the_built_image():
    """tests/test_gpu_mapping_replay.py::run_replay's per-frame assertions on the "ndt_dev" scenario: the first cloud is built on the device
    and every later update is a device batch on the same image -- no host-path update in between."""
    r = replay.make_replay("ndt_dev")
    mode, y = r["mode"], r["y"]
    m = reg.make_matcher(mode, y)
    o = util.oracle_for(mode, y)
    m.AddCloudToLocalMap(r["init_clouds"])
    o.AddCloudToLocalMap(*r["init_clouds"])
    assert m.map_size(0) == o.map_size(0)
    assert (m.map_size(150), m.map_size(151)) == (1, 0)
    Tprev = np.eye(4)
    updates = 0
    for k, f in enumerate(r["frames"]):
        guess = Tprev @ f["guess_step"]
        T = guess.copy()
        ok = m.Match(util.cluster_for(mode, f["scan"], f["corner"]), T, update_map=True)
        ok_ref, T_ref = o.Match(f["scan"], guess, src1=f["corner"], update_map=True)
        util.assert_same_registration(m, o, ok, T, ok_ref, T_ref, sets_only_tail=False, max_tie_rows=int(o.counters().tie_queries))
        assert m.stats.map_updated == o.stats.map_updated, k
        assert m.stats.n_source == o.stats.n_source, k
        assert m.map_size(0) == o.map_size(0), (k, m.map_size(0), o.map_size(0))
        updates += int(o.stats.map_updated)
        Tprev = T_ref
    n = len(r["frames"])
    assert updates == n
    assert m.map_size(150) == 1 and m.map_size(109) >= n - 1 and m.map_size(110) == 0
    assert (m.map_size(107), m.map_size(108)) == (1, 0), "the image was built once, on the device, and never synchronised from the host mirror"
    m.close(); o.close()


def test_evictions_on_the_device_in_a_reload(monkeypatch):
    """(a) capacity a little above the first cloud's voxel count; a second, disjoint cloud evicts old, untouched voxels inside the device batch"""
    c1 = cfg20k()["map"]
    c2 = (c1[::8] + np.array([300.0, 0.0, 0.0], np.float32)).astype(np.float32)
    v1, v2 = n_voxels(c1), n_voxels(c2)
    assert 50 < v2 < v1
    y = dict(Y, ndt_capacity=v1 + 50)
    a, b = handles(monkeypatch, True, y)
    for c in (c1, c2):
        a.AddCloudToLocalMap([c]); b.AddCloudToLocalMap([c])
        assert same_dump(a, b) == []
    assert a.map_size() == b.map_size() == v1 + 49
    assert b.map_size(117) == v2 - 49 and (b.map_size(150), b.map_size(151)) == (2, 0)
    a.close(); b.close()


def test_a_first_cloud_beyond_the_capacity_is_the_hosts(monkeypatch):
    """(b) with an empty map every eviction reaches a voxel of the batch itself"""
    rng = np.random.default_rng(5)
    cloud = np.concatenate([in_voxel((v + 1, v % 7, 0), 2, rng) for v in range(100)])
    a, b = handles(monkeypatch, False, dict(Y, ndt_capacity=64))
    a.AddCloudToLocalMap([cloud]); b.AddCloudToLocalMap([cloud])
    assert build_counts(b) == (0, 1, 0, 1, 0, 0)
    assert (b.map_size(109), b.map_size(110)) == (0, 0)
    assert a.map_size() == b.map_size() == 63 and same_dump(a, b) == []
    a.close(); b.close()


@pytest.mark.parametrize("loc", [False, True])
def test_a_key_out_of_range_leaves_no_trace(loc, monkeypatch):
    cfg = cfg20k()
    bad = cfg["map"][:1000].copy()
    bad[500, 1] = np.float32((KEY_LIMIT + 10) * VOXEL)
    a, b = handles(monkeypatch, loc)
    for m in (a, b):  # an empty handle
        with pytest.raises(_lib.FlsError) as e:
            m.AddCloudToLocalMap([bad])
        assert e.value.status == _lib.FLS_ERR_RANGE and m.map_size() == 0 and len(m.ndt_voxels()["vid"]) == 0
    assert build_counts(b) == (0, 1, 0, 0, 1, 0)
    a.AddCloudToLocalMap([cfg["map"]]); b.AddCloudToLocalMap([cfg["map"]])
    assert (b.map_size(150), b.map_size(151)) == (1, 1) and same_dump(a, b) == []
    fit = []
    for m in (a, b):  # after a successful build
        T = cfg["T_init"].copy()
        m.Match(util.cluster_for(MODE, cfg["scan"]), T, update_map=False)
        before, f0 = m.ndt_voxels(), m.GetFitnessScore(2.0)
        with pytest.raises(_lib.FlsError) as e:
            m.AddCloudToLocalMap([bad])
        assert e.value.status == _lib.FLS_ERR_RANGE
        after, f1 = m.ndt_voxels(), m.GetFitnessScore(2.0)
        assert all(np.array_equal(before[k], after[k]) for k in before) and f0 == f1
        fit.append(f1)
    assert fit[0] == fit[1]
    # (a mapping handle's second cloud is an incremental update, not a build: only the reload of a localization handle counts again)
    assert build_counts(b) == ((1, 2, 0, 0, 2, 0) if loc else (1, 1, 0, 0, 1, 0))
    assert (b.map_size(109), b.map_size(110)) == (0, 0) and same_dump(a, b) == []
    a.close(); b.close()


def test_other_declines(monkeypatch):
    cloud = cfg20k()["map"]
    # more unconsumed points per voxel than a device row carries
    a, b = handles(monkeypatch, False, dict(Y, ndt_min_points_in_voxel=KNDT_CARRY + 1))
    a.AddCloudToLocalMap([cloud]); b.AddCloudToLocalMap([cloud])
    assert build_counts(b) == (0, 1, 0, 0, 0, 1) and same_dump(a, b) == []
    a.close(); b.close()
    # the device VoxelGrid switched off: nothing on the device has the host filter's bits
    monkeypatch.setenv("FLS_DEVICE_VOXELGRID", "0")
    a, b = handles(monkeypatch, True)
    a.AddCloudToLocalMap([cloud]); b.AddCloudToLocalMap([cloud])
    a.AddCloudToLocalMap([cloud[::2]]); b.AddCloudToLocalMap([cloud[::2]])
    assert build_counts(b) == (0, 2, 0, 0, 0, 2) and same_dump(a, b) == []
    a.close(); b.close()
    monkeypatch.delenv("FLS_DEVICE_VOXELGRID")
    # a NaN: the host filter drops the point, the device filter hands the cloud to the host
    nan = cloud[:2000].copy()
    nan[77, 2] = np.nan
    a, b = handles(monkeypatch, True)
    a.AddCloudToLocalMap([nan]); b.AddCloudToLocalMap([nan])
    assert build_counts(b) == (0, 1, 0, 0, 1, 0) and same_dump(a, b) == []
    a.AddCloudToLocalMap([cloud]); b.AddCloudToLocalMap([cloud])  # the next reload is built on the device, on top of the host-built map
    assert (b.map_size(150), b.map_size(151)) == (1, 1) and same_dump(a, b) == []
    a.close(); b.close()
    # an empty cloud: FLS_OK, counted nowhere
    b = reg.make_matcher(MODE, Y)
    b.AddCloudToLocalMap([np.zeros((0, 3), np.float32)])
    assert build_counts(b) == (0,) * 6 and b.map_size() == 0
    b.close()
    # FLS_NDT_DEVICE_UPDATE=0 alone: the handle stays on the host
    monkeypatch.setenv("FLS_NDT_DEVICE_UPDATE", "0")
    b = reg.make_matcher(MODE, Y)
    monkeypatch.delenv("FLS_NDT_DEVICE_UPDATE")
    b.AddCloudToLocalMap([cloud])
    assert build_counts(b) == (0, 1, 0, 0, 0, 0) and (b.map_size(109), b.map_size(110)) == (0, 0)
    b.close()


def test_batch_lanes_read_the_built_image(monkeypatch):
    cfgs = [synth.make_config(2, job=j, scale=0.02) for j in range(3)]
    b = reg.make_matcher(MODE, Y, is_localization_mode=True)
    b.AddCloudToLocalMap([cfgs[0]["map"]])
    assert b.map_size(150) == 1
    clusters = [util.cluster_for(MODE, c["scan"]) for c in cfgs]
    oks, Ts, stats = b.MatchBatch(clusters, [c["T_init"] for c in cfgs], lanes=3)
    monkeypatch.setenv("FLS_NDT_DEVICE_BUILD", "0")
    for j, c in enumerate(cfgs):
        f = reg.make_matcher(MODE, Y, is_localization_mode=True)  # a fresh handle on the host-built map
        f.AddCloudToLocalMap([cfgs[0]["map"]])
        assert f.map_size(150) == 0
        T = c["T_init"].copy()
        ok = f.Match(clusters[j], T, update_map=False)
        assert oks[j] == ok and np.array_equal(Ts[j], T), j
        assert (stats[j].iterations, stats[j].n_valid) == (f.stats.iterations, f.stats.n_valid), j
        f.close()
    b.close()


def test_read_out_arguments(monkeypatch):
    """what tests/test_debug_ndt_abi.py cannot reach without a handle: another kind, NULL arrays, a buffer too small"""
    L = _lib.lib()
    n = C.c_size_t(0)
    other = reg.make_matcher("PointToPlane_IVOX", reg.YAML_NCLT_IVOX)
    assert L.fls_debug_ndt_voxels(other._h, 0, *([None] * 8), C.byref(n)) == _lib.FLS_ERR_INVALID
    other.close()
    b = reg.make_matcher(MODE, Y)
    b.AddCloudToLocalMap([hand_made()["truncation toward zero"]])
    i32 = np.zeros(64 * 3, np.int32); u8 = np.zeros(64, np.uint8); f64 = np.zeros(64 * 9)
    ip, bp, dp = i32.ctypes.data_as(C.POINTER(C.c_int32)), u8.ctypes.data_as(C.POINTER(C.c_uint8)), f64.ctypes.data_as(C.POINTER(C.c_double))
    full = [ip, ip, ip, bp, bp, dp, dp, dp]
    for k in range(8):
        q = list(full); q[k] = None
        assert L.fls_debug_ndt_voxels(b._h, 64, *q, C.byref(n)) == _lib.FLS_ERR_INVALID, k
    assert L.fls_debug_ndt_voxels(b._h, 64, *full, None) == _lib.FLS_ERR_INVALID
    assert L.fls_debug_ndt_voxels(b._h, 1, *full, C.byref(n)) == _lib.FLS_ERR_NOMEM and n.value == b.map_size() == 27
    assert not i32.any() and not u8.any() and not f64.any()
    before = build_counts(b), b.map_size(107), b.map_size(109)
    d = b.ndt_voxels()
    assert len(d["vid"]) == 27 and sorted(d["vid"]) == list(range(27)) and (build_counts(b), b.map_size(107), b.map_size(109)) == before
    b.close()
