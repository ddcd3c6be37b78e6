"""The iVox map's FLSIVOX1 blob packed from and built into the device image (include/fls_map_ivox.h: fls_ivox_map_bytes / _export / _import;
IvoxMap::export_blob_device / import_blob_device, kernels_ivox_blob.hpp).  Two kinds of handle: A created with FLS_IVOX_DEVICE_IMAGE=0 (the host
writer and fls_map_import's host path, what every handle did before) and B with the default.  Every comparison is bit for bit: the new calls
must write the bytes fls_map_export writes and leave a handle that fls_map_import's cannot be told from -- exports, poses, correspondences and
iteration logs of the mapping that follows, exact distance ties included.

A handle's own next Match after an export is NOT what a fresh importer computes (its nearest_points_ of the last scan persist, the importer
has none: tests/test_gpu_parity.py says the same of fls_map_import), so "the importer continues the exporter's run" is checked on the exporter
itself: it takes its own blob back from its own device buffer -- checkpoint and resume on one handle -- and must then agree with A and B."""
import functools

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg, synth
from tests import util
from tests.test_gpu_ivox_build import MODE, Y, cfg20k, cloud300k, hand_made
from tests.test_gpu_ndt_image import DevMem

pytestmark = pytest.mark.gpu

HDR = np.dtype([("magic", "S8"), ("version", "<u4"), ("kind", "<u4"), ("resolution", "<f4"), ("is_first", "<u4"), ("capacity", "<u8"), ("n_voxels", "<u8"),
                ("n_points", "<u8"), ("next_id", "<i8")])
VOX = np.dtype([("key", "<u8"), ("count", "<u4"), ("pad", "<u4")])
PT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("id", "<i4")])
OFF = {"FLS_IVOX_DEVICE_IMAGE": "0"}
MEM = ["host", "device"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"
    assert HDR.itemsize == _lib.IVOX_BLOB_HEADER_BYTES and VOX.itemsize == _lib.IVOX_BLOB_VOXEL_BYTES and PT.itemsize == _lib.IVOX_BLOB_POINT_BYTES


def make(monkeypatch, env=None, loc=False, y=Y):
    """the switches are read when the handle is created"""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    m = reg.make_matcher(MODE, y, is_localization_mode=loc)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return m


def blob_of(m, mem):
    """ExportMapBlob into host or device memory; the bytes"""
    n = m.MapBlobBytes()
    assert n >= HDR.itemsize
    if mem == "host":
        out = np.full(n, 0xA5, np.uint8)
        m.ExportMapBlob(out.ctypes.data, n, False)
        return out
    d = DevMem(n)
    m.ExportMapBlob(d.p.value, n, True)
    out = d.host()
    d.free()
    return out


def take_blob(m, blob, mem):
    """ImportMapBlob from host or device memory"""
    if mem == "host":
        m.ImportMapBlob(blob.ctypes.data, blob.size, False)
        return
    d = DevMem(blob.size, fill=blob)
    try:
        m.ImportMapBlob(d.p.value, blob.size, True)
    finally:
        d.free()


def parse(blob):
    """views into the blob: header record, voxel records, points"""
    h = blob[:HDR.itemsize].view(HDR)
    nv = int(h["n_voxels"][0])
    return h, blob[HDR.itemsize:HDR.itemsize + 16 * nv].view(VOX), blob[HDR.itemsize + 16 * nv:].view(PT)


def pack_key(x, y, z):
    return ((x & 0x1FFFFF) << 42) | ((y & 0x1FFFFF) << 21) | (z & 0x1FFFFF)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def run_setup(evict):
    """(map, LRU capacity or None, six scans).  evict: the set-up of test_later_evictions_follow_the_bulk_built_stamps (capacity = the first
    cloud's voxels + 50); otherwise the 20k map of configs[1] and the default capacity.  The scans leave the mapped disc, so every one creates voxels."""
    scene = synth.make_scene()
    if evict:
        mp = synth.sample_map(scene, 20000, synth.rng_for(1, 0, 5), radius=18.0)
        probe = util.oracle_for(MODE, Y)
        probe.AddCloudToLocalMap(mp)
        cap = probe.map_voxels() + 50
        probe.close()
    else:
        mp, cap = cfg20k()["map"], None
    rng = synth.rng_for(1, 12)
    Tgt, scans = np.eye(4), []
    for _ in range(6):
        Tgt = Tgt @ synth.random_pose(rng, 1.0, 0.6)
        scans.append(synth.cast_scan(scene, Tgt, rng=rng, max_range=30.0, **dict(synth.VELODYNE_64, n_az=60)))
    return mp, cap, scans


def with_capacity(monkeypatch, cap):
    if cap is not None:
        monkeypatch.setenv("FLS_IVOX_CAPACITY", str(cap))


def drive(m, scans, guess):
    """Match(update_map=True) per scan from the previous pose: everything the call leaves behind, as bytes; the last pose"""
    out = []
    for s in scans:
        T = guess.copy()
        ok = m.Match(reg.PointcloudCluster(planar_cloud_=s), T, update_map=True)
        out.append((ok, T.tobytes(), m.stats.iterations, m.stats.n_valid, m.stats.map_updated, [a.tobytes() for a in m.correspondences()],
                    [np.asarray(a).tobytes() for a in m.iteration_log()], m.ExportMap().tobytes()))
        guess = T
    return out, guess


# ---------------------------------------------------------------- export ----------------------------------------------------------------
def check_export(b, twin, name, device_packs=True):
    """ExportMapBlob of b, to host and to device memory, against ExportMap of a twin that saw the same calls -- before b's own ExportMap (which
    builds the mirror: slot 147) and after it"""
    want = twin.ExportMap()
    before = [b.map_size(s) for s in range(100, 148)]
    n168, n169 = b.map_size(168), b.map_size(169)
    assert b.MapBlobBytes() == want.size, name
    for mem in MEM:
        assert same(blob_of(b, mem), want), (name, mem)
    assert [b.map_size(s) for s in range(100, 148)] == before, (name, "no counter moves: no mirror, no rebuild")
    packed = (b.map_size(168) - n168, b.map_size(169) - n169)
    print(f"{name}: exports packed on the device / written by the host {packed}")
    assert packed == ((2, 0) if device_packs else (0, 2)) if device_packs is not None else sum(packed) == 2, name
    assert same(b.ExportMap(), want), name
    for mem in MEM:
        assert same(blob_of(b, mem), want), (name, mem, "after the handle's own ExportMap")
    return want


def test_export_bytes_of_first_builds(monkeypatch):
    clouds = dict(hand_made())
    clouds["20k"] = cfg20k()["map"]
    for name, cloud in clouds.items():
        b, twin = make(monkeypatch), make(monkeypatch)
        b.AddCloudToLocalMap([cloud]); twin.AddCloudToLocalMap([cloud])
        assert b.map_size(140) == 1 and b.map_size(147) == 0, name
        blob = check_export(b, twin, name)
        assert b.map_size(147) == 1, name  # (only the handle's own ExportMap built the mirror)
        h, vox, pts = parse(blob)
        assert (h["magic"][0], int(h["version"][0]), int(h["kind"][0]), float(h["resolution"][0])) == (b"FLSIVOX1", 1, _lib.P2PLANE_IVOX, 0.5), name
        assert int(h["n_points"][0]) == int(h["next_id"][0]) == len(cloud) == int(vox["count"].sum()) and not vox["pad"].any(), name
        # written out by hand, independent of the library: voxel order (oldest first), counts, ids
        if name == "ABAAB":  # A's last member is point 3, B's point 4: A is the older voxel
            assert vox["key"].tolist() == [pack_key(1, 1, 1), pack_key(20, 1, 1)] and vox["count"].tolist() == [3, 2]
            assert pts["id"].tolist() == [0, 2, 3, 1, 4]
            assert np.array_equal(np.stack([pts["x"], pts["y"], pts["z"]], 1), cloud[[0, 2, 3, 1, 4]])
        if name == "37 in one voxel":
            assert vox["key"].tolist() == [pack_key(3, -2, 1)] and vox["count"].tolist() == [37] and pts["id"].tolist() == list(range(37))
            assert np.array_equal(np.stack([pts["x"], pts["y"], pts["z"]], 1), cloud)
        b.close(); twin.close()


@pytest.mark.parametrize("evict", [False, True])
def test_export_bytes_after_updates(evict, monkeypatch):
    """four Match(update_map=True) scans on the device: regions relocated, garbage in the point array, the layout no longer sorted; with the
    capacity just above the first cloud's voxels the scans evict as well"""
    mp, cap, scans = run_setup(evict)
    with_capacity(monkeypatch, cap)
    b, twin = make(monkeypatch), make(monkeypatch)
    b.AddCloudToLocalMap([mp]); twin.AddCloudToLocalMap([mp])
    gb = gt = np.eye(4)
    for k in range(4):
        Tb, Tt = gb.copy(), gt.copy()
        assert b.Match(reg.PointcloudCluster(planar_cloud_=scans[k]), Tb, update_map=True)
        assert twin.Match(reg.PointcloudCluster(planar_cloud_=scans[k]), Tt, update_map=True)
        assert np.array_equal(Tb, Tt), k
        gb, gt = Tb, Tt
    print(f"evict={evict}: {b.map_size(103)} device batches, {b.map_size(104)} host fallbacks, {b.map_size(117)} voxels evicted on the device")
    assert b.map_size(103) >= 1 and (b.map_size(117) > 50) == evict
    if not evict:
        assert b.map_size(103) == 4 and b.map_size(104) == 0 and b.map_size(147) == 0, "four device batches, no mirror so far"
    # (a batch the eviction selection refuses is replayed on the host and leaves the map there until the next Match: either writer may answer then)
    check_export(b, twin, f"after updates, evict={evict}", device_packs=None if evict and b.map_size(104) else True)
    b.close(); twin.close()


def test_export_bytes_of_a_localization_handle_and_a_host_held_map(monkeypatch):
    cfg = cfg20k()
    b, twin = make(monkeypatch, loc=True), make(monkeypatch, loc=True)
    b.AddCloudToLocalMap([cfg["map"]]); twin.AddCloudToLocalMap([cfg["map"]])
    assert b.map_size(140) == 1  # (ImageOnly: nothing on the device updates it)
    check_export(b, twin, "localization")
    b.close(); twin.close()
    # the host holds the map: inserted point by point, updated on the host
    host = {"FLS_IVOX_DEVICE_UPDATE": "0", "FLS_IVOX_DEVICE_BUILD": "0"}
    b, twin = make(monkeypatch, host), make(monkeypatch, host)
    for m in (b, twin):
        m.AddCloudToLocalMap([cfg["map"]])
        T = np.eye(4)
        assert m.Match(reg.PointcloudCluster(planar_cloud_=cfg["scan"]), T, update_map=True)
    assert b.map_size(103) == 0 and b.map_size(140) == 0
    check_export(b, twin, "host-held", device_packs=False)
    b.close(); twin.close()
    # the switch sends a device-held map through the host writer too
    a, twin = make(monkeypatch, OFF), make(monkeypatch)
    a.AddCloudToLocalMap([cfg["map"]]); twin.AddCloudToLocalMap([cfg["map"]])
    want = twin.ExportMap()
    for mem in MEM:
        assert same(blob_of(a, mem), want), mem
    assert (a.map_size(168), a.map_size(169), a.map_size(147)) == (0, 2, 1)
    # too small a buffer, a replica, another kind
    small = np.zeros(want.size - 1, np.uint8)
    with pytest.raises(_lib.FlsError) as e:
        twin.ExportMapBlob(small.ctypes.data, small.size, False)
    assert e.value.status == _lib.FLS_ERR_RANGE
    r = make(monkeypatch)
    n = twin.MapImageBytes()
    img = np.zeros(n, np.uint8)
    twin.ExportMapImage(img.ctypes.data, n, False)
    r.ImportMapImage(img.ctypes.data, n, False)
    assert r.MapBlobBytes() == 0
    with pytest.raises(_lib.FlsError) as e:
        r.ExportMapBlob(img.ctypes.data, n, False)
    assert e.value.status == _lib.FLS_ERR_STATE
    ndt = reg.make_matcher("IncrementalNDT", reg.YAML_NCLT_NDT)
    assert ndt.MapBlobBytes() == 0
    with pytest.raises(_lib.FlsError) as e:
        ndt.ImportMapBlob(want.ctypes.data, want.size, False)
    assert e.value.status == _lib.FLS_ERR_STATE
    r.close(); ndt.close(); a.close(); twin.close()


# ---------------------------------------------------------------- import ----------------------------------------------------------------
@pytest.mark.parametrize("evict", [False, True])
@pytest.mark.parametrize("mem", MEM)
def test_import_equality_and_the_mapping_that_follows(mem, evict, monkeypatch):
    mp, cap, scans = run_setup(evict)
    with_capacity(monkeypatch, cap)
    e, a, b = make(monkeypatch), make(monkeypatch, OFF), make(monkeypatch)
    e.AddCloudToLocalMap([mp])
    _, guess = drive(e, scans[:2], np.eye(4))  # the blob is taken from the middle of a run
    blob = blob_of(e, mem)
    a.ImportMap(blob)
    take_blob(b, blob, mem)
    take_blob(e, blob, mem)  # checkpoint and resume on one handle: over a map the device has been updating
    for m in (b, e):
        assert m.map_size(170) == 1 and m.map_size(171) == 0
    assert b.map_size(147) == 0 and b.map_size(101) == 1 and a.map_size(101) == 1  # no mirror; one full build of the image either way
    assert (b.map_size(), b.map_size(102)) == (a.map_size(), a.map_size(102)) == (e.map_size(), e.map_size(102))
    assert same(blob_of(b, mem), blob) and b.map_size(147) == 0
    ea = a.ExportMap()
    assert same(ea, blob) and same(b.ExportMap(), ea) and same(e.ExportMap(), ea)
    assert b.map_size(147) == 1
    ra, _ = drive(a, scans[2:], guess)
    rb, _ = drive(b, scans[2:], guess)
    re_, _ = drive(e, scans[2:], guess)
    for k, (x, y, z) in enumerate(zip(ra, rb, re_)):
        assert x[0] and x[4] == 1, k  # converged, the map was updated
        assert x == y, (k, "B against A")
        assert x == z, (k, "the exporter resumed from its own blob against A")
    assert (b.map_size(103), b.map_size(104)) == (a.map_size(103), a.map_size(104)) and b.map_size(103) >= 1
    if not evict:
        assert b.map_size(103) == 4 and b.map_size(104) == 0
    if evict:
        assert b.map_size(117) > 0 and b.map_size(117) == a.map_size(117)
    for m in (e, a, b):
        m.close()


def test_import_under_exact_ties(monkeypatch):
    """the lattice map and the cell-centre queries of test_slot_layout_under_exact_ties: the neighbours chosen depend on the slot order of the image"""
    y = dict(Y, optimization_iter_num=1)
    g = np.arange(0.0, 3.0, 0.125)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    lattice = lattice[np.random.default_rng(3).permutation(len(lattice))]
    c = np.arange(0.25, 3.0, 0.25)
    queries = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    e, a, b = make(monkeypatch, y=y), make(monkeypatch, OFF, y=y), make(monkeypatch, y=y)
    e.AddCloudToLocalMap([lattice])
    blob = blob_of(e, "device")
    a.ImportMap(blob)
    take_blob(b, blob, "device")
    assert b.map_size(170) == 1
    res = []
    for m in (a, b):
        T = np.eye(4)
        m.Match(reg.PointcloudCluster(planar_cloud_=queries), T, update_map=False)
        res.append((T, m.correspondences(), m.iteration_log()))
    assert np.array_equal(res[0][0], res[1][0])
    assert res[0][1][1].min() == 5  # every query has its five neighbours: ties are in play
    for u, v in zip(res[0][1], res[1][1]):
        assert np.array_equal(u, v)
    for u, v in zip(res[0][2], res[1][2]):
        assert np.array_equal(np.asarray(u), np.asarray(v))
    for m in (e, a, b):
        m.close()


def test_device_only_round_trip_batch_and_replicas(monkeypatch):
    """export into a device buffer, import from it on a second handle: no host copy of the blob exists"""
    n_jobs = 4
    cfgs = [synth.make_config(1, job=j, scale=0.02) for j in range(n_jobs)]
    for loc in (False, True):
        e, b = make(monkeypatch, loc=loc), make(monkeypatch, loc=loc)
        e.AddCloudToLocalMap([cfgs[0]["map"]])
        n = e.MapBlobBytes()
        d = DevMem(n)
        e.ExportMapBlob(d.p.value, n, True)
        b.ImportMapBlob(d.p.value, n, True)
        d.free()
        assert (e.map_size(168), b.map_size(170), e.map_size(147), b.map_size(147)) == (1, 1, 0, 0)
        clusters = [reg.PointcloudCluster(planar_cloud_=c["scan"]) for c in cfgs]
        oke, Te, se = e.MatchBatch(clusters, [np.eye(4)] * n_jobs, lanes=2)
        okb, Tb, sb = b.MatchBatch(clusters, [np.eye(4)] * n_jobs, lanes=2)
        rs = b.Replicas([0])
        okr, Tr, sr = rs.MatchBatch(clusters, [np.eye(4)] * n_jobs, lanes=2)
        assert list(oke) == list(okb) == list(okr)
        assert np.array_equal(Te, Tb) and np.array_equal(Te, Tr)
        for x, y_, z in zip(se, sb, sr):
            assert (x.iterations, x.n_valid) == (y_.iterations, y_.n_valid) == (z.iterations, z.n_valid)
        assert b.map_size(147) == 0, "readers of the image need no mirror"
        if loc:  # the fitness grid is left as fls_map_import leaves it
            a = make(monkeypatch, OFF, loc=True)
            a.ImportMap(e.ExportMap())
            out = []
            for m in (a, b):
                T = np.eye(4)
                m.Match(clusters[0], T, update_map=False)
                try:
                    out.append((T.tobytes(), m.GetFitnessScore(2.0)))
                except _lib.FlsError as err:
                    out.append((T.tobytes(), err.status))
            assert out[0] == out[1]
            a.close()
        rs.close(); e.close(); b.close()


def bad_blobs(good):
    """name -> a blob fls_ivox_map_import must refuse"""
    out = {"truncated by a record": good[:-16].copy(), "truncated inside the header": good[:40].copy(), "ragged": good[:-3].copy()}

    def edited(name):
        out[name] = good.copy()
        return parse(out[name])
    h, vox, pts = edited("bad magic"); h["magic"] = b"FLSIVOX2"
    h, vox, pts = edited("wrong kind"); h["kind"] = _lib.INCREMENTAL_NDT
    h, vox, pts = edited("other resolution"); h["resolution"] = 0.25
    h, vox, pts = edited("a zero count"); vox["count"][4] += vox["count"][3]; vox["count"][3] = 0  # (the counts still sum)
    h, vox, pts = edited("counts that do not sum"); vox["count"][5] += 1
    h, vox, pts = edited("counts that sum modulo 2^32")
    old = int(vox["count"][5])
    vox["count"][5] = 0xFFFFFFFF
    vox["count"][6] = (int(vox["count"][6]) + old + 1) & 0xFFFFFFFF
    h, vox, pts = edited("a duplicated key"); vox["key"][7] = vox["key"][2]
    h, vox, pts = edited("next_id < n_points"); h["next_id"] = int(h["n_points"][0]) - 1
    return out


def test_rejections_leave_the_handle_as_it_was(monkeypatch):
    cfg = cfg20k()
    m = make(monkeypatch)
    m.AddCloudToLocalMap([cfg["map"]])
    T = np.eye(4)
    assert m.Match(reg.PointcloudCluster(planar_cloud_=cfg["scan"]), T, update_map=True)
    good = blob_of(m, "host")
    probe = [reg.PointcloudCluster(planar_cloud_=cfg["scan"])]  # (a batch job has fresh per-job state: the same answer every time)
    ok0, T0, s0 = m.MatchBatch(probe, [np.eye(4)], lanes=1)
    counters = [m.map_size(s) for s in list(range(100, 148)) + [170, 171, 172, 173, 174, 175]]
    for name, bad in bad_blobs(good).items():
        for mem in MEM:
            with pytest.raises(_lib.FlsError) as e:
                take_blob(m, bad, mem)
            assert e.value.status == _lib.FLS_ERR_INVALID, (name, mem)
            assert same(blob_of(m, "host"), good), (name, mem)
            ok1, T1, s1 = m.MatchBatch(probe, [np.eye(4)], lanes=1)
            assert list(ok1) == list(ok0) and np.array_equal(T1, T0) and (s1[0].iterations, s1[0].n_valid) == (s0[0].iterations, s0[0].n_valid), (name, mem)
    assert [m.map_size(s) for s in list(range(100, 148)) + [170, 171, 172, 173, 174, 175]] == counters
    # and it still maps on the device
    T = np.eye(4)
    assert m.Match(reg.PointcloudCluster(planar_cloud_=cfg["scan"]), T, update_map=True) and m.map_size(103) == 2 and m.map_size(104) == 0
    m.close()


def test_declines_land_in_their_slots(monkeypatch):
    cfg = cfg20k()
    e = make(monkeypatch)
    e.AddCloudToLocalMap([cfg["map"]])
    blob = blob_of(e, "device")
    V = e.map_size(102)
    cases = {"switch": (OFF, {171: 1, 172: 0, 173: 0, 174: 0, 175: 0}),
             "hash-table form": ({"FLS_IVOX_DENSE": "0"}, {171: 1, 172: 0, 173: 0, 174: 0, 175: 1}),
             "n_voxels >= capacity": ({"FLS_IVOX_CAPACITY": str(V)}, {171: 1, 172: 1, 173: 0, 174: 0, 175: 0})}
    for name, (env, slots) in cases.items():
        for mem in MEM:
            a, b = make(monkeypatch, dict(env, **OFF)), make(monkeypatch, env)
            a.ImportMap(blob)
            take_blob(b, blob, mem)
            assert b.map_size(170) == 0 and {s: b.map_size(s) for s in slots} == slots, (name, mem)
            assert (b.map_size(), b.map_size(102)) == (a.map_size(), a.map_size(102)) == (e.map_size(), V), (name, mem)
            Ta, Tb = np.eye(4), np.eye(4)
            oka = a.Match(reg.PointcloudCluster(planar_cloud_=cfg["scan"]), Ta, update_map=True)
            okb = b.Match(reg.PointcloudCluster(planar_cloud_=cfg["scan"]), Tb, update_map=True)
            assert oka and okb and np.array_equal(Ta, Tb), (name, mem)
            for u, v in zip(a.correspondences(), b.correspondences()):
                assert np.array_equal(u, v), (name, mem)
            assert same(a.ExportMap(), b.ExportMap()), (name, mem)
            a.close(); b.close()
    # an empty blob: the host path answers
    fresh, b = make(monkeypatch), make(monkeypatch)
    empty = blob_of(fresh, "host")
    assert empty.size == HDR.itemsize
    b.ImportMap(blob)
    take_blob(b, empty, "device")
    assert (b.map_size(170), b.map_size(171), b.map_size(172), b.map_size(), b.map_size(102)) == (0, 1, 1, 0, 0)
    fresh.close(); b.close(); e.close()


def test_a_voxel_list_that_spans_several_sort_tiles(monkeypatch):
    """the 300k cloud: tens of thousands of voxels, many 1,024-key tiles of the radix sort and many blocks of every scan (the only case above 20k)"""
    e, a, b = make(monkeypatch), make(monkeypatch, OFF), make(monkeypatch)
    e.AddCloudToLocalMap([cloud300k()])
    assert e.map_size(102) > 8 * 1024
    blob = blob_of(e, "device")
    a.ImportMap(blob)
    take_blob(b, blob, "device")
    assert b.map_size(170) == 1 and b.map_size(147) == 0 and (b.map_size(), b.map_size(102)) == (300000, e.map_size(102))
    assert same(blob_of(b, "device"), blob) and b.map_size(147) == 0
    ea = a.ExportMap()
    assert same(ea, blob) and same(b.ExportMap(), ea) and same(e.ExportMap(), ea)
    cfg = cfg20k()
    Ta, Tb = np.eye(4), np.eye(4)
    oka = a.Match(reg.PointcloudCluster(planar_cloud_=cfg["scan"]), Ta, update_map=True)
    okb = b.Match(reg.PointcloudCluster(planar_cloud_=cfg["scan"]), Tb, update_map=True)
    assert oka == okb and np.array_equal(Ta, Tb)
    for u, v in zip(a.correspondences(), b.correspondences()):
        assert np.array_equal(u, v)
    assert same(a.ExportMap(), b.ExportMap())
    for m in (e, a, b):
        m.close()
