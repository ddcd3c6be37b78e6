"""The flat image of the kd-tree kinds' local maps (include/fls_map_kd.h): fls_map_export / fls_map_import, fls_map_image_export / _import,
replica sets, the fused batch over a replica set and the two-rank broadcast for IcpOptimized, LoamPointToPlaneKdtree and LoamFull handles.
Every comparison is bit for bit.

Deque states are driven with AddCloudToLocalMap of hand-made clouds wherever no Match is needed, with local_map_size = 3 (LoamFull:
local_planar_size = local_corner_size = 6, see KINDS) so that the deque trims early; the resume tests replay tests/replay.py's trajectories with the replay's own parameters."""
import ctypes as C
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg, synth
from tests import replay, util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOST = {"FLS_DEVICE_VOXELGRID": "0"}
GATE = dict(keyframe_delta_distance=1.0, keyframe_delta_rotation=0.2)
KINDS = {
    "icp": ("IcpOptimized", dict(reg.YAML_NCLT_ICP, local_map_size=3)),
    "kd": ("PointToPlane_KdTree", dict(reg.YAML_NCLT_LOC_KDTREE, local_map_size=3, **GATE)),
    # LoamFull filters its maps only once a deque holds more than 5 clouds (loam_full_kdtree.h:92-100): with deques of 3 no map filter would
    # ever run, on either path, and nothing could tell the paths apart (slots 115 / 116); its deques hold 6 here
    "loam": ("LoamFull_KdTree", dict(reg.YAML_NCLT_LOAM_FULL, local_corner_map_size=6, local_planar_map_size=6)),
}
KEEP = {"icp": 3, "kd": 3, "loam": 6}
KIND_ID = {"icp": _lib.ICP_OPTIMIZED, "kd": _lib.P2PLANE_KDTREE, "loam": _lib.LOAM_FULL}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"


@functools.lru_cache(maxsize=None)
def hip():
    h = C.CDLL("libamdhip64.so")  # the runtime libfls_reg.so itself is linked against
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


class DevMem:
    """n bytes of device memory, `skew` bytes into an allocation (skew 4: a buffer the image kernels cannot use directly)"""

    def __init__(self, n, fill=None, skew=0):
        self.n, self.base = n, C.c_void_p()
        assert hip().hipMalloc(C.byref(self.base), n + 32) == 0
        self.p = self.base.value + skew
        if fill is not None:
            assert hip().hipMemcpy(self.p, fill.ctypes.data, n, 1) == 0  # hipMemcpyHostToDevice

    def host(self):
        out = np.zeros(self.n, np.uint8)
        assert hip().hipMemcpy(out.ctypes.data, self.p, self.n, 2) == 0  # hipMemcpyDeviceToHost
        return out

    def free(self):
        hip().hipFree(self.base)


def make(monkeypatch, kind, env=None, loc=False, y=None):
    """the switches are read when the handle is created"""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    mode, y0 = KINDS[kind]
    m = reg.make_matcher(mode, y0 if y is None else y, is_localization_mode=loc)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return m


def cloud(n, seed):
    """n points of a flat 24 x 24 m patch, xyz + intensity; a few negative zeros among the coordinates and NaNs with payloads among the
    intensities (a VoxelGrid averages the intensity and nothing reads the average: the rows must carry the bits all the same)"""
    rng = np.random.default_rng(seed)
    c = np.empty((n, 4), np.float32)
    c[:, :2] = rng.uniform(-12.0, 12.0, (n, 2))
    c[:, 2] = rng.uniform(-1.5, 2.5, n)
    c[:, 3] = rng.uniform(0.0, 255.0, n)
    c[::97, 1] = np.float32(-0.0)
    bits = c.view(np.uint32)
    bits[5::131, 3] = 0x7FC00000 | (np.arange(len(bits[5::131])) + 1)
    bits[7::173, 3] = 0xFF800001 + np.arange(len(bits[7::173]))
    return c


def add(m, kind, planar, corner=None):
    m.AddCloudToLocalMap([planar, corner] if kind == "loam" else [planar])


# the deque drops the first two clouds: the ring's head is 1001 + 777 = 1778 points in, 2 past a multiple of 4
SIZES = {"icp": (1001, 777, 64, 1, 2050), "kd": (1001, 777, 64, 1, 2050), "loam": (1001, 777, 64, 1, 2050, 333, 17, 250)}
CORNER_SIZES = (301, 54, 0, 5, 130, 40, 9, 77)  # (LoamFull) an empty cloud inside the deque; head 355, 3 past a multiple of 4


def feed(m, kind, sizes=None, corner_sizes=CORNER_SIZES, seed=100):
    sizes = SIZES[kind] if sizes is None else sizes
    fed = []
    for k, n in enumerate(sizes):
        p, c = cloud(n, seed + k), cloud(corner_sizes[k], seed + 50 + k) if kind == "loam" else None
        add(m, kind, p, c)
        fed.append((p, c))
    return fed


def parse(blob):
    h = _lib.KdImageHeader.from_buffer_copy(blob[:224].tobytes())
    nm = int(h.n_maps)
    L = _lib.kd_image_layout(list(h.n_clouds)[:nm], list(h.n_points)[:nm])
    raw = blob.tobytes()
    sizes = [np.frombuffer(raw, np.uint32, int(h.n_clouds[m]), L["sizes"][m]).copy() for m in range(nm)]
    rows = [np.frombuffer(raw, np.uint32, 4 * int(h.n_points[m]), L["rows"][m]).reshape(-1, 4).copy() for m in range(nm)]
    return h, L, sizes, rows


def export_all_ways(m):
    """ExportMap, ExportMapImage to the host, to a device buffer and to a device buffer off the 16-byte grid: one image"""
    blob = m.ExportMap()
    n = m.MapImageBytes()
    assert blob.size == n
    host = np.full(n, 0xAB, np.uint8)
    m.ExportMapImage(host.ctypes.data, n, False)
    assert np.array_equal(blob, host)
    for skew in (0, 4):
        dev = DevMem(n, np.full(n, 0xCD, np.uint8), skew)
        m.ExportMapImage(dev.p, n, True)
        back = dev.host()
        dev.free()
        assert np.array_equal(blob, back), skew
    return blob


EXPORTS_PER_CALL = 4  # of export_all_ways


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1, 4)


@pytest.mark.parametrize("kind", ["icp", "kd", "loam"])
def test_one_image_three_calls_two_paths(kind, monkeypatch):
    dev, host = make(monkeypatch, kind), make(monkeypatch, kind, HOST)
    fed = feed(dev, kind)
    feed(host, kind)
    img = export_all_ways(dev)
    img_h = export_all_ways(host)
    assert np.array_equal(img, img_h), "the image depends on where the deque is kept"
    # which path ran
    assert dev.map_size(115) > 0 and (dev.map_size(160), dev.map_size(161)) == (EXPORTS_PER_CALL, 0)
    assert host.map_size(115) == 0 and host.map_size(116) > 0 and (host.map_size(160), host.map_size(161)) == (0, EXPORTS_PER_CALL)
    h, L, sizes, rows = parse(img)
    mode, y = KINDS[kind]
    assert (h.magic, h.revision, h.kind, h.total_bytes, h.is_localization_mode, h.gate_init, h.reserved) == (b"FLSKDM01", 1, KIND_ID[kind], img.size, 0, 0, 0)
    assert not any(h.gate_last_T)
    f32 = lambda v: int(np.float32(v).view(np.uint32))
    f64 = lambda v: int(np.float64(v).view(np.uint64))
    if kind == "loam":
        assert h.n_maps == 2 and list(h.local_size) == [6, 6] and h.point_search_thres_bits == f64(y["point_search_thres"])
        assert list(h.filter_size_bits) == [f32(y["local_planar_voxel_filter_size"]), f32(y["local_corner_voxel_filter_size"])]
    else:
        assert h.n_maps == 1 and list(h.local_size) == [3, 0] and list(h.filter_size_bits) == [f32(y["local_map_cloud_filter_size"]), 0]
        assert h.point_search_thres_bits == (f64(y["point_search_thres"]) if kind == "icp" else 0)
    keep = KEEP[kind]
    assert len(SIZES[kind]) == keep + 2
    assert list(sizes[0]) == list(SIZES[kind][-keep:]) and np.array_equal(rows[0], np.concatenate([bits(p) for p, _ in fed[-keep:]]))
    if kind == "loam":
        assert list(sizes[1]) == list(CORNER_SIZES[-keep:]) and np.array_equal(rows[1], np.concatenate([bits(c) for _, c in fed[-keep:]]))
    nan_rows = np.isnan(rows[0][:, 3].view(np.float32))
    assert nan_rows.sum() >= 10 and np.signbit(rows[0][:, 1].view(np.float32)[rows[0][:, 1] == 0x80000000]).all() and (rows[0][:, 1] == 0x80000000).sum() >= 10
    covered = np.zeros(img.size, bool)
    covered[:224] = True
    for m in range(h.n_maps):
        covered[L["sizes"][m]:L["sizes"][m] + 4 * len(sizes[m])] = True
        covered[L["rows"][m]:L["rows"][m] + 16 * len(rows[m])] = True
    assert not img[~covered].any()  # padding
    # both handles take the image, from host bytes and from a device buffer (one of them off the 16-byte grid), and write it again
    for k, m in enumerate((dev, host)):
        buf = DevMem(img.size, img, skew=4 * k)
        m.ImportMapImage(buf.p, img.size, True)
        buf.free()
        m.ImportMap(img)
        assert np.array_equal(m.ExportMap(), img)
    assert (dev.map_size(162), dev.map_size(163), host.map_size(162), host.map_size(163)) == (2, 0, 0, 2)
    dev.close(); host.close()


def test_ring_geometry(monkeypatch):
    """DeviceCloudRing::make_room (csrc/kd_map.hpp): a ring starts at 65,536 floats per plane and appends at its tail.  With
    local_map_size = 1 and clouds of 30,001 points: the first two lie at 0 and 30,001 (tail 60,002 <= 65,536) and the first is popped (head
    30,001); the third does not fit behind the tail (90,003 > 65,536) but fits the ring (30,001 live + 30,001 <= 65,536) and the live
    cloud's 30,001 floats do not overlap their destination (head >= live): the ring is re-packed IN PLACE, and after the pop its head is
    30,001 again, one past a multiple of 4.  A fourth cloud of 40,000 points fits no more (30,001 + 40,000 > 65,536): the ring GROWS to
    131,072.  Every export equals the host-path handle's, whose deque never lived in a ring."""
    y = dict(KINDS["icp"][1], local_map_size=1)
    dev, host = make(monkeypatch, "icp", y=y), make(monkeypatch, "icp", HOST, y=y)
    for k, n in enumerate((30001, 30001, 30001, 40000, 3)):
        c = cloud(n, 300 + k)
        add(dev, "icp", c); add(host, "icp", c)
        img = export_all_ways(dev)
        assert np.array_equal(img, host.ExportMap()), k
        h, _, sizes, rows = parse(img)
        assert list(sizes[0]) == [n] and np.array_equal(rows[0], bits(c)), k
    assert dev.map_size(161) == 0 and dev.map_size(115) == 5
    dev.close(); host.close()


def drive(m, mode, frames, Tprev, update=True):
    """Match from the predicted pose, per frame: everything the call returned and left; the last pose"""
    slots = (0, 1) if mode == "LoamFull_KdTree" else (0,)
    out = []
    for f in frames:
        T = Tprev @ f["guess_step"]
        ok = m.Match(util.cluster_for(mode, f["scan"], f["corner"]), T, update_map=update)
        st = m.stats
        out.append(((ok, T.tobytes(), st.iterations, st.n_valid, st.n_valid_corner, st.map_updated, tuple(m.map_size(s) for s in slots)),
                    [a.tobytes() for s in slots for a in m.correspondences(s)]))
        Tprev = T
    return out, Tprev


K_EXPORT = 4  # frames 0 .. 3 run before the image is taken


@pytest.mark.parametrize("name", ["icp", "loam", "p2plane_kd"])
def test_importer_equals_exporter_and_both_map_on(name, monkeypatch):
    """The replay's steps alternate long (1.25 m: alone past the 1.0 m keyframe gate) and short (0.25 m, 0.5 degrees: alone below both
    thresholds); frame k is short when k % 3 == 1.  Frames 0 - 2 run with update_map = True, frame 3 (long) with update_map = False, which
    leaves the gate alone: its last_T stays at frame 2's pose.  The image is taken there.  Frame 4 is short, but 1.5 m from last_T: the
    exporter takes a keyframe (map_updated == 1).  A handle whose gate was not restored would set last_T to frame 4's own pose and decide 0."""
    r = replay.make_replay(name)
    mode, y, frames = r["mode"], r["y"], r["frames"]
    step = frames[K_EXPORT]["guess_step"]
    rot = np.arccos(np.clip((np.trace(step[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))
    assert K_EXPORT % 3 == 1 and np.linalg.norm(step[:3, 3]) < y["keyframe_delta_distance"] and rot < y["keyframe_delta_rotation"]
    a = reg.make_matcher(mode, y)
    a.AddCloudToLocalMap(r["init_clouds"])
    before, T = drive(a, mode, frames[:K_EXPORT - 1], np.eye(4))
    last, T = drive(a, mode, frames[K_EXPORT - 1:K_EXPORT], T, update=False)
    print(name, "before the image: map_updated", [b[0][5] for b in before], "ok", [b[0][0] for b in before + last])
    assert before[-1][0][5] == 1, "frame 2 did not take a keyframe: the gate's last_T is not where the scenario needs it"
    img = export_all_ways(a)
    h0 = parse(img)[0]
    assert h0.gate_init == 1 and np.array_equal(np.array(h0.gate_last_T).reshape(4, 4).T, np.frombuffer(before[-1][0][1], np.float64).reshape(4, 4))
    b, c = reg.make_matcher(mode, y), reg.make_matcher(mode, y)
    b.ImportMap(img)
    buf = DevMem(img.size, img)
    c.ImportMapImage(buf.p, img.size, True)
    buf.free()
    assert (b.map_size(162), c.map_size(162)) == (1, 1)
    n_slots = 2 if mode == "LoamFull_KdTree" else 1
    assert [a.map_size(s) for s in range(n_slots)] == [b.map_size(s) for s in range(n_slots)] == [c.map_size(s) for s in range(n_slots)]
    Ts = [T, T, T]
    updates = []
    for k, f in enumerate(frames[K_EXPORT:]):
        res = []
        for i, m in enumerate((a, b, c)):
            r1, Ts[i] = drive(m, mode, [f], Ts[i])
            res.append(r1)
        assert res[0] == res[1] == res[2], (name, K_EXPORT + k)
        updates.append(res[0][0][0][5])
    print(name, "after the image: map_updated", updates)
    assert updates[0] == 1, "the first frame after the image took no keyframe: the scenario does not tell a restored gate from a fresh one"
    fin = a.ExportMap()
    assert np.array_equal(fin, b.ExportMap()) and np.array_equal(fin, c.ExportMap())
    if name == "loam":  # the VoxelGrid of a LoamFull map starts when a deque holds more than 5 clouds: after the import here
        assert max(h0.n_clouds) <= 5 < min(parse(fin)[0].n_clouds[:2])
    for m in (a, b, c):
        m.close()


@pytest.mark.parametrize("kind", ["icp", "kd"])
def test_localization_handles(kind, monkeypatch):
    cfg = synth.make_config(0 if kind == "icp" else 1, scale=0.1 if kind == "icp" else 0.05)
    a, b = make(monkeypatch, kind, loc=True), make(monkeypatch, kind, loc=True)
    add(a, kind, cloud(500, 1)); add(a, kind, cfg["map"])
    img = export_all_ways(a)
    h, _, sizes, rows = parse(img)
    assert h.is_localization_mode == 1 and list(sizes[0]) == [len(cfg["map"])] and np.array_equal(rows[0][:, :3], bits(np.c_[cfg["map"][:, :3], np.zeros(len(cfg["map"]))])[:, :3])
    add(b, kind, cloud(700, 2))
    b.ImportMap(img)
    assert b.map_size() == a.map_size()
    mode = KINDS[kind][0]
    cl = util.cluster_for(mode, cfg["scan"])
    Ta, Tb = cfg["T_init"].copy(), cfg["T_init"].copy()
    oka = a.Match(cl, Ta, update_map=False)
    assert a.stats.n_valid > 0
    fa = a.GetFitnessScore(2.0)
    with pytest.raises(_lib.FlsError) as e:
        b.GetFitnessScore(2.0)  # the final pose of a Match is not in the image
    assert e.value.status == _lib.FLS_ERR_STATE
    assert b.Match(cl, Tb, update_map=False) == oka and np.array_equal(Ta, Tb) and (a.stats.iterations, a.stats.n_valid) == (b.stats.iterations, b.stats.n_valid)
    assert b.GetFitnessScore(2.0) == fa
    # an import clears the final pose of the importer's own last Match as well
    b.ImportMap(img)
    with pytest.raises(_lib.FlsError):
        b.GetFitnessScore(2.0)
    # a mapping handle's image is refused
    m = make(monkeypatch, kind)
    add(m, kind, cfg["map"])
    with pytest.raises(_lib.FlsError) as e:
        b.ImportMap(m.ExportMap())
    assert e.value.status == _lib.FLS_ERR_INVALID
    a.close(); b.close(); m.close()


@pytest.mark.parametrize("kind", ["icp", "kd", "loam"])
def test_edge_images(kind, monkeypatch):
    mode = KINDS[kind][0]
    empty = np.zeros((0, 4), np.float32)
    never = make(monkeypatch, kind)
    img0 = export_all_ways(never)
    h = parse(img0)[0]
    assert img0.size == 224 and list(h.n_clouds) == [0, 0] and list(h.n_points) == [0, 0] and h.gate_init == 0
    # the header-only image resets a fed handle
    fed = make(monkeypatch, kind)
    feed(fed, kind)
    assert fed.map_size(0) > 0
    fed.ImportMap(img0)
    assert fed.map_size(0) == 0 and np.array_equal(fed.ExportMap(), img0)
    scan = cloud(400, 9)
    with pytest.raises(_lib.FlsError) as e:
        fed.Match(util.cluster_for(mode, scan, cloud(100, 10)), np.eye(4), update_map=False)
    assert e.value.status == _lib.FLS_ERR_STATE
    with pytest.raises(_lib.FlsError):
        fed.Replicas([0])
    # ... and it goes on like a handle that was never fed
    for m in (fed, never):
        feed(m, kind, seed=500)
    assert np.array_equal(fed.ExportMap(), never.ExportMap()) and fed.map_size(0) == never.map_size(0)
    # a deque holding one empty cloud; a 1-point cloud behind it; both taken by a second handle that then goes on like the first
    a, b = make(monkeypatch, kind), make(monkeypatch, kind)
    add(a, kind, empty, empty)
    img1 = export_all_ways(a)
    h1, _, sizes1, _ = parse(img1)
    assert h1.n_clouds[0] == 1 and h1.n_points[0] == 0 and list(sizes1[0]) == [0] and img1.size == 224 + 16 * h1.n_maps
    b.ImportMap(img1)
    assert np.array_equal(export_all_ways(b), img1)
    one = cloud(1, 77)
    add(a, kind, one, empty); add(b, kind, one, empty)
    img2 = export_all_ways(a)
    assert list(parse(img2)[2][0]) == [0, 1] and np.array_equal(parse(img2)[3][0], bits(one)) and np.array_equal(export_all_ways(b), img2)
    c = make(monkeypatch, kind)
    buf = DevMem(img2.size, img2)
    c.ImportMapImage(buf.p, img2.size, True)
    buf.free()
    for m in (a, b, c):
        feed(m, kind, seed=700)
    assert np.array_equal(a.ExportMap(), b.ExportMap()) and np.array_equal(a.ExportMap(), c.ExportMap())
    assert a.map_size(0) == b.map_size(0) == c.map_size(0) > 0
    for m in (never, fed, a, b, c):
        m.close()


def poke(good, offset, value):
    b = good.copy()
    raw = np.atleast_1d(value).view(np.uint8)
    b[offset:offset + raw.size] = raw
    return b


@pytest.mark.parametrize("env", [None, HOST], ids=["device importer", "host importer"])
def test_refusals_leave_the_handle_as_it_was(env, monkeypatch):
    H = _lib.KdImageHeader
    src = make(monkeypatch, "icp")
    feed(src, "icp", sizes=(40, 50, 61))  # three sizes: 4 bytes of padding in front of the rows
    good = src.ExportMap()
    h, L, sizes, _ = parse(good)
    assert L["rows"][0] - (L["sizes"][0] + 12) == 4
    bad = {
        "truncated by 16 bytes": good[:-16].copy(),
        "truncated, total_bytes adjusted": poke(good, H.total_bytes.offset, np.uint64(good.size - 16))[:-16].copy(),
        "flipped magic": poke(good, 2, np.uint8(good[2] ^ 0x40)),
        "revision 2": poke(good, H.revision.offset, np.uint32(2)),
        "kind rewritten": poke(good, H.kind.offset, np.uint32(_lib.P2PLANE_KDTREE)),
        "two maps": poke(good, H.n_maps.offset, np.uint32(2)),
        "sizes sum to one more than n_points": poke(good, L["sizes"][0] + 4, np.uint32(51)),
        "n_points one less": poke(good, H.n_points.offset, np.uint64(150)),
        "four clouds in a deque of three": poke(good, H.n_clouds.offset, np.uint64(4)),
        "2^62 points": poke(good, H.n_points.offset, np.uint64(1 << 62)),
        "padding byte set": poke(good, L["sizes"][0] + 12, np.uint8(1)),
        "last padding byte set": poke(good, L["rows"][0] - 1, np.uint8(0x80)),
        "reserved word set": poke(good, H.reserved.offset, np.uint32(1)),
        "gate init = 2": poke(good, H.gate_init.offset, np.uint32(2)),
        "last_T set while init is 0": poke(good, H.gate_last_T.offset + 8 * 5, np.float64(1.0)),
        "gate init = 1 with a NaN in last_T": poke(poke(good, H.gate_init.offset, np.uint32(1)), H.gate_last_T.offset + 8 * 12, np.float64(np.nan)),
        "mapping image marked localization": poke(good, H.is_localization_mode.offset, np.uint32(1)),
    }
    assert all(not np.array_equal(b, good) for b in bad.values())
    # images that are fine, for another handle
    for name, kind, kw in (("a P2PlaneKd image", "kd", {}), ("a LoamFull image", "loam", {}),
                           ("another map_cloud_filter_size", "icp", dict(y=dict(KINDS["icp"][1], local_map_cloud_filter_size=0.5))),
                           ("another local_map_size", "icp", dict(y=dict(KINDS["icp"][1], local_map_size=4))),
                           ("another point_search_thres", "icp", dict(y=dict(KINDS["icp"][1], point_search_thres=1.5))),
                           ("a localization handle's image", "icp", dict(loc=True))):
        o = make(monkeypatch, kind, **kw)
        feed(o, kind, sizes=(40,), corner_sizes=(9,))
        bad[name] = o.ExportMap()
        o.close()
    iv = reg.make_matcher("PointToPlane_IVOX", reg.YAML_NCLT_IVOX)
    iv.AddCloudToLocalMap([cloud(2000, 3)])
    bad["an iVox blob"] = iv.ExportMap()
    nd = reg.make_matcher("IncrementalNDT", reg.YAML_NCLT_NDT)
    nd.AddCloudToLocalMap([cloud(2000, 3)])
    bad["an NDT blob"] = nd.ExportMap()

    m = make(monkeypatch, "icp", env)
    feed(m, "icp")
    before = m.ExportMap()
    size_before = m.map_size(0)
    imports = (m.map_size(162), m.map_size(163))
    for k, (name, b) in enumerate(bad.items()):
        with pytest.raises(_lib.FlsError) as e:
            if k % 2:
                buf = DevMem(b.size, b, skew=4 * (k % 4 == 1))
                try:
                    m.ImportMapImage(buf.p, b.size, True)
                finally:
                    buf.free()
            else:
                m.ImportMap(b)
        assert e.value.status == _lib.FLS_ERR_INVALID, name
        assert np.array_equal(m.ExportMap(), before) and m.map_size(0) == size_before, name
    assert (m.map_size(162), m.map_size(163)) == imports
    # the other kinds do not take an ICP image either
    for other in (iv, nd):
        with pytest.raises(_lib.FlsError):
            other.ImportMap(good)
        other.close()
    # still an ordinary handle: it goes on like a twin that never saw a bad image
    twin = make(monkeypatch, "icp", env)
    feed(twin, "icp")
    for x in (m, twin):
        feed(x, "icp", seed=900)
    assert np.array_equal(m.ExportMap(), twin.ExportMap()) and m.map_size(0) == twin.map_size(0)
    # the good image passes
    m.ImportMap(good)
    assert np.array_equal(m.ExportMap(), good)
    src.close(); m.close(); twin.close()


def rows_of(oks, Ts, stats):
    return [(bool(oks[j]), Ts[j].tobytes(), stats[j].iterations, stats[j].n_valid, stats[j].sum_res) for j in range(len(oks))]


@functools.lru_cache(maxsize=None)
def batch_world():
    """the 5 % cut of configs[0]: the map and 6 jobs"""
    cfg0 = synth.make_config(0, job=0, scale=0.05)
    scans = (cfg0["scan"],) + tuple(synth.make_config(0, job=j, scale=0.05, with_map=False)["scan"] for j in range(1, 6))
    return cfg0["map"], scans


@pytest.mark.parametrize("via_blob", [False, True], ids=["device to device", "via blob"])
def test_replica_set_tables_equal_the_owners(via_blob, monkeypatch):
    if via_blob:
        monkeypatch.setenv("FLS_REPLICAS_VIA_BLOB", "1")
    world_map, scans = batch_world()
    m = make(monkeypatch, "icp")
    with pytest.raises(_lib.FlsError) as e:
        m.Replicas([0])  # no map: nothing a replica could match against
    assert e.value.status == _lib.FLS_ERR_STATE
    m.AddCloudToLocalMap([world_map])
    clusters = [util.cluster_for("IcpOptimized", s) for s in scans]
    T0 = [np.eye(4)] * len(scans)
    serial = rows_of(*m.MatchBatch(clusters, T0, lanes=2))
    fused = rows_of(*m.MatchBatchFused(clusters, T0, slots=3))
    assert all(r[3] > 0 for r in serial) and all(r[3] > 0 for r in fused), "a job found no correspondence: the table shows nothing"
    print("ok", [r[0] for r in serial], "iterations", [r[2] for r in serial], "n_valid", [r[3] for r in serial])
    rs = m.Replicas([0, 0])
    ms = rs.import_ms()
    assert len(ms) == 2 and ms[0] == 0.0 and ms[1] > 0.0
    assert rows_of(*rs.MatchBatch(clusters, T0, lanes=2)) == serial
    assert rows_of(*rs.MatchBatchFused(clusters, T0, slots=3)) == fused
    exports = m.map_size(160) + m.map_size(161)
    assert exports == 1
    # the owner takes a keyframe, the set follows after a refresh
    m.AddCloudToLocalMap([cloud(3000, 41)])
    serial2 = rows_of(*m.MatchBatch(clusters, T0, lanes=2))
    fused2 = rows_of(*m.MatchBatchFused(clusters, T0, slots=3))
    assert serial2 != serial
    half = len(scans) // 2  # the block partition: the first half runs on the owner itself, the second on the replica, which still holds the old map
    stale = rows_of(*rs.MatchBatchFused(clusters, T0, slots=3))
    assert stale[:half] == fused2[:half] and stale[half:] == fused[half:] and fused2[half:] != fused[half:]
    rs.Refresh()
    assert m.map_size(160) + m.map_size(161) == exports + 1
    assert rows_of(*rs.MatchBatch(clusters, T0, lanes=2)) == serial2
    assert rows_of(*rs.MatchBatchFused(clusters, T0, slots=3)) == fused2
    rs.close(); m.close()


WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["FLS_ROOT"])
import numpy as np
import torch.distributed as dist
from funny_lidar_slam_amd import batch, registration as reg, synth

dist.init_process_group(backend="gloo")
rank, world = dist.get_rank(), dist.get_world_size()
n_jobs, scale = 6, 0.05
m = reg.make_matcher("IcpOptimized", dict(reg.YAML_NCLT_ICP, local_map_size=3), device_id=0)   # both ranks share the one GPU
if rank == 0:
    m.AddCloudToLocalMap([synth.make_config(0, job=0, scale=scale)["map"]])
if os.environ["FLS_TEST_FORM"] == "blob":
    blob = batch.broadcast_blob(m.ExportMap() if rank == 0 else None, src=0)
    if rank != 0:
        m.ImportMap(blob)
else:
    batch.broadcast_map_image(m, src=0, device=None)   # gloo: the image goes through pinned host memory
b, e = batch.partition(n_jobs, world, rank)
scans = [synth.make_config(0, job=j, scale=scale, with_map=False)["scan"] for j in range(n_jobs)]
mk = lambda s: reg.PointcloudCluster(ordered_cloud_=s)
oks, Tb, sb = m.MatchBatchFused([mk(scans[j]) for j in range(b, e)], [np.eye(4)] * (e - b), slots=3)
rows = np.stack([batch.pack_result(Tb[k], oks[k], sb[k].iterations, sb[k].n_valid, sb[k].sum_res) for k in range(e - b)])
table = batch.gather_results(rows, n_jobs, batch.RESULT_WIDTH)
if rank == 0:
    oks, Ts, ss = m.MatchBatchFused([mk(s) for s in scans], [np.eye(4)] * n_jobs, slots=3)   # all jobs on the exporter's own handle
    serial = np.stack([batch.pack_result(Ts[k], oks[k], ss[k].iterations, ss[k].n_valid, ss[k].sum_res) for k in range(n_jobs)])
    np.savez(os.environ["FLS_OUT"], table=table, serial=serial, imports=np.array([m.map_size(162) + m.map_size(163)]))
else:
    assert m.map_size(162) + m.map_size(163) == 1 and m.map_size() > 0
m.close()
dist.barrier()
dist.destroy_process_group()
'''


@pytest.mark.parametrize("form", ["blob", "image"])
def test_two_gloo_ranks_on_one_device(form, tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    out = tmp_path / "table.npz"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(FLS_ROOT=ROOT, FLS_OUT=str(out), MASTER_ADDR="127.0.0.1", FLS_TEST_FORM=form)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)]
    run = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    z = np.load(out)
    assert z["table"].shape == (6, 20) and int(z["imports"][0]) == 0
    assert np.array_equal(z["table"], z["serial"]), "sharded over two ranks (imported ICP image) != all jobs on the exporter's handle"
    assert (z["table"][:, 18] > 0).all()  # every job found correspondences
