"""Keyframes of the kd-tree kinds (IcpOptimized, LoamFull, LoamPointToPlaneKdtree) pushed into the device deque on the device
(csrc/kernels_kd_push.hpp, DeviceCloudRing::push_back_device, KdLocalMap in csrc/kd_map.hpp) and the host deque that is filled
only when something reads it (csrc/kd_lazy_deque.hpp).  Handle A is created with FLS_KD_DEVICE_PUSH=0 (the push through the host: download,
host transform, upload), handle B with the default; both live in one process and get the same calls.  Every comparison is bit for bit.
fls_map_size slots: 164 clouds pushed on the device, 165 pushed through the host while a ring exists, 166 fetched to the host lazily,
167 device rebuilds declined after a device push (include/fls_reg.h)."""
import functools

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg, synth
from oracle import oracle as O
from tests import replay, util
from tests.test_gpu_kd_image import DevMem, parse

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
HOST_PUSH = {"FLS_KD_DEVICE_PUSH": "0"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"


def make(mode, y, env=None, loc=False):
    """the switch is read when the handle is created"""
    with pytest.MonkeyPatch.context() as mp:
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        return reg.make_matcher(mode, y, is_localization_mode=loc)


def with_intensity(cloud, seed, payloads=True):
    """xyz + an intensity column; among the intensities a few NaNs with payloads and a negative zero (the deque must carry the bits)"""
    if cloud is None:
        return None
    rng = np.random.default_rng(seed)
    c = np.empty((len(cloud), 4), F32)
    c[:, :3] = cloud[:, :3]
    c[:, 3] = rng.uniform(0.0, 255.0, len(cloud))
    if payloads and len(c):
        b = c.view(np.uint32)
        b[5::131, 3] = 0x7FC00000 | (np.arange(len(b[5::131])) + 1)
        b[7::173, 3] = 0xFF800001 + np.arange(len(b[7::173]))
        b[3::211, 3] = 0x80000000
    return c


def slots_of(mode):
    return (0, 1) if mode == "LoamFull_KdTree" else (0,)


def match(m, mode, f, Tprev, update=True):
    T = Tprev @ f["guess_step"]
    ok = m.Match(util.cluster_for(mode, f["scan"], f["corner"]), T, update_map=update)
    st = m.stats
    return dict(ok=ok, T=T, stats=(int(st.iterations), int(st.n_valid), int(st.n_valid_corner), int(st.map_updated)),
                sizes=tuple(m.map_size(s) for s in slots_of(mode)), corr=[a.copy() for s in slots_of(mode) for a in m.correspondences(s)])


def assert_same_match(a, b, where):
    assert a["ok"] == b["ok"] and a["stats"] == b["stats"] and a["sizes"] == b["sizes"], (where, a["ok"], b["ok"], a["stats"], b["stats"], a["sizes"], b["sizes"])
    assert np.array_equal(np.ascontiguousarray(a["T"]).view(np.uint64), np.ascontiguousarray(b["T"]).view(np.uint64)), (where, "pose bits")
    assert len(a["corr"]) == len(b["corr"])
    for u, v in zip(a["corr"], b["corr"]):
        assert np.array_equal(u, v), (where, "correspondences")


@functools.lru_cache(maxsize=None)
def scenario(name, n_frames=None):
    """a replay of tests/replay.py whose scans carry intensities (NaN payloads where no VoxelGrid averages them: not for ICP's source);
    built once per kind and left unchanged (a test that alters a frame copies it)"""
    r = replay.make_replay(name, n_frames=n_frames) if n_frames else replay.make_replay(name)
    for k, f in enumerate(r["frames"]):
        f["scan"] = with_intensity(f["scan"], 1000 + k, payloads=name != "icp")
        f["corner"] = with_intensity(f["corner"], 2000 + k)
    return r


N_FRAMES = {"icp": None, "loam": None, "p2plane_kd": None}  # the replays' own lengths: each gives at least three keyframes (asserted)
CLOUDS_PER_KEYFRAME = {"icp": 1, "loam": 2, "p2plane_kd": 1}


@functools.lru_cache(maxsize=None)
def paired_run(name):
    """A and B through one replay, once per kind: what every frame returned and left on both, and the images after every keyframe"""
    r = scenario(name, N_FRAMES[name])
    mode, y = r["mode"], r["y"]
    a, b = make(mode, y, HOST_PUSH), make(mode, y)
    for m in (a, b):
        m.AddCloudToLocalMap(r["init_clouds"])
    rec, Ta, Tb = [], np.eye(4), np.eye(4)
    for f in r["frames"]:
        ra, rb = match(a, mode, f, Ta), match(b, mode, f, Tb)
        Ta, Tb = ra["T"], rb["T"]
        key = ra["stats"][3] or rb["stats"][3]
        rec.append(dict(a=ra, b=rb, img_a=a.ExportMap() if key else None, img_b=b.ExportMap() if key else None))
    counters = dict(a=[a.map_size(s) for s in (164, 165, 166, 167)], b=[b.map_size(s) for s in (164, 165, 166, 167)])
    a.close(); b.close()
    return r, rec, counters


@pytest.mark.parametrize("name", ["icp", "loam", "p2plane_kd"])
def test_device_push_equals_host_push(name):
    r, rec, counters = paired_run(name)
    keyframes = 0
    for k, e in enumerate(rec):
        assert_same_match(e["a"], e["b"], (name, k))
        if e["img_a"] is not None:
            keyframes += 1
            assert np.array_equal(e["img_a"], e["img_b"]), (name, k, "the images differ after the keyframe")
    print(name, "map_updated", [e["a"]["stats"][3] for e in rec], "counters", counters)
    assert keyframes >= 3, (name, keyframes)
    per = CLOUDS_PER_KEYFRAME[name]
    assert counters["b"][0] == per * keyframes and counters["b"][2] == 0 and counters["b"][3] == 0, counters  # fails where no push runs on the device: slot 164 stays 0
    assert counters["b"][1] == per  # the first cloud(s), AddCloudToLocalMap from the host
    assert counters["a"][0] == 0 and counters["a"][1] == per * (keyframes + 1) and counters["a"][2] == 0, counters


def xform_f(cloud, T):
    """hm::xform_cloud_f restated: R, t cast to float, then (R0 x + (R3 y + R6 z)) + t0 in float32, one rounding per operation"""
    R, t = T[:3, :3].astype(F32), T[:3, 3].astype(F32)
    x, y, z = (np.ascontiguousarray(cloud[:, i], F32) for i in range(3))
    out = np.array(cloud, F32, copy=True)
    for i in range(3):
        out[:, i] = (R[i, 0] * x + (R[i, 1] * y + R[i, 2] * z)) + t[i]
    return out


def xform_d(cloud, T):
    """hm::xform_cloud_d restated: float(((T0 x + T4 y) + T8 z) + T12) in float64"""
    x, y, z = (cloud[:, i].astype(F64) for i in range(3))
    out = np.array(cloud, F32, copy=True)
    for i in range(3):
        out[:, i] = (((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3]).astype(F32)
    return out


def last_cloud(img, m=0):
    _, _, sizes, rows = parse(img)
    n = int(sizes[m][-1])
    return rows[m][len(rows[m]) - n:]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32).reshape(-1, 4)


@pytest.mark.parametrize("name", ["icp", "loam", "p2plane_kd"])
def test_pushed_rows_against_the_restated_transform(name):
    """the expected rows come from numpy (and the oracle's VoxelGrid for ICP's source filter), not from handle A"""
    r, rec, _ = paired_run(name)
    checked = 0
    for k, (f, e) in enumerate(zip(r["frames"], rec)):
        if not e["b"]["stats"][3]:
            continue
        T = e["b"]["T"]
        if name == "loam":
            assert np.array_equal(last_cloud(e["img_b"], 0), bits(xform_d(f["scan"], T))), (name, k, "planar")
            assert np.array_equal(last_cloud(e["img_b"], 1), bits(xform_d(f["corner"], T))), (name, k, "corner")
        else:
            src = O.voxel_grid(f["scan"], r["y"]["source_cloud_filter_size"]) if name == "icp" else f["scan"]
            assert 10 < len(src) <= len(f["scan"])
            assert np.array_equal(last_cloud(e["img_b"]), bits(xform_f(src, T))), (name, k)
        checked += 1
    assert checked >= 3


# ---- ring edges ----------------------------------------------------------------------------------------------------------------------------
def ring_model(pushes, keep):
    """DeviceCloudRing::make_room + pop_front restated (csrc/kd_map.hpp): `pushes` = [(points, pushed on the device)], a trim to
    `keep` clouds after every push.  Returns how often a DEVICE push re-packed the ring in place / moved it to new planes."""
    cap = head = tail = 0
    sizes, in_place, moved = [], 0, 0
    for n, on_device in pushes:
        if tail + n > cap:
            live, ncap = tail - head, cap
            while live + n > ncap or ncap < 65536:
                ncap = ncap * 2 if ncap else 65536
            if ncap == cap and head >= live:
                in_place += on_device
            else:
                cap = ncap * 2 if ncap == cap else ncap
                moved += on_device
            head, tail = 0, live
        tail += n
        sizes.append(n)
        if len(sizes) > keep:
            head += sizes.pop(0)
    return in_place, moved


def test_ring_edges():
    """LoamPointToPlaneKdtree with local_map_size = 2; the first cloud is a 50,000-point map, every frame but the first (which sets the
    keyframe gate's pose) a keyframe (1.25 m steps) of 9,001 / 9,002 / 9,003 points (no multiple of 4: the tail lands on every alignment).  The ring starts at 65,536 floats per plane:
    the second device push (50,000 + 9,002 live + 9,003) fits no more and MOVES the ring to 131,072; the tail then advances ~9,002 per
    keyframe while the head follows two clouds behind, and the tenth device push finds no room behind the tail and re-packs IN PLACE
    (18,00x live floats, head far beyond them).  ring_model derives both from the sizes actually pushed; the handle's state shows them
    through slot 0 and the exported images, which equal A's (whose pushes take the same two branches through the host) throughout.  The
    clouds the trim drops were never fetched: slot 166 stays 0."""
    scene = synth.make_scene()
    rng = synth.rng_for(5, 41)
    lid = dict(synth.VELODYNE_64, n_az=150)  # 9,600 rays
    y = dict(reg.YAML_NCLT_LOC_KDTREE, local_map_size=2, keyframe_delta_distance=1.0, keyframe_delta_rotation=0.2)
    mode = "PointToPlane_KdTree"
    init = synth.sample_map(scene, 50000, synth.rng_for(5, 41, 9), radius=45.0)
    a, b = make(mode, y, HOST_PUSH), make(mode, y)
    for m in (a, b):
        m.AddCloudToLocalMap([init])
    pushes, T_gt, Ta, Tb = [(len(init), 0)], np.eye(4), np.eye(4), np.eye(4)
    for k in range(13):
        step = np.eye(4)
        step[:3, :3] = synth.so3_exp(np.deg2rad([0.0, 0.0, 4.0]))
        step[:3, 3] = [1.25, 0.1 * (k % 2), 0.0]
        T_gt = T_gt @ step @ synth.random_pose(rng, 0.4, 0.06)
        scan = synth.cast_scan(scene, T_gt, rng=rng, max_range=40.0, **lid)
        scan = with_intensity(scan[rng.permutation(len(scan))[:9001 + k % 3]], 3000 + k)
        f = dict(scan=scan, corner=None, guess_step=step)
        ra, rb = match(a, mode, f, Ta), match(b, mode, f, Tb)
        Ta, Tb = ra["T"], rb["T"]
        assert_same_match(ra, rb, k)
        assert rb["stats"][3] == (k > 0), (k, "keyframe?", rb["ok"], rb["stats"])  # (the first Match sets the gate's pose and takes none)
        if k == 0:
            continue
        pushes.append((len(scan), 1))
        img = b.ExportMap()
        assert np.array_equal(img, a.ExportMap()), k
        _, _, sizes, _ = parse(img)
        assert list(sizes[0]) == [n for n, _ in pushes[-2:]], (k, list(sizes[0]))  # the two newest clouds
        assert np.array_equal(last_cloud(img), bits(xform_f(scan, Tb))), k
    in_place, moved = ring_model(pushes, 2)
    print("device pushes that re-packed in place / moved the ring:", in_place, moved)
    assert in_place >= 1 and moved >= 1, (in_place, moved)
    assert (b.map_size(164), b.map_size(165), b.map_size(166), b.map_size(167)) == (12, 1, 0, 0)
    assert (a.map_size(164), a.map_size(165), a.map_size(166)) == (0, 13, 0)
    a.close(); b.close()


def test_loam_keyframe_with_an_empty_corner_cloud():
    r = scenario("loam", None)
    mode, y = r["mode"], r["y"]
    a, b = make(mode, y, HOST_PUSH), make(mode, y)
    for m in (a, b):
        m.AddCloudToLocalMap(r["init_clouds"])
    Ta, Tb, keyframes = np.eye(4), np.eye(4), 0
    for k, f in enumerate(r["frames"][:4]):
        if k == 2:  # a long step: a keyframe
            f = dict(f, corner=np.zeros((0, 4), F32))
        ra, rb = match(a, mode, f, Ta), match(b, mode, f, Tb)
        Ta, Tb = ra["T"], rb["T"]
        assert_same_match(ra, rb, k)
        keyframes += rb["stats"][3]
        img = b.ExportMap()
        assert np.array_equal(img, a.ExportMap()), k
        if k == 2:
            assert rb["stats"][3] == 1 and rb["stats"][2] == 0
            _, _, sizes, _ = parse(img)
            assert int(sizes[1][-1]) == 0 and int(sizes[0][-1]) == len(f["scan"]) and len(sizes[0]) == len(sizes[1])  # the deque gained a cloud of size 0
            assert np.array_equal(last_cloud(img, 0), bits(xform_d(f["scan"], Tb)))
    assert b.map_size(166) == 0 and b.map_size(164) == 2 * keyframes and a.map_size(164) == 0  # (the empty cloud counts: two per keyframe)
    a.close(); b.close()


def test_attached_scan_pushes_its_fourth_plane():
    """LoamPointToPlaneKdtree fed by fls_scan_attach_preprocessed (tests/test_gpu_preprocess_handoff.py's mapping replay): the scan was
    written on the device with its intensity plane, which the device push uses as it is.  A (switch off) fetches the attached scan and
    pushes through the host, B pushes on the device, C gets the same rows from the host (fls_scan_upload_raw) and pushes on the device
    with the intensity plane sent up at push time: one image, after every frame."""
    from tests import deskew_util as du
    from tests.test_gpu_preprocess import STAMP
    from tests.test_gpu_preprocess_handoff import KD_MAPPING, make_pre, match_device, match_host, trajectory_scans
    mode = "PointToPlane_KdTree"
    cfg = synth.make_config(1, scale=0.1)
    pre = make_pre()
    a, b, c = make(mode, KD_MAPPING, HOST_PUSH), make(mode, KD_MAPPING), make(mode, KD_MAPPING)
    for m in (a, b, c):
        m.AddCloudToLocalMap([cfg["map"]])
    Ts, updates = [cfg["T_gt"].copy() for _ in range(3)], 0
    for k, raw in enumerate(trajectory_scans(cfg, 6, 300, 0.45, 0.004)):
        t, q = du.imu_for(yaw_rate=np.deg2rad(20.0 + k))
        assert pre.scan_device(raw, STAMP, t, q).status == _lib.FLS_OK
        res = [match_device(a, pre, "planar_filtered", Ts[0], True), match_device(b, pre, "planar_filtered", Ts[1], True),
               match_host(c, pre, "planar_filtered", Ts[2], True)]
        Ts = [r[1] for r in res]
        assert res[0][0] == res[1][0] == res[2][0] and Ts[0].tobytes() == Ts[1].tobytes() == Ts[2].tobytes(), k
        assert a.stats.map_updated == b.stats.map_updated == c.stats.map_updated
        updates += int(b.stats.map_updated)
        img = a.ExportMap()
        assert np.array_equal(img, b.ExportMap()) and np.array_equal(img, c.ExportMap()), k
        if b.stats.map_updated:
            rows = pre.get("planar_filtered")
            assert np.array_equal(last_cloud(img), bits(xform_f(rows, Ts[1]))), k
            assert len(np.unique(last_cloud(img)[:, 3])) > 10  # real intensities, not a plane of zeros
    assert updates >= 2 and (b.map_size(164), b.map_size(166)) == (updates, 0) and (c.map_size(164), c.map_size(166)) == (updates, 0)
    assert a.map_size(164) == 0
    for m in (a, b, c):
        m.close()


# ---- the host deque: not fetched on the default path, right when it is ---------------------------------------------------------------------
def export_three_ways(m):
    """ExportMap, ExportMapImage to host memory and to device memory: one image, three exports"""
    blob = m.ExportMap()
    n = m.MapImageBytes()
    host = np.full(n, 0xAB, np.uint8)
    m.ExportMapImage(host.ctypes.data, n, False)
    dev = DevMem(n, np.full(n, 0xCD, np.uint8))
    m.ExportMapImage(dev.p, n, True)
    back = dev.host()
    dev.free()
    assert np.array_equal(blob, host) and np.array_equal(blob, back)
    return blob


class DequeMirror:
    """which clouds of B's deque have a host copy (csrc/kd_lazy_deque.hpp restated for a single deque)"""

    def __init__(self, keep):
        self.keep, self.have = keep, []

    def push(self, on_host):
        self.have.append(on_host)
        if len(self.have) > self.keep:
            self.have.pop(0)

    def fetch(self):
        missing = self.have.count(False)
        self.have = [True] * len(self.have)
        return missing


def test_host_deque_is_lazy_and_right_when_fetched():
    """IcpOptimized, the icp replay (local_map_size = 3; frames k % 3 == 1 are short and take no keyframe, frame 6 does not converge).
    Frames 0 - 3: two device pushes (the first Match sets the gate's pose, frame 1 is short); every kind of export leaves slot 166 at 0.  Then one AddCloudToLocalMap from the host, frames
    4 - 7, and frame 8 (a keyframe) carries one point 560 / 430 / 300 m out: the source VoxelGrid (leaf 0.4) and the map VoxelGrid still fit
    their 2^31 leaves, so the scan is filtered and pushed on the device, but the search grid's window (1 m cells) would hold more than
    GridImage::kMaxWindowCells (48 Mi) cells and DeviceGridBuilder::run DECLINES -- a return value; the host path rebuilds from the host
    deque, which first fetches what the device pushes left in the ring alone.  A takes the same decline with a deque it always had."""
    r = scenario("icp")
    mode, y, frames = r["mode"], r["y"], r["frames"]
    a, b = make(mode, y, HOST_PUSH), make(mode, y)
    for m in (a, b):
        m.AddCloudToLocalMap(r["init_clouds"])
    mirror = DequeMirror(y["local_map_size"])
    mirror.push(True)
    Ta, Tb = np.eye(4), np.eye(4)

    def run(ks, far=None):
        nonlocal Ta, Tb
        out = []
        for k in ks:
            f = frames[k]
            if k == far:
                scan = f["scan"].copy()
                scan[17, :3] = [560.0, 430.0, 300.0]
                f = dict(f, scan=scan)
            ra, rb = match(a, mode, f, Ta), match(b, mode, f, Tb)
            Ta, Tb = ra["T"], rb["T"]
            assert_same_match(ra, rb, k)
            assert np.array_equal(a.ExportMap(), b.ExportMap()), k
            if rb["stats"][3]:
                mirror.push(False)
            out.append(rb)
        return out

    first = run(range(4))
    assert sum(e["stats"][3] for e in first) == 2 and b.map_size(164) == 2 and b.map_size(166) == 0
    packed = b.map_size(160)
    export_three_ways(b)
    assert b.map_size(166) == 0 and b.map_size(160) == packed + 3 and b.map_size(161) == 0
    # one cloud from the host, then on
    extra = with_intensity(r["init_clouds"][0], 77)
    for m in (a, b):
        m.AddCloudToLocalMap([extra])
    mirror.push(True)
    assert np.array_equal(a.ExportMap(), b.ExportMap()) and a.map_size(0) == b.map_size(0)
    run(range(4, 8))
    assert b.map_size(166) == 0 and b.map_size(167) == 0 and b.map_size(165) == 2
    # the decline
    builds_a, host_filters_a = a.map_size(114), a.map_size(116)
    dec = run([8], far=8)[0]
    assert dec["stats"][3] == 1, "frame 8 took no keyframe: the scenario needs one there"
    assert a.map_size(116) == host_filters_a + 1 and a.map_size(114) == builds_a, "handle A's device rebuild was not declined"
    missing = mirror.fetch()
    assert missing >= 2
    assert b.map_size(167) == 1 and b.map_size(166) == missing, (b.map_size(167), b.map_size(166), missing)
    assert a.map_size(167) == 0 and a.map_size(166) == 0
    # the next two Matches (frame 9 takes a keyframe while the far point is still in the deque: pushed on the device, declined, one cloud fetched)
    after = run([9, 10])
    print("after the decline: ok", [e["ok"] for e in after], "map_updated", [e["stats"][3] for e in after], "slots 164-167", [b.map_size(s) for s in (164, 165, 166, 167)])
    assert b.map_size(166) == missing + mirror.fetch() and b.map_size(167) == 1 + sum(e["stats"][3] for e in after)
    a.close(); b.close()


# ---- hand-off to the other consumers -------------------------------------------------------------------------------------------------------
def test_import_and_replicas_after_device_pushes():
    r = scenario("icp")
    mode, y, frames = r["mode"], r["y"], r["frames"]
    a, b = make(mode, y, HOST_PUSH), make(mode, y)
    for m in (a, b):
        m.AddCloudToLocalMap(r["init_clouds"])
    Ta, Tb = np.eye(4), np.eye(4)
    for k in range(4):
        ra, rb = match(a, mode, frames[k], Ta), match(b, mode, frames[k], Tb)
        Ta, Tb = ra["T"], rb["T"]
    assert b.map_size(164) == 2 and a.map_size(164) == 0
    # what leaves 164 alone: update_map = False, a batch lane, a localization-mode handle
    pushed = b.map_size(164)
    probe = match(b, mode, frames[5], Tb, update=False)
    assert probe["stats"][3] == 0 and b.map_size(164) == pushed
    clusters = [util.cluster_for(mode, frames[k]["scan"]) for k in (4, 5)]
    guesses = [Tb @ frames[4]["guess_step"], Tb @ frames[4]["guess_step"] @ frames[5]["guess_step"]]
    lanes_b = b.MatchBatch(clusters, guesses, lanes=2)
    assert b.map_size(164) == pushed
    loc = make(mode, y, loc=True)
    loc.AddCloudToLocalMap(r["init_clouds"])
    T = np.eye(4) @ frames[0]["guess_step"]
    loc.Match(util.cluster_for(mode, frames[0]["scan"]), T, update_map=True)
    assert loc.map_size(164) == 0 and loc.stats.map_updated == 0
    loc.close()
    # B's image into a fresh handle and into a replica set
    img = b.ExportMap()
    assert np.array_equal(img, a.ExportMap())
    c = make(mode, y)
    c.ImportMap(img)
    rs = b.Replicas([0, 0])
    lanes_a = a.MatchBatch(clusters, guesses, lanes=2)
    lanes_rs = rs.MatchBatch(clusters, guesses, lanes=2)
    for got in (lanes_b, lanes_rs):
        assert got[0] == lanes_a[0] and np.array_equal(got[1].view(np.uint64), lanes_a[1].view(np.uint64))
        assert [(s.iterations, s.n_valid) for s in got[2]] == [(s.iterations, s.n_valid) for s in lanes_a[2]]
    rs.close()
    assert b.map_size(166) == 0  # neither export fetched a cloud
    Tc = Tb.copy()
    for k in (4, 5, 6, 7):  # (frame 6 does not converge; frame 7 takes a keyframe)
        ra, rb, rc = match(a, mode, frames[k], Ta), match(b, mode, frames[k], Tb), match(c, mode, frames[k], Tc)
        Ta, Tb, Tc = ra["T"], rb["T"], rc["T"]
        assert_same_match(ra, rb, k)
        assert_same_match(ra, rc, ("importer", k))
    fin = a.ExportMap()
    assert np.array_equal(fin, b.ExportMap()) and np.array_equal(fin, c.ExportMap())
    assert c.map_size(164) >= 1 and c.map_size(166) == 0
    a.close(); b.close(); c.close()
