"""GPU: the device keyframe store (include/fls_keyframes.h).  Every expected value is a restatement built here from two things:
fls_voxel_grid_cloud(..., FLS_VOXELGRID_EXACT, ...) for the filter (pinned to the reference's filter by tests/test_abi.py) and a numpy
float32 restatement of TransformPointCloud(cloud, Mat4d) -- R and t cast to float, then (r0*x + (r1*y + r2*z)) + t per row;
elementwise float32 operations are IEEE and do not contract.  Comparisons are on bits."""
import ctypes as C

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, keyframes, preprocess, registration as reg, synth
from tests import deskew_util as du, loopdata
from tests.test_gpu_preprocess import LEAF, MAX_D, MIN_D, SPAN, STAMP

pytestmark = pytest.mark.gpu

FP, DP, IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def exact(cloud, leaf):
    return reg.VoxelGridCloud(cloud, leaf, on_device=False)


def xform(cloud, T):
    R, t = T[:3, :3].astype(np.float32), T[:3, 3].astype(np.float32)
    x, y, z = cloud[:, 0], cloud[:, 1], cloud[:, 2]
    out = np.empty((cloud.shape[0], 4), np.float32)
    for r in range(3):
        out[:, r] = (R[r, 0] * x + (R[r, 1] * y + R[r, 2] * z)) + t[r]
    out[:, 3] = cloud[:, 3]
    return out


def restate(clouds, ids, poses, leaf_each=0.0, leaf_final=0.0, filtered=None):
    parts = []
    for k, i in enumerate(ids):
        c = clouds[i] if leaf_each == 0 else (filtered[i] if filtered is not None else exact(clouds[i], leaf_each))
        parts.append(xform(c, poses[k]))
    out = np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)
    return exact(out, leaf_final) if leaf_final > 0 else out


def random_poses(rng, n, reach):
    P = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        P[k, :3, :3] = synth.so3_exp(rng.normal(size=3))
        P[k, :3, 3] = rng.uniform(-reach, reach, 3)
    return P


def random_cloud(rng, n, box=40.0):
    c = rng.uniform(-box / 2, box / 2, (n, 4)).astype(np.float32)
    c[:, 3] = rng.uniform(0, 255, n).astype(np.float32)
    return c


def make_store(clouds):
    s = keyframes.KeyframeStore()
    assert [s.add(c) for c in clouds] == list(range(len(clouds))) and len(s) == len(clouds)
    return s


@pytest.fixture(scope="module")
def sub41():
    """41 keyframes of about 3,000 points in a 40 m box, and their exact 0.2 m filters (computed once, never changed)"""
    rng = np.random.default_rng(41)
    clouds = [random_cloud(rng, 3000 + int(rng.integers(-200, 200))) for _ in range(41)]
    return clouds, [exact(c, 0.2) for c in clouds]


# ---- 1. segment boundaries ---------------------------------------------------------------------------------------------------------
def test_merge_segment_boundaries():
    rng = np.random.default_rng(1)
    sizes = [1, 63, 64, 65, 255, 0, 256, 257, 5000]  # an empty keyframe in the middle
    clouds = [random_cloud(rng, n) for n in sizes]
    s = make_store(clouds)
    every = list(range(len(sizes)))
    many_tiny = [0, 5] * 200 + [8] + [5, 0] * 100  # more segments in one tile than a workgroup stages at once, empty ones among them
    for ids in (every, every[::-1], [3, 8, 3, 5, 8, 0], [8], [5], [5, 5, 2], many_tiny):
        P = random_poses(rng, len(ids), 1.0e4)  # translations of kilometres: the float cast of t matters
        got = s.merge(ids, P, 0.0, 0.0)
        assert got.shape[0] == sum(sizes[i] for i in ids)
        assert same(got, restate(clouds, ids, P)), ids[:8]
    assert s.stats()["filters_run"] == 0 and s.stats()["stored_points"] == sum(sizes)
    for i in every:
        assert same(s.get(i), clouds[i])


# ---- 2. GetSubMap shape ------------------------------------------------------------------------------------------------------------
def test_getsubmap_shape_one_launch_41_filters(sub41):
    clouds, filtered = sub41
    s = make_store(clouds)
    ids = list(range(41))
    P = random_poses(np.random.default_rng(2), 41, 30.0)
    before = s.stats()
    got = s.merge(ids, P, 0.2, 0.0)
    after = s.stats()
    assert same(got, restate(clouds, ids, P, 0.2, filtered=filtered))
    assert after["filters_run"] - before["filters_run"] == 41 and after["merge_launches"] - before["merge_launches"] == 1
    assert after["filters_declined"] == 0 and after["cached_clouds"] == 41
    # GetSubMap itself: the range clipped to the keyframes there are, poses relative to the reference keyframe
    sel_ids, sel = keyframes.KeyframeStore.submap_selection(38, 20, 20, True, P)
    assert list(sel_ids) == list(range(18, 41)) and np.allclose(sel[20], np.eye(4), atol=1e-9)
    assert same(s.submap(38, 20, 20, True, P), restate(clouds, sel_ids, sel, 0.2, filtered=filtered))


# ---- 3. the cache ------------------------------------------------------------------------------------------------------------------
def test_cache_hits_new_poses_and_eviction(sub41):
    clouds, filtered = sub41
    s = make_store(clouds)
    ids = list(range(41))
    rng = np.random.default_rng(3)
    s.merge(ids, random_poses(rng, 41, 30.0), 0.2, 0.0)
    P2 = random_poses(rng, 41, 30.0)
    before = s.stats()
    got = s.merge(ids, P2, 0.2, 0.0)
    after = s.stats()
    assert after["filters_run"] == before["filters_run"] and after["cache_hits"] - before["cache_hits"] == 41
    assert same(got, restate(clouds, ids, P2, 0.2, filtered=filtered))
    first = s.get(7, 0.2)
    assert same(first, exact(s.get(7, 0.0), 0.2)) and same(first, filtered[7])
    for leaf in (0.3, 0.5, 0.7):  # slots two to four of keyframe 7
        n = s.stats()["cached_clouds"]
        assert same(s.get(7, leaf), exact(clouds[7], leaf))
        assert s.stats()["cached_clouds"] == n + 1
    full = s.stats()
    assert same(s.get(7, 1.0), exact(clouds[7], 1.0))  # a fifth leaf size: the oldest entry (0.2) goes
    assert s.stats()["cached_clouds"] == full["cached_clouds"] and s.stats()["filters_run"] == full["filters_run"] + 1
    mid = s.stats()
    assert same(s.get(7, 0.3), exact(clouds[7], 0.3)) and s.stats()["filters_run"] == mid["filters_run"]  # still cached
    again = s.get(7, 0.2)  # recomputed
    assert s.stats()["filters_run"] == mid["filters_run"] + 1 and s.stats()["cached_clouds"] == full["cached_clouds"]
    assert same(again, first)
    assert s.stats()["bytes_resident"] >= 16 * s.stats()["stored_points"]


# ---- 4. SaveMap shape --------------------------------------------------------------------------------------------------------------
def test_savemap_shape_filters_each_and_the_merged_cloud(sub41):
    clouds = sub41[0][:8]
    s = make_store(clouds)
    ids = [0, 1, 2, 3, 4, 5, 6, 7]
    P = random_poses(np.random.default_rng(4), 8, 10.0)  # overlapping clouds: the final filter has leaves to merge
    got = s.merge(ids, P, 0.3, 0.3)
    want = restate(clouds, ids, P, 0.3, 0.3)
    assert 0 < want.shape[0] < sum(exact(c, 0.3).shape[0] for c in clouds)
    assert same(got, want)
    assert same(s.merge(ids, P, 0.0, 0.3), restate(clouds, ids, P, 0.0, 0.3))


# ---- 5. a filter the device declines -----------------------------------------------------------------------------------------------
def test_declined_device_filter_takes_the_exact_host_filter(sub41):
    clouds = [c.copy() for c in sub41[0][:3]]
    clouds[1][17, 1] = np.nan
    s = make_store(clouds)
    P = random_poses(np.random.default_rng(5), 3, 30.0)
    before = s.stats()
    got = s.merge([0, 1, 2], P, 0.2, 0.0)
    want = restate(clouds, [0, 1, 2], P, 0.2)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    assert s.stats()["filters_declined"] - before["filters_declined"] == 1 and s.stats()["filters_run"] - before["filters_run"] == 3
    empty = make_store([np.zeros((0, 4), np.float32)])  # an empty cloud is declined as well
    assert empty.merge([0], np.eye(4)[None], 0.2, 0.2).shape == (0, 4) and empty.stats()["filters_declined"] == 1


# ---- 6. device hand-over -----------------------------------------------------------------------------------------------------------
def test_add_preprocessed_device_to_device():
    static, moving, T_gt = du.raw_scan(0, n_az=300)
    t, q = du.imu_for()
    pre = preprocess.ScanPreprocessor(MIN_D, MAX_D, SPAN, LEAF, du.T_NCLT)
    res = pre.scan_device(moving, STAMP, t, q)
    assert res.status == _lib.FLS_OK and res.n_ordered > 1000
    s = keyframes.KeyframeStore()
    for which in ("ordered", "planar", "planar_filtered"):
        i = s.add_preprocessed(pre, which)
        assert same(s.get(i, 0.0), pre.get(which)), which
    assert len(s) == 3 and s.stats()["stored_points"] == res.n_ordered + res.n_planar + res.n_planar_filtered
    # the next scan may overwrite the handle's buffers: the stored keyframe is a copy
    ordered = pre.get("ordered").copy()
    pre.scan_device(moving[::-1].copy(), STAMP, t, q)
    assert same(s.get(0, 0.0), ordered)
    res = pre.scan_device(moving, STAMP, t[5:], q[5:])  # DROP
    assert (res.status, res.imu_status) == (_lib.FLS_ERR_STATE, _lib.FLS_IMU_DROP)
    with pytest.raises(_lib.FlsError) as e:
        s.add_preprocessed(pre, "ordered")
    assert e.value.status == _lib.FLS_ERR_STATE and len(s) == 3
    kid = C.c_int32(-7)
    assert _lib.lib().fls_keyframes_add_preprocessed(s._h, pre._h, 1, C.byref(kid)) == _lib.FLS_ERR_INVALID and kid.value == -7


# ---- 7. loop match -----------------------------------------------------------------------------------------------------------------
def test_loop_match_equals_loop_match_on_the_merged_clouds():
    src, tgt, Tt = loopdata.make_pair(job=3, n_az=200, n_t=2, n_s=2)
    rng = np.random.default_rng(7)
    s = keyframes.KeyframeStore()

    def group(cloud, n):  # n keyframes that the poses put back where make_pair had the points
        P = random_poses(rng, n, 5.0)
        ids = []
        for part, T in zip(np.array_split(cloud, n), P):
            Ti = np.linalg.inv(T)
            local = (part.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
            ids.append(s.add(local))
        return ids, P

    si, sp = group(src, 3)
    ti, tp = group(tgt, 4)
    a, b = s.merge(si, sp, 0.2, 0.0), s.merge(ti, tp, 0.2, 0.0)
    assert a.shape[0] > 1000 and b.shape[0] > 1000
    T1, T2 = np.eye(4), np.eye(4)
    f1, st1 = reg.LoopClosureMatch(a, b, T1)
    f2, st2 = s.loop_match(si, sp, ti, tp, T2)
    assert np.array_equal(T1.view(np.uint64), T2.view(np.uint64))
    assert np.float32(f1).view(np.uint32) == np.float32(f2).view(np.uint32)
    assert bytes(st1) == bytes(st2) and st2.gicp_iterations > 0
    et, er = synth.pose_error(T2, Tt)
    assert et < 0.05 and er < 5e-3, (et, er)


# ---- 8. errors and independence ----------------------------------------------------------------------------------------------------
def test_errors_and_two_stores():
    rng = np.random.default_rng(8)
    ca, cb = [random_cloud(rng, 700), random_cloud(rng, 300)], [random_cloud(rng, 1500)]
    a, b = make_store(ca), make_store(cb)
    L = _lib.lib()
    out = np.zeros((2000, 4), np.float32)
    n = C.c_size_t(99)
    I = np.ascontiguousarray(np.tile(np.eye(4).reshape(-1), (3, 1)))

    def merge(store, ids, cap, leaf=(0.0, 0.0), ptr=out):
        i = np.asarray(ids, np.int32)
        return L.fls_keyframes_merge(store._h, i.ctypes.data_as(IP), I.ctypes.data_as(DP), len(ids), np.float32(leaf[0]), np.float32(leaf[1]),
                                     ptr.ctypes.data_as(FP) if ptr is not None else None, cap, C.byref(n))

    for bad in ([-1], [0, 2], [2]):
        assert merge(a, bad, 2000) == _lib.FLS_ERR_INVALID
    assert L.fls_keyframes_get(a._h, 2, np.float32(0), out.ctypes.data_as(FP), 2000, C.byref(n)) == _lib.FLS_ERR_INVALID
    assert L.fls_keyframes_get(a._h, -1, np.float32(0), out.ctypes.data_as(FP), 2000, C.byref(n)) == _lib.FLS_ERR_INVALID
    for leaf in ((-0.1, 0.0), (0.0, np.nan), (np.inf, 0.0)):
        assert merge(a, [0], 2000, leaf) == _lib.FLS_ERR_INVALID
    assert merge(a, [0, 1], 999) == _lib.FLS_ERR_INVALID and n.value == 1000  # too small: the size is reported
    assert merge(a, [0, 1], 0, ptr=None) == _lib.FLS_ERR_INVALID and n.value == 1000
    want_f = exact(np.concatenate(ca), 5.0).shape[0]
    assert merge(a, [0, 1], want_f - 1, (0.0, 5.0)) == _lib.FLS_ERR_INVALID and n.value == want_f
    assert merge(a, [0, 1], 1000) == _lib.FLS_OK and n.value == 1000 and same(out[:1000], np.concatenate(ca))
    assert merge(a, [], 0, ptr=None) == _lib.FLS_OK and n.value == 0
    assert a.merge([], np.zeros((0, 4, 4))).shape == (0, 4)
    # two stores on one device
    P = random_poses(rng, 2, 100.0)
    ga = a.merge([1, 0], P, 0.2, 0.0)
    gb = b.merge([0, 0], P, 0.2, 0.0)
    assert same(a.merge([1, 0], P, 0.2, 0.0), ga) and same(ga, restate(ca, [1, 0], P, 0.2)) and same(gb, restate(cb, [0, 0], P, 0.2))
    assert (len(a), len(b)) == (2, 1) and a.stats()["filters_run"] == 2 and b.stats()["filters_run"] == 1 and b.stats()["cache_hits"] == 1
    b.close()
    assert same(a.get(1, 0.2), exact(ca[1], 0.2))
