"""IMU de-skew and scan preprocessing without a GPU: the test model (tests/host/deskew_model.cpp) against the reference's own unit-test
answers and an independent numpy rotation, the segment rules of GetDataSegment written out sample by sample, the C ABI of
include/fls_preprocess.h, and the C++ adapter include/fls_hip_preprocess.h."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, synth
from tests import deskew_util as du

ROOT = du.ROOT


def yaw_q(deg):
    a = np.deg2rad(deg) / 2
    return np.array([0.0, 0.0, np.sin(a), np.cos(a)])


def angle(q):  # Eigen::AngleAxisd(q).angle()
    return 2.0 * np.arctan2(np.linalg.norm(q[:3]), abs(q[3]))


def test_known_answer_lidar_distortion_corrector_ut():
    """test/lidar_distortion_corrector_ut.cpp: yaw 1/3/5/7 deg at 1/3/5/7 us, ref 2 us, (1, 2, 3) at 4.000001e-6 s -> R(2)^-1 R(6) p."""
    t = np.array([1, 3, 5, 7], np.uint64)
    q = np.stack([yaw_q(d) for d in (1, 3, 5, 7)])
    out, ok = du.process_points(t, q, 2, np.eye(4), [[1, 2, 3]], [np.float32(4.000001 * 1e-6)])
    assert ok[0]
    real = (synth.quat_to_rot(yaw_q(2)).T @ synth.quat_to_rot(yaw_q(6)) @ np.array([1.0, 2.0, 3.0])).astype(np.float32)
    assert du.ulp_diff(out[0], real).max() <= 4, (out[0], real)  # EXPECT_FLOAT_EQ


def test_known_answer_motion_interpolator_ut():
    """test/motion_interpolator_ut.cpp: nlerp / slerp angles (EXPECT_DOUBLE_EQ, 4 ulps)."""
    def eq(a, b):
        assert abs(a - b) <= 4 * np.spacing(b), (a, b)
    q1, q3, q2, q6 = yaw_q(1), yaw_q(3), yaw_q(2), yaw_q(6)
    eq(angle(du.nlerp(q1, q3, 0.5)), np.deg2rad(2))
    eq(angle(du.nlerp(q1, q3, 0.0)), np.deg2rad(1))
    eq(angle(du.nlerp(q1, q3, 1.0)), np.deg2rad(3))
    for t, deg in ((3, 4), (2, 2), (4, 6)):
        eq(angle(du.slerp_ts(q2, q6, 2, 4, t)), np.deg2rad(deg))
    for t, deg in ((0.5, 4), (0.0, 2), (1.0, 6)):
        eq(angle(du.slerp(q2, q6, t)), np.deg2rad(deg))


IMU_T = np.array([0, 10, 20, 30], np.uint64)
IMU_Q = np.stack([yaw_q(d) for d in (0, 10, 25, 31)])


@pytest.mark.parametrize("left,right,expect_t,exact", [
    (5, 25, [5, 10, 25], {1: 1}),            # the sample before `end` (20) is left out
    (0, 30, [0, 10, 20, 30], {0: 0, 1: 1, 2: 2, 3: 3}),  # start / end on the front / back: the samples themselves
    (10, 30, [10, 20, 30], {1: 2, 2: 3}),    # start on a middle sample: slerp with t = 0 at the left end
    (5, 20, [5, 10, 20], {1: 1}),            # end on a middle sample: slerp(20, 30, 0), nothing between 10 and 20 left out
    (0, 25, [0, 10, 25], {0: 0, 1: 1}),
    (5, 30, [5, 10, 20, 30], {1: 1, 2: 2, 3: 3}),
])
def test_segment_rules(left, right, expect_t, exact):
    t, q = du.segment(IMU_T, IMU_Q, left, right)
    assert t.tolist() == expect_t
    for k, src in exact.items():
        assert np.array_equal(q[k], IMU_Q[src])
    if left not in IMU_T.tolist() or left == 10:
        lb = int(np.searchsorted(IMU_T, left, side="right")) - 1
        assert np.array_equal(q[0], du.slerp_ts(IMU_Q[lb], IMU_Q[lb + 1], int(IMU_T[lb]), int(IMU_T[lb + 1]), left))
    if right not in (30,):
        rb = int(np.searchsorted(IMU_T, right, side="right")) - 1
        assert np.array_equal(q[-1], du.slerp_ts(IMU_Q[rb], IMU_Q[rb + 1], int(IMU_T[rb]), int(IMU_T[rb + 1]), right))


def test_segment_empty_and_undefined():
    assert du.segment(IMU_T, IMU_Q, 12, 12)[0].size == 0  # start == end
    assert du.segment(IMU_T, IMU_Q, 14, 12)[0].size == 0
    assert du.segment(IMU_T, IMU_Q, 12, 18) is None       # the reference walks off the deque (the library: the two ends)


def _tiny_raw(times):
    raw = np.zeros(len(times), dtype=synth.RAW_POINT_DTYPE)
    raw["x"], raw["y"], raw["z"], raw["time"] = 10.0, 1.0, 0.5, np.asarray(times, np.float32)
    return raw


def test_header_stamp_outside_the_point_times():
    t, q = du.imu_for(1_000_000, before_us=50_000, after_us=150_000)
    r = du.preprocess(_tiny_raw([0.002, 0.01]), 1_000_000, t, q, np.eye(4), 1.0, 100.0, 1)
    # start widened down to the stamp; float(0.01) * 1e6 = 9999.99977... truncates to 9999
    assert (r["start"], r["end"]) == (1_000_000, 1_009_999) and r["status"] == 0
    r = du.preprocess(_tiny_raw([-0.01, -0.002]), 1_000_000, t, q, np.eye(4), 1.0, 100.0, 1)
    assert (r["start"], r["end"]) == (990_001, 1_000_000) and r["status"] == 0    # end widened up to the stamp (truncation toward zero)
    r = du.preprocess(_tiny_raw([0.0, 0.0]), 1_000_000, t, q, np.eye(4), 1.0, 100.0, 1)
    assert r["status"] == 3 and r["ordered"].shape[0] == 0 and r["planar"].shape[0] == 0  # start == end: empty segment, empty clouds
    assert du.preprocess(_tiny_raw([0.0, 0.01]), 1_000_000, t[20:], q[20:], np.eye(4), 1.0, 100.0, 1)["status"] == 1  # drop
    assert du.preprocess(_tiny_raw([0.0, 0.2]), 1_000_000, t, q, np.eye(4), 1.0, 100.0, 1)["status"] == 2             # wait


@pytest.mark.parametrize("T", [du.T_NCLT, du.T_GENERAL], ids=["nclt", "general"])
def test_model_vs_independent_rotation(T):
    """10^5 random points: the model equals an independent f64 numpy rotation (matrices, not quaternion products) within 1 float ulp."""
    rng = np.random.default_rng(7)
    stamp = 5_000_000
    t, q = du.imu_for(stamp, yaw_rate=np.deg2rad(90.0), wobble=np.deg2rad(3.0))
    n = 100_000
    xyz = (rng.uniform(-60, 60, (n, 3))).astype(np.float32)
    rel = rng.uniform(0.0, 0.1, n).astype(np.float32)
    out, ok = du.process_points(t, q, stamp, T, xyz, rel)
    assert ok.all()
    # numpy: bracket, nlerp, rotation matrices
    tp = stamp + np.trunc(rel.astype(np.float64) * 1e6).astype(np.int64)
    ti = t.astype(np.int64)

    def q_at(tt):
        l = np.clip(np.searchsorted(ti, tt, side="right") - 1, 0, ti.size - 2)
        r = (tt - ti[l]) / (ti[l + 1] - ti[l])
        qq = q[l] * (1 - r)[:, None] + q[l + 1] * r[:, None]
        return qq / np.linalg.norm(qq, axis=1, keepdims=True)
    R_ref = synth.quat_to_rot(q_at(np.array([stamp])))[0]
    R_pt = synth.quat_to_rot(q_at(tp))
    p_imu = xyz.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    expect = np.einsum("ij,njk,nk->ni", R_ref.T, R_pt, p_imu).astype(np.float32)
    assert du.ulp_diff(out, expect).max() <= 1


# ---- C ABI (no GPU needed) ------------------------------------------------------------------------------------------------
def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src)))


def test_preprocess_symbols_exported(built):
    L = _lib.lib()
    assert _declared("fls_preprocess.h") == sorted(_lib.PREPROCESS_SYMBOLS)
    for s in _lib.PREPROCESS_SYMBOLS:
        assert hasattr(L, s), s
    assert L.fls_abi_revision() >= 8


def test_preprocess_struct_layouts(built, tmp_path):
    """sizeof / offsetof of every fls_preprocess.h struct, compiled from the header, equal the ctypes mirrors."""
    structs = {"fls_raw_layout": _lib.RawLayout, "fls_preprocess_params": _lib.PreprocessParams, "fls_preprocess_result": _lib.PreprocessResult}
    lines = ['#include "fls_preprocess.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)


def test_preprocess_invalid_arguments(built):
    L = _lib.lib()
    h = C.c_void_p()
    p = _lib.PreprocessParams(C.sizeof(_lib.PreprocessParams), 1, 1.0, 100.0, 0.5, 0.0, (C.c_double * 16)(*np.eye(4).reshape(-1)))
    assert L.fls_preprocess_create(None, 0, C.byref(h)) == _lib.FLS_ERR_INVALID
    assert L.fls_preprocess_create(C.byref(p), 0, None) == _lib.FLS_ERR_INVALID
    for field, bad in (("struct_size", 8), ("lidar_point_jump_span", 0), ("planar_voxel_filter_size", -1.0)):
        q = _lib.PreprocessParams.from_buffer_copy(p)
        setattr(q, field, bad)
        assert L.fls_preprocess_create(C.byref(q), 0, C.byref(h)) == _lib.FLS_ERR_INVALID and not h.value
    q = _lib.PreprocessParams.from_buffer_copy(p)
    q.T_lidar_to_imu[3] = float("nan")
    assert L.fls_preprocess_create(C.byref(q), 0, C.byref(h)) == _lib.FLS_ERR_INVALID
    lay = _lib.RawLayout(32, 0, 16, 20, 1, 24)
    assert L.fls_preprocess_scan(None, None, 0, C.byref(lay), 0, None, None, 0, None) == _lib.FLS_ERR_INVALID
    assert L.fls_features_project_deskew(None, None, 0, C.byref(lay), 0, None, None, 0, None, None, None) == _lib.FLS_ERR_INVALID
    assert L.fls_preprocess_get(None, 0, None, 0) == 0
    assert L.fls_preprocess_get_time(None, None, None) == _lib.FLS_ERR_INVALID
    if L.fls_device_count() == 0:
        assert L.fls_preprocess_create(C.byref(p), 0, C.byref(h)) == _lib.FLS_ERR_DEVICE and not h.value  # no CPU fallback


def test_adapter_header_builds_and_links(built, tmp_path):
    exe = str(tmp_path / "preprocess_adapter_smoke")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "stubs", "preprocess"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "stubs", "preprocess_smoke.cpp"), "-o", exe,
                           "-L" + libdir, "-lfls_reg", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "preprocess adapter ok" in out.stdout, out.stdout + out.stderr
