"""GPU: the loop-closure Match from clouds on the device (include/fls_loop_device.h) against fls_loop_match on the same points as host rows:
T as uint64 bits, the fitness as uint32 bits, bytes(stats) -- equal, whatever the path the ten filters and four leaf builds took; the counters
of fls_loop_device_stat say which path that was.  Device buffers come from hipMalloc through ctypes (tests/loop_device_util.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, keyframes, registration as reg, synth
from tests import loop_device_util as U, loopdata

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"


@pytest.fixture(scope="module")
def pair():
    """the pair of tests/test_gpu_keyframes.py's loop test and fls_loop_match's answer for it (computed once, never changed)"""
    src, tgt, Tt = loopdata.make_pair(job=3, n_az=200, n_t=2, n_s=2)
    rng = np.random.default_rng(3)  # an intensity column, so that the fourth plane is there (no result depends on it)
    src, tgt = [np.ascontiguousarray(np.c_[c[:, :3], rng.uniform(0.0, 255.0, len(c))], np.float32) for c in (src, tgt)]
    T, f, st = U.match_rows(src, tgt)
    et, er = synth.pose_error(T, Tt)
    assert et < 0.05 and er < 5e-3 and st.gicp_iterations > 0, (et, er)
    for a in (src, tgt):
        a.setflags(write=False)
    return src, tgt, Tt, U.result(T, f, st)


def test_equals_loop_match_on_rows(pair):
    src, tgt, Tt, want = pair
    before = U.stats()
    T, f, st = U.match_device(src, tgt)
    assert U.result(T, f, st) == want
    et, er = synth.pose_error(T, Tt)
    assert et < 0.05 and er < 5e-3, (et, er)
    # ten filters and four leaf grids on the device, nothing declined, nothing of the inputs downloaded
    d = U.delta(before)
    assert d[:6] == [1, 10, 0, 4, 0, 0], d
    assert reg.loop_device_stats()["matches"] == U.stats()[0]


def test_unaligned_planes(pair):
    src, tgt, _, want = pair
    before = U.stats()
    assert U.result(*U.match_device(src, tgt, skew=4)) == want
    assert U.delta(before)[:6] == [1, 10, 0, 4, 0, 0]


def test_null_intensity_planes(pair):
    src, tgt, _, want = pair
    before = U.stats()
    got = U.result(*U.match_device(src, tgt, intensity=False))
    assert got == U.result(*U.match_rows(src[:, :3], tgt[:, :3])), "rows of three floats: intensity 0"
    assert got == want, "no result depends on the intensity"
    assert U.delta(before)[:6] == [1, 10, 0, 4, 0, 0]


def test_keyframe_variant(pair):
    """the grouping of tests/test_gpu_keyframes.py: 3 + 4 keyframes under random poses"""
    src, tgt, Tt, _ = pair
    rng = np.random.default_rng(7)
    s = keyframes.KeyframeStore()

    def group(cloud, n):
        P = np.tile(np.eye(4), (n, 1, 1))
        ids = []
        for k, part in enumerate(np.array_split(cloud, n)):
            P[k, :3, :3] = synth.so3_exp(rng.normal(size=3))
            P[k, :3, 3] = rng.uniform(-5.0, 5.0, 3)
            Ti = np.linalg.inv(P[k])
            ids.append(s.add((part[:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)))
        return ids, P

    si, sp = group(src, 3)
    ti, tp = group(tgt, 4)
    T1, T2 = np.eye(4), np.eye(4)
    f1, st1 = s.loop_match(si, sp, ti, tp, T1)
    before = U.stats()
    f2, st2 = s.loop_match(si, sp, ti, tp, T2, on_device=True)
    assert U.result(T1, f1, st1) == U.result(T2, f2, st2) and st2.gicp_iterations > 0
    et, er = synth.pose_error(T2, Tt)
    assert et < 0.05 and er < 5e-3, (et, er)
    d = U.delta(before)
    assert d[:6] == [1, 10, 0, 4, 0, 0], d
    # empty selections answer what fls_keyframes_loop_match answers
    T3, T4 = np.eye(4), np.eye(4)
    f3, st3 = s.loop_match([], np.zeros((0, 4, 4)), ti, tp, T3)
    f4, st4 = s.loop_match([], np.zeros((0, 4, 4)), ti, tp, T4, on_device=True)
    assert U.result(T3, f3, st3) == U.result(T4, f4, st4) and f4 == FLT_MAX
    s.close()


def test_declined_filter_goes_through_the_host(pair):
    """a target with one NaN row: its five filters decline, the cloud is downloaded once (every plane it has), the results are fls_loop_match's"""
    src, tgt, _, _ = pair
    bad = np.insert(tgt, 1234, np.full(tgt.shape[1], np.nan, np.float32), axis=0)
    want = U.result(*U.match_rows(src, bad))
    before = U.stats()
    assert U.result(*U.match_device(src, bad)) == want
    d = U.delta(before)
    assert d[:6] == [1, 5, 5, 4, 0, bad.size * 4], d


CHILD = r'''
import json, os, sys
sys.path.insert(0, os.environ["FLS_ROOT"])
from tests import loop_device_util as U, loopdata
src, tgt, _ = loopdata.make_pair(job=3, n_az=200, n_t=2, n_s=2)
rows = U.result(*U.match_rows(src, tgt))
before = U.stats()
dev = U.result(*U.match_device(src, tgt))
print("RESULT " + json.dumps({"equal": rows == dev, "rows": rows, "delta": U.delta(before), "bytes": int(src.nbytes + tgt.nbytes)}))
'''


@pytest.mark.parametrize("name,value", [("FLS_LOOP_DEVICE_LEAVES", "0"), ("FLS_DEVICE_VOXELGRID", "0")])
def test_environment_switches(pair, name, value):
    """a child process each: the switch is read when the matcher is created (leaves) or per call (filters)"""
    env = dict(os.environ, FLS_ROOT=ROOT)
    env[name] = value
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    assert out["equal"] and (out["rows"][0], out["rows"][1], out["rows"][2]) == pair[3], "the switch changes the path, not the result"
    d = out["delta"]
    if name == "FLS_LOOP_DEVICE_LEAVES":
        assert d[:6] == [1, 10, 0, 0, 4, 0] and d[6] > 0, d  # the four filtered targets are downloaded for build_target
    else:
        assert d[:6] == [1, 0, 10, 4, 0, out["bytes"]], d  # each input downloaded once


def test_small_sides(pair):
    src, tgt, _, _ = pair
    few = np.ascontiguousarray(src[:15])
    none = np.zeros((0, src.shape[1]), np.float32)
    for a, b in ((few, tgt), (src, np.ascontiguousarray(tgt[:19])), (none, tgt), (src, none), (none, none)):
        T0 = np.eye(4)
        T0[:3, 3] = (0.25, -0.5, 0.125)
        want = U.match_rows(a, b, T0)
        got = U.match_device(a, b, T0)
        assert U.result(*got) == U.result(*want), (a.shape, b.shape)
        assert got[1] == FLT_MAX and got[2].gicp_iterations == 0


def test_calls_are_independent(pair):
    """the per-device buffers carry nothing over: the same call after a call on other clouds gives the same bits"""
    src, tgt, _, want = pair
    other_s, other_t, _ = loopdata.make_pair(job=1, n_az=150, n_t=3, n_s=2)
    assert U.result(*U.match_device(src, tgt)) == want
    assert U.result(*U.match_device(other_s, other_t)) == U.result(*U.match_rows(other_s, other_t))
    assert U.result(*U.match_device(src, tgt)) == want
