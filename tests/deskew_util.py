"""Shared helpers of the IMU de-skew tests: the test model (tests/host/deskew_model.cpp, built here with g++ and loaded with ctypes),
the synthetic scans / IMU traces, and the two extrinsics."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from funny_lidar_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAMP_US = 1_700_000_000_123_456  # a header stamp of the order a driver writes

# config_nclt*.yaml:31-34: R = I, t = (0, 0, -0.28); and a general rotation + translation
T_NCLT = np.eye(4)
T_NCLT[2, 3] = -0.28
T_GENERAL = np.eye(4)
T_GENERAL[:3, :3] = synth.so3_exp(np.array([0.21, -0.13, 0.37]))
T_GENERAL[:3, 3] = [0.31, -0.07, 0.12]

_model = None


def model():
    global _model
    if _model is None:
        d = tempfile.mkdtemp(prefix="deskew_model_")
        so = os.path.join(d, "libdeskew_model.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                               os.path.join(ROOT, "tests", "host", "deskew_model.cpp"), "-o", so])
        L = C.CDLL(so)
        dp, fp, u64p = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint64)
        L.dm_nlerp.argtypes = [dp, dp, C.c_double, dp]
        L.dm_slerp.argtypes = [dp, dp, C.c_double, dp]
        L.dm_slerp_ts.argtypes = [dp, dp, C.c_uint64, C.c_uint64, C.c_uint64, dp]
        L.dm_segment.restype = C.c_int
        L.dm_segment.argtypes = [u64p, dp, C.c_size_t, C.c_uint64, C.c_uint64, u64p, dp, C.c_size_t]
        L.dm_process_points.restype = C.c_int
        L.dm_process_points.argtypes = [u64p, dp, C.c_size_t, C.c_uint64, dp, fp, fp, C.c_size_t, fp, C.POINTER(C.c_uint8)]
        L.dm_preprocess.restype = None
        L.dm_preprocess.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, u64p, dp, C.c_size_t, dp,
                                    C.c_float, C.c_float, C.c_int, fp, C.POINTER(C.c_int32), fp, u64p, u64p, fp]
        _model = L
    return _model


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def q_arr(q):
    return np.ascontiguousarray(q, dtype=np.float64)


def nlerp(a, b, t):
    out = np.zeros(4)
    model().dm_nlerp(_p(q_arr(a), C.c_double), _p(q_arr(b), C.c_double), t, _p(out, C.c_double))
    return out


def slerp(a, b, t):
    out = np.zeros(4)
    model().dm_slerp(_p(q_arr(a), C.c_double), _p(q_arr(b), C.c_double), t, _p(out, C.c_double))
    return out


def slerp_ts(a, b, t0, t1, t):
    out = np.zeros(4)
    model().dm_slerp_ts(_p(q_arr(a), C.c_double), _p(q_arr(b), C.c_double), t0, t1, t, _p(out, C.c_double))
    return out


def segment(t_us, q, left, right):
    t = np.ascontiguousarray(t_us, dtype=np.uint64)
    q = q_arr(q)
    ot, oq = np.zeros(t.size + 2, np.uint64), np.zeros((t.size + 2, 4))
    m = model().dm_segment(_p(t, C.c_uint64), _p(q, C.c_double), t.size, left, right, _p(ot, C.c_uint64), _p(oq, C.c_double), ot.size)
    if m < 0:
        return None
    return ot[:m], oq[:m]


def process_points(t_us, q, ref, T, xyz, rel):
    t = np.ascontiguousarray(t_us, dtype=np.uint64)
    q = q_arr(q)
    Tc = np.ascontiguousarray(np.asarray(T, dtype=np.float64).T.reshape(-1))  # column-major
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    rel = np.ascontiguousarray(rel, dtype=np.float32).reshape(-1)
    out, ok = np.zeros_like(xyz), np.zeros(xyz.shape[0], np.uint8)
    model().dm_process_points(_p(t, C.c_uint64), _p(q, C.c_double), t.size, ref, _p(Tc, C.c_double), _p(xyz, C.c_float), _p(rel, C.c_float),
                              xyz.shape[0], _p(out, C.c_float), _p(ok, C.c_uint8))
    return out, ok.astype(bool)


def preprocess(raw, stamp, t_us, q, T, min_d, max_d, span, want_all=False):
    """The model's non-LOAM loop: dict(status, start, end, n_seg, ordered, ordered_index, planar[, deskew_all])."""
    raw = np.ascontiguousarray(raw)
    f = raw.dtype.fields
    t = np.ascontiguousarray(t_us, dtype=np.uint64)
    q = q_arr(q)
    Tc = np.ascontiguousarray(np.asarray(T, dtype=np.float64).T.reshape(-1))
    n = raw.shape[0]
    ordered, idx, planar = np.zeros((max(n, 1), 4), np.float32), np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 4), np.float32)
    counts, info = np.zeros(2, np.uint64), np.zeros(4, np.uint64)
    alld = np.zeros((max(n, 1), 4), np.float32) if want_all else None
    model().dm_preprocess(raw.ctypes.data, n, raw.dtype.itemsize, f["x"][1], f["intensity"][1], f["time"][1], stamp, _p(t, C.c_uint64),
                          _p(q, C.c_double), t.size, _p(Tc, C.c_double), min_d, max_d, span, _p(ordered, C.c_float), _p(idx, C.c_int32),
                          _p(planar, C.c_float), _p(counts, C.c_uint64), _p(info, C.c_uint64), None if alld is None else _p(alld, C.c_float))
    no, npl = int(counts[0]), int(counts[1])
    out = dict(status=int(info[0]), start=int(info[1]), end=int(info[2]), n_seg=int(info[3]), ordered=ordered[:no], ordered_index=idx[:no],
               planar=planar[:npl])
    if want_all:
        out["deskew_all"] = alld[:n]
    return out


def raw_scan(seed=0, n_az=1800, stamp_us=STAMP_US, **motion):
    """configs[1]-sized raw Velodyne-64 scan (RAW_POINT_DTYPE, ~115k points) with the per-point time: (as seen at the header stamp,
    as measured by the sensor turning during the sweep), and configs[1]'s ground-truth pose."""
    cfg = synth.make_config(1, scale=1.0, with_map=False)
    lid = dict(synth.VELODYNE_64)
    lid["n_az"] = n_az
    raw = synth.cast_raw_scan(cfg["scene"], cfg["T_gt"], rng=np.random.default_rng(100 + seed), **lid)
    return raw, synth.sweep_distort(raw, stamp_us, stamp_us, **motion), cfg["T_gt"]


def imu_for(stamp_us=STAMP_US, before_us=20_000, after_us=130_000, **motion):
    """A 200 Hz trace around one sweep (origin of the motion = the header stamp)."""
    return synth.imu_trace(stamp_us - before_us, stamp_us + after_us, stamp_us, **motion)


def ulp_diff(a, b):
    """|a - b| in float32 ulps (same-sign finite floats)."""
    ai = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    bi = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, np.int64(-2**31) - ai, ai)
    bi = np.where(bi < 0, np.int64(-2**31) - bi, bi)
    return np.abs(ai - bi)
