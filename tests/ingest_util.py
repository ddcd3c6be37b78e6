"""Shared helpers of the driver-cloud front end tests: the test model (tests/host/ingest_model.cpp, built here with g++ and loaded with
ctypes), the product's host-compilable pieces (tests/host/ingest_product_shim.cpp, built with hipcc), and the test messages."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from funny_lidar_slam_amd import preprocess, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENSORS = list(synth.SENSORS)
B = 256  # workgroup size of the conversion kernels (kIngestThreads)
# LidarModel of a 16-ring Velodyne (lidar_model.cpp:24-30) for the None branch: lower_angle = 15 deg, v_res = 2 deg
VSN, LOWER, VRES = 16, float(np.float32(np.deg2rad(15.0))), float(np.float32(np.deg2rad(2.0)))

_model = None
_shim = None


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def model():
    global _model
    if _model is None:
        d = tempfile.mkdtemp(prefix="ingest_model_")
        so = os.path.join(d, "libingest_model.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                               os.path.join(ROOT, "tests", "host", "ingest_model.cpp"), "-o", so])
        L = C.CDLL(so)
        dp, fp, bp = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        L.im_atan2.restype = C.c_double
        L.im_atan2.argtypes = [C.c_double, C.c_double]
        L.im_atan2_many.argtypes = [dp, dp, C.c_size_t, dp]
        L.im_fast_atan2.restype = C.c_float
        L.im_fast_atan2.argtypes = [C.c_float, C.c_float]
        L.im_period_loop.argtypes = [fp, bp, bp, C.c_size_t, C.c_int, fp]
        L.im_convert.restype = C.c_size_t
        L.im_convert.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.c_double, C.c_int, C.c_float, C.c_float,
                                 C.c_uint64, C.c_void_p, C.POINTER(C.c_int32), dp, C.POINTER(C.c_uint64), bp]
        _model = L
    return _model


def product_shim():
    """The product's A(y, x) and step-function combine operator, compiled for the host from kernels_ingest.hpp."""
    global _shim
    if _shim is None:
        d = tempfile.mkdtemp(prefix="ingest_shim_")
        so = os.path.join(d, "libingest_shim.so")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                               "-Wno-unused-result", "-Wno-unused-function", os.path.join(ROOT, "tests", "host", "ingest_product_shim.cpp"), "-o", so])
        L = C.CDLL(so)
        dp, fp, bp = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        L.ip_atan2_many.argtypes = [dp, dp, C.c_size_t, dp]
        L.ip_base_time.restype = C.c_float
        L.ip_base_time.argtypes = [C.c_float] * 4
        L.ip_period_scan.argtypes = [fp, bp, bp, C.c_size_t, C.c_int, C.c_size_t, fp]
        _shim = L
    return _shim


def atan2_many(y, x, lib=None):
    y, x = np.ascontiguousarray(y, np.float64), np.ascontiguousarray(x, np.float64)
    out = np.zeros_like(y)
    fn = model().im_atan2_many if lib is None else lib.ip_atan2_many
    fn(_p(y, C.c_double), _p(x, C.c_double), y.size, _p(out, C.c_double))
    return out


def convert(msg, sensor, is_dense=True, scale=1.0, vsn=VSN, lower=LOWER, vres=VRES, stamp=0, cloud=None):
    """The model's ConvertMessageToCloud: dict(rows (CONVERTED_DTYPE), index, n, min, max, last, t0, timeless, stamp_out, branch)."""
    msg = np.ascontiguousarray(msg)
    dc = preprocess.driver_cloud(msg.dtype, synth.SENSORS[sensor], is_dense) if cloud is None else cloud
    off = np.array([dc.x_offset, dc.y_offset, dc.z_offset, dc.intensity_offset, dc.ring_offset, dc.time_offset, dc.tag_offset, dc.line_offset], np.uint32)
    n = msg.shape[0]
    rows = np.zeros(max(n, 1), dtype=preprocess.CONVERTED_DTYPE)
    idx, info, branch = np.zeros(max(n, 1), np.int32), np.zeros(6), np.zeros(max(n, 1), np.uint8)
    so = C.c_uint64()
    m = model().im_convert(msg.ctypes.data, n, dc.sensor, dc.point_step, dc.is_dense, _p(off, C.c_uint32), scale, vsn, lower, vres, stamp,
                           rows.ctypes.data, _p(idx, C.c_int32), _p(info, C.c_double), C.byref(so), _p(branch, C.c_uint8))
    return dict(rows=rows[:m], index=idx[:m], n=m, min=np.float32(info[1]), max=np.float32(info[2]), last=np.float32(info[3]), t0=float(info[4]),
                timeless=bool(info[5]), stamp_out=int(so.value), branch=branch[:m])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def firing_scan(n_rings=16, n_az=400, revolutions=1.2, seed=0, r_lo=5.0, r_hi=40.0):
    """A Velodyne message in firing order (azimuth-major, rings interleaved), `revolutions` turns clockwise as a spinning lidar sweeps,
    every time zero: the cloud of a driver without point times (NCLT)."""
    rng = np.random.default_rng(seed)
    n = n_rings * n_az
    raw = np.zeros(n, dtype=synth.RAW_POINT_DTYPE)
    ring = np.tile(np.arange(n_rings), n_az)
    az = 0.3 - np.repeat(np.arange(n_az), n_rings) * (2.0 * np.pi * revolutions / n_az)  # yaw decreases: time = (first - yaw) / omega grows
    el = np.deg2rad(-15.0 + 2.0 * ring)
    r = rng.uniform(r_lo, r_hi, n)
    raw["x"], raw["y"], raw["z"] = r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)
    raw["intensity"] = rng.uniform(0, 255, n)
    raw["ring"] = ring
    return raw
