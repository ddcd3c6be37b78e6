"""The driver-cloud front end without a GPU (include/fls_ingest.h): the test model (tests/host/ingest_model.cpp) against a numpy
restatement of ConvertMessageToCloud per sensor, the yaw function A(y, x) against numpy.arctan2, the step-function scan of
ComputePointOffsetTime against the sequential loop, the C ABI and its ctypes mirrors, and the C++ adapter's smoke program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, preprocess, synth
from tests import ingest_util as iu

ROOT = iu.ROOT


def small_raw(n=500, seed=3):
    rng = np.random.default_rng(seed)
    raw = np.zeros(n, dtype=synth.RAW_POINT_DTYPE)
    raw["x"], raw["y"], raw["z"] = rng.uniform(-30, 30, n), rng.uniform(-30, 30, n), rng.uniform(-3, 3, n)
    raw["intensity"] = rng.uniform(0, 255, n)
    raw["ring"] = rng.integers(0, 16, n)
    raw["time"] = np.sort(rng.uniform(0.0, 0.1, n)).astype(np.float32)
    return raw


def np_fast_atan2(y, x):
    """include/common/math_function.h FastAtan2<float>, vectorised in float32."""
    f = np.float32
    y, x = np.asarray(y, f), np.asarray(x, f)
    p1, p3, p5, p7 = f(0.9997878412794807), f(-0.3258083974640975), f(0.1555786518463281), f(-0.04432655554792128)
    ax, ay, eps = np.abs(x), np.abs(y), f(1.1920928955078125e-07)
    big = ax >= ay
    c = np.where(big, ay / (ax + eps), ax / (ay + eps)).astype(f)
    c2 = c * c
    poly = ((((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c).astype(f)
    a = np.where(big, poly, f(1.57079632679489661923) - poly).astype(f)
    a = np.where(x < 0, f(np.pi) - a, a).astype(f)
    a = np.where(y < 0, f(2 * np.pi) - a, a).astype(f)
    return np.where(a > f(np.pi), a - f(2 * np.pi), a).astype(f)


def np_convert(msg, sensor, is_dense, scale):
    """(kept message indices, ring, time) of ConvertMessageToCloud, without ComputePointOffsetTime."""
    fin = np.isfinite(msg["x"]) & np.isfinite(msg["y"]) & np.isfinite(msg["z"])
    ring = np.zeros(msg.shape[0], np.uint8)
    if sensor == "livox_avia":
        cls = msg["tag"] & 0x30
        keep = (msg["line"] < 6) & ((cls == 0x10) | (cls == 0x00))
    elif sensor == "none":
        with np.errstate(invalid="ignore", over="ignore"):
            xy = np.sqrt(msg["x"] * msg["x"] + msg["y"] * msg["y"])
            row = np.round((np_fast_atan2(msg["z"], xy) + np.float32(iu.LOWER)) / np.float32(iu.VRES))
        keep = fin & (row >= 0) & (row < iu.VSN)
        ring = np.where(keep, row, 0).astype(np.uint8)
    else:
        keep = fin | bool(is_dense)
    k = np.nonzero(keep)[0]
    if sensor in ("velodyne", "ouster", "robosense", "leishen"):
        ring = (msg["ring"].astype(np.int64) & 0xFF).astype(np.uint8)
    if sensor == "velodyne":
        t = (msg["time"].astype(np.float64) * scale).astype(np.float32)
    elif sensor == "ouster":
        t = (msg["t"].astype(np.float64) * scale).astype(np.float32)
    elif sensor == "livox_avia":
        t = (msg["time"].astype(np.float64) * scale).astype(np.float32)
    elif sensor == "leishen":
        t = (msg["timestamp"] * scale).astype(np.float32)
    elif sensor in ("robosense", "livox_mid_360"):
        t0 = msg["timestamp"][k[0]] if k.size else 0.0
        t = ((msg["timestamp"] - t0) * scale).astype(np.float32)
    else:
        t = np.zeros(msg.shape[0], np.float32)
    return k, ring[k], t[k]


@pytest.mark.parametrize("sensor", iu.SENSORS)
@pytest.mark.parametrize("dense", [True, False])
def test_model_equals_numpy_per_sensor(sensor, dense):
    raw = small_raw()
    if sensor == "none":
        raw["z"] = np.random.default_rng(5).uniform(-12, 12, raw.shape[0])  # rows below 0 and above 15 occur
    stamp = 1_700_000_000_123_456
    msg = synth.driver_message(sensor, raw, stamp)
    if not dense or sensor == "none":
        msg = synth.punch_nonfinite(msg, np.arange(0, raw.shape[0], 7))
    scale = synth.DRIVER_TIME_SCALE[sensor]
    m = iu.convert(msg, sensor, dense, scale, stamp=stamp)
    k, ring, t = np_convert(msg, sensor, dense, scale)
    assert m["n"] == k.size and 0 < k.size and np.array_equal(m["index"], k)
    if sensor not in ("livox_avia",) and (not dense or sensor == "none"):
        assert k.size < msg.shape[0]
    for f in ("x", "y", "z", "intensity"):
        assert iu.bits(m["rows"][f]) == iu.bits(msg[f][k]), f
    assert np.array_equal(m["rows"]["ring"], ring)
    assert not m["timeless"] or sensor == "none"
    if sensor != "none":
        assert iu.bits(m["rows"]["time"]) == iu.bits(t)
        assert m["min"] == t.min() and m["max"] == t.max() and m["last"] == t[-1]
    assert m["stamp_out"] == (int(msg["timestamp"][k[0]] * 1e6) if sensor == "robosense" else stamp)
    # the padding bytes of the 32-byte rows are zero
    pad = m["rows"].view(np.uint8).reshape(-1, 32)
    assert not pad[:, 12:16].any() and not pad[:, 21:24].any() and not pad[:, 28:32].any()


@pytest.mark.parametrize("sensor", ["robosense", "livox_mid_360"])
def test_first_surviving_point_rule(sensor):
    """t0 is the stamp of the first point that survives the NaN filter, not of the first message point."""
    raw = small_raw(50)
    stamp = 1_700_000_000_000_000
    msg = synth.driver_message(sensor, raw, stamp)
    msg["timestamp"][0] -= 5.0  # the first message point carries another stamp ...
    msg["x"][0] = np.nan        # ... and does not survive
    m = iu.convert(msg, sensor, False, 1.0, stamp=stamp)
    assert m["n"] == 49 and m["t0"] == msg["timestamp"][1] and m["rows"]["time"][0] == 0.0
    assert iu.bits(m["rows"]["time"]) == iu.bits((msg["timestamp"][1:] - msg["timestamp"][1]).astype(np.float32))
    if sensor == "robosense":
        assert m["stamp_out"] == int(msg["timestamp"][1] * 1e6) != stamp
    d = iu.convert(msg, sensor, True, 1.0, stamp=stamp)  # dense: nothing is dropped, t0 is the first message point's
    assert d["n"] == 50 and d["t0"] == msg["timestamp"][0]


@pytest.mark.parametrize("packed", [False, True])
def test_avia_lines_and_tag_classes(packed):
    lines, tags = np.meshgrid(np.arange(8), np.array([0x00, 0x10, 0x20, 0x30]) | 0x05, indexing="ij")
    raw = small_raw(32)
    msg = synth.driver_message("livox_avia", raw, packed=packed)
    assert msg.dtype.itemsize == (22 if packed else 32)
    msg["line"], msg["tag"] = lines.reshape(-1), tags.reshape(-1)
    m = iu.convert(msg, "livox_avia", True, 1e-9)
    want = [i for i in range(32) if msg["line"][i] < 6 and (msg["tag"][i] & 0x30) in (0x00, 0x10)]
    assert len(want) == 12 and m["index"].tolist() == want and not m["rows"]["ring"].any()
    assert iu.bits(m["rows"]["time"]) == iu.bits((msg["time"][want].astype(np.float64) * 1e-9).astype(np.float32))


def test_ring_wraps_like_uint8():
    raw = small_raw(8)
    raw["ring"] = [0, 255, 256, 257, 300, 511, 512, 65535]
    for sensor in ("velodyne", "robosense", "leishen"):
        m = iu.convert(synth.driver_message(sensor, raw), sensor, True, 1.0, vsn=255)
        assert m["rows"]["ring"].tolist() == [0, 255, 0, 1, 44, 255, 0, 255]


def test_none_row_against_numpy_fast_atan2():
    rng = np.random.default_rng(11)
    n = 20000
    raw = np.zeros(n, dtype=synth.RAW_POINT_DTYPE)
    raw["x"], raw["y"], raw["z"] = rng.uniform(-50, 50, n), rng.uniform(-50, 50, n), rng.uniform(-25, 25, n)
    msg = synth.driver_message("none", raw)
    m = iu.convert(msg, "none")
    k, ring, _ = np_convert(msg, "none", True, 1.0)
    assert 0 < k.size < n and np.array_equal(m["index"], k) and np.array_equal(m["rows"]["ring"], ring)
    assert set(ring.tolist()) == set(range(iu.VSN))
    fa = np.array([iu.model().im_fast_atan2(float(y), float(x)) for y, x in zip(raw["z"][:2000], raw["x"][:2000])], np.float32)
    assert iu.bits(fa) == iu.bits(np_fast_atan2(raw["z"][:2000], raw["x"][:2000]))


# ---- A(y, x) ------------------------------------------------------------------------------------------------------------------
def atan2_inputs():
    rng = np.random.default_rng(2024)
    n = 1_000_000
    y = rng.uniform(-100, 100, n).astype(np.float32).astype(np.float64)
    x = rng.uniform(-100, 100, n).astype(np.float32).astype(np.float64)
    s = 10.0 ** rng.uniform(-30, 30, n // 10)  # ratios over the whole reduction range
    y[: n // 10] *= s
    return y, x


@pytest.mark.parametrize("which", ["model", "product"])
def test_yaw_function_against_numpy(built, which):
    """|A(y, x) - numpy.arctan2(y, x)| <= 1e-12 rad on 10^6 inputs; axes, signed zeros and infinities exactly as IEEE atan2."""
    lib = None if which == "model" else iu.product_shim()
    y, x = atan2_inputs()
    err = np.abs(iu.atan2_many(y, x, lib) - np.arctan2(y, x))
    print("max |A - arctan2| =", err.max())
    assert err.max() <= 1e-12
    z, inf = 0.0, np.inf
    ys = np.array([z, -z, z, -z, 1, -1, 1, -1, z, -z, inf, -inf, inf, -inf, 3, -3, 3, -3, 1e-300, 1e300])
    xs = np.array([1, 1, -1, -1, z, z, -z, -z, z, z, inf, inf, -inf, -inf, inf, inf, -inf, -inf, -1e300, 1e-300])
    got, want = iu.atan2_many(ys, xs, lib), np.arctan2(ys, xs)
    special = ~((ys == 0) & (xs == 0))  # atan2(+-0, +-0): A returns +-0 / +-pi like IEEE, checked below
    assert np.abs(got - want)[special].max() <= 1e-15
    assert np.array_equal(np.signbit(got), np.signbit(want))
    assert np.isnan(iu.atan2_many(np.array([np.nan, 1.0]), np.array([1.0, np.nan]), lib)).all()


def test_product_yaw_equals_model_bit_for_bit(built):
    y, x = atan2_inputs()
    assert iu.bits(iu.atan2_many(y, x, iu.product_shim())) == iu.bits(iu.atan2_many(y, x))


# ---- the step-function scan -------------------------------------------------------------------------------------------------------
def period_cases():
    P = np.float32(0.1)
    rng = np.random.default_rng(9)
    cases = {}
    # two revolutions of 4 rings: the base time wraps, so the period is added; plus equal times (t == last exactly)
    n = 600
    ring = np.tile(np.arange(4), n // 4).astype(np.uint8)
    base = (np.repeat(np.arange(n // 4), 4) * np.float32(0.2 / (n // 4)) % P).astype(np.float32)
    base[100:140] = base[100]
    cases["two_revolutions_equal_times"] = (base, ring, 4)
    # a ring with one point, a ring first seen late, rings >= scan_num, random order
    ring = rng.integers(0, 6, n).astype(np.uint8)
    ring[ring == 2] = 0
    ring[300] = 2                      # a single point of ring 2
    ring[:450][ring[:450] == 3] = 1
    ring[rng.integers(0, n, 40)] = 9   # >= scan_num: skipped
    cases["single_late_invalid"] = (rng.uniform(0, 0.1, n).astype(np.float32), ring, 6)
    # NaN base times and jitter around `last`
    base = np.sort(rng.uniform(0, 0.1, n)).astype(np.float32)
    base[::17] = np.nextafter(base[::17], np.float32(-1))
    base[50], base[51] = np.nan, base[49]
    cases["jitter_nan"] = (base, rng.integers(0, 3, n).astype(np.uint8), 3)
    return cases


@pytest.mark.parametrize("name", list(period_cases()))
@pytest.mark.parametrize("chunk", [1, 7, 64, 10_000])
def test_step_function_scan_equals_sequential_loop(built, name, chunk):
    base, ring, vsn = period_cases()[name]
    n = base.size
    first = np.zeros(n, np.uint8)
    for r in range(vsn):
        w = np.nonzero(ring == r)[0]
        if w.size:
            first[w[0]] = 1
    own = np.full(n, -7.0, np.float32)
    a, b = own.copy(), own.copy()
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    iu.model().im_period_loop(base.ctypes.data_as(fp), ring.ctypes.data_as(bp), first.ctypes.data_as(bp), n, vsn, a.ctypes.data_as(fp))
    iu.product_shim().ip_period_scan(base.ctypes.data_as(fp), ring.ctypes.data_as(bp), first.ctypes.data_as(bp), n, vsn, chunk, b.ctypes.data_as(fp))
    assert iu.bits(a) == iu.bits(b)
    untouched = (first == 1) | (ring >= vsn)
    assert (a[untouched] == -7.0).all() and untouched.any()
    if name == "two_revolutions_equal_times":
        assert (a[~untouched] >= np.float32(0.1)).any()  # the period was added


def test_timeless_model_branches_and_base_time(built):
    """The model's ComputePointOffsetTime on a 1.2-revolution firing-order cloud: all four branches occur, times grow along each ring,
    and the product's base time (yaw, division) equals the model's on every point whose period was not added."""
    raw = iu.firing_scan()
    m = iu.convert(synth.driver_message("velodyne", raw), "velodyne")
    assert m["timeless"] and m["n"] == raw.shape[0]
    br = m["branch"]
    assert {1, 2, 3} <= set((br & 3).tolist()) and (br & 4).any()
    t = m["rows"]["time"]
    for r in range(16):
        assert (np.diff(t[m["rows"]["ring"] == r][1:]) >= 0).all()
    assert 0.11 < t.max() < 0.13
    S = iu.product_shim()
    rows = m["rows"]
    firsts = {int(r): int(np.nonzero(rows["ring"] == r)[0][0]) for r in range(16)}
    for i in list(range(16, 600)) + list(range(raw.shape[0] - 300, raw.shape[0])):
        if br[i] & 4:
            continue
        f = firsts[int(rows["ring"][i])]
        assert np.float32(S.ip_base_time(rows["y"][f], rows["x"][f], rows["y"][i], rows["x"][i])) == t[i]


# ---- C ABI (no GPU needed) ------------------------------------------------------------------------------------------------------
def test_ingest_symbols_exported(built):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fls_ingest.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src)))
    L = _lib.lib()
    assert declared == sorted(_lib.INGEST_SYMBOLS)
    for s in _lib.INGEST_SYMBOLS:
        assert hasattr(L, s), s
    assert L.fls_ingest_revision() == 1 and "#define FLS_INGEST_REVISION 1" in src and L.fls_abi_revision() == 9


def test_ingest_struct_layouts(built, tmp_path):
    structs = {"fls_driver_cloud": _lib.DriverCloud, "fls_ingest_params": _lib.IngestParams, "fls_ingest_info": _lib.IngestInfo}
    lines = ['#include "fls_ingest.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {",
             'printf("codes %d %d %d %d\\n", FLS_PRE_CONVERTED, FLS_PRE_CONVERTED_INDEX, FLS_SENSOR_VELODYNE, FLS_SENSOR_NONE);']
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.check_output([exe], text=True).splitlines()
    assert out[0].split()[1:] == [str(_lib.FLS_PRE_CONVERTED), str(_lib.FLS_PRE_CONVERTED_INDEX), "0", "6"]
    got = dict(l.split() for l in out[1:])
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)


def test_default_layouts_equal_the_pcl_structs(built):
    L = _lib.lib()
    for name, sid in synth.SENSORS.items():
        d = _lib.DriverCloud()
        assert L.fls_ingest_default_layout(sid, C.byref(d)) == _lib.FLS_OK
        want = preprocess.driver_cloud(synth.DRIVER_DTYPES[name], sid, True)
        assert bytes(d) == bytes(want), name
    assert L.fls_ingest_default_layout(7, C.byref(d)) == _lib.FLS_ERR_INVALID and L.fls_ingest_default_layout(-1, C.byref(d)) == _lib.FLS_ERR_INVALID
    assert L.fls_ingest_default_layout(0, None) == _lib.FLS_ERR_INVALID


def _call(L, h, msg, dc, ip, t, q):
    res = _lib.PreprocessResult()
    res.struct_size = C.sizeof(_lib.PreprocessResult)
    return L.fls_preprocess_scan_driver(h, msg.ctypes.data, msg.shape[0], C.byref(dc), C.byref(ip), 1_000_000, t.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        q.ctypes.data_as(C.POINTER(C.c_double)), t.shape[0], 0, C.byref(res), None, None)


def invalid_cases():
    """(name, sensor, mutation of (descriptor, params))"""
    def setf(obj, field, v):
        return lambda dc, ip: setattr(dc if obj == "dc" else ip, field, v)
    cases = [("cloud_struct_size", "velodyne", setf("dc", "struct_size", 44)), ("params_struct_size", "velodyne", setf("ip", "struct_size", 16)),
             ("sensor_high", "velodyne", setf("dc", "sensor", 7)), ("sensor_negative", "velodyne", setf("dc", "sensor", -1)),
             ("scale_nan", "ouster", setf("ip", "lidar_point_time_scale", float("nan"))), ("scale_inf", "ouster", setf("ip", "lidar_point_time_scale", float("inf"))),
             ("vsn_zero_velodyne", "velodyne", setf("ip", "vertical_scan_num", 0)), ("vsn_256_velodyne", "velodyne", setf("ip", "vertical_scan_num", 256)),
             ("vsn_zero_none", "none", setf("ip", "vertical_scan_num", 0)), ("vsn_256_none", "none", setf("ip", "vertical_scan_num", 256)),
             ("x_past_step", "none", setf("dc", "x_offset", 29)), ("z_past_step", "ouster", setf("dc", "z_offset", 46)),
             ("intensity_past_step", "leishen", setf("dc", "intensity_offset", 30)), ("ring16_past_step", "velodyne", setf("dc", "ring_offset", 31)),
             ("ring8_past_step", "ouster", setf("dc", "ring_offset", 48)), ("time32_past_step", "livox_avia", setf("dc", "time_offset", 29)),
             ("time64_past_step", "robosense", setf("dc", "time_offset", 25)), ("time64_past_step_mid", "livox_mid_360", setf("dc", "time_offset", 28)),
             ("tag_past_step", "livox_avia", setf("dc", "tag_offset", 32)), ("line_past_step", "livox_avia", setf("dc", "line_offset", 40)),
             ("zero_step", "none", setf("dc", "point_step", 0))]
    return cases


@pytest.mark.parametrize("case", invalid_cases(), ids=[c[0] for c in invalid_cases()])
def test_invalid_descriptor_and_parameters(built, case):
    """Every FLS_ERR_INVALID case of the header.  Without a device no handle can exist: the NULL-handle call is FLS_ERR_INVALID and
    the validation itself is exercised where a GPU is present (the same cases run in tests/test_gpu_ingest.py on a live handle)."""
    L = _lib.lib()
    name, sensor, mutate = case
    msg = synth.driver_message(sensor, small_raw(10))
    dc = preprocess.driver_cloud(msg.dtype, synth.SENSORS[sensor])
    ip = preprocess.ingest_params(synth.DRIVER_TIME_SCALE[sensor], 16, iu.LOWER, iu.VRES)
    mutate(dc, ip)
    t, q = np.arange(2, dtype=np.uint64) * 10_000_000, np.tile([0.0, 0, 0, 1], (2, 1))
    assert _call(L, None, msg, dc, ip, t, q) == _lib.FLS_ERR_INVALID
    if L.fls_device_count() >= 1:
        pre = preprocess.ScanPreprocessor(1.0, 100.0)
        assert _call(L, pre._h, msg, dc, ip, t, q) == _lib.FLS_ERR_INVALID
        mutate_back = preprocess.driver_cloud(msg.dtype, synth.SENSORS[sensor])
        good = preprocess.ingest_params(synth.DRIVER_TIME_SCALE[sensor], 16, iu.LOWER, iu.VRES)
        assert _call(L, pre._h, msg, mutate_back, good, t, q) in (_lib.FLS_OK, _lib.FLS_ERR_STATE)
        pre.close()


def test_null_arguments_and_no_device(built):
    L = _lib.lib()
    msg = synth.driver_message("velodyne", small_raw(10))
    dc = preprocess.driver_cloud(msg.dtype, 0)
    ip = preprocess.ingest_params(1.0, 16)
    assert L.fls_preprocess_scan_driver(None, None, 0, C.byref(dc), C.byref(ip), 0, None, None, 0, 0, None, None, None) == _lib.FLS_ERR_INVALID
    assert L.fls_features_project_driver(None, None, 0, C.byref(dc), C.byref(ip), 0, None, None, 0, None, None, None, None, None) == _lib.FLS_ERR_INVALID
    if L.fls_device_count() == 0:  # no CPU fallback: no handle can be made, so no conversion can run
        h = C.c_void_p()
        p = _lib.PreprocessParams(C.sizeof(_lib.PreprocessParams), 1, 1.0, 100.0, 0.5, 0.0, (C.c_double * 16)(*np.eye(4).reshape(-1)))
        assert L.fls_preprocess_create(C.byref(p), 0, C.byref(h)) == _lib.FLS_ERR_DEVICE and not h.value


def test_ingest_adapter_smoke_builds_and_links(built, tmp_path):
    exe = str(tmp_path / "ingest_adapter_smoke")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "stubs", "preprocess"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "stubs", "ingest_smoke.cpp"), "-o", exe,
                           "-L" + libdir, "-lfls_reg", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "ingest adapter ok" in out.stdout, out.stdout + out.stderr
