"""Timing of the driver-cloud front end (include/fls_ingest.h): driver message to iVox pose, two routes alternating in one process,
wall clock around the whole sequence, update_map = 0, config_nclt settings (min / max distance 4 / 100 m, jump span 6, planar leaf 0.5 m,
1e6-point map).

  (a) "host_convert": ConvertMessageToCloud + ComputePointOffsetTime on the host by the test model's compiled loop
      (tests/host/ingest_model.cpp, g++ -O2, single thread; the reference's own cannot be compiled here, it needs PCL and ROS), then
      fls_preprocess_scan_device + fls_scan_attach_preprocessed + fls_match_resident: the best route without this front end;
  (b) "device_convert": fls_preprocess_scan_driver(keep_on_device = 1) + the same attach and Match.

Messages: a time-less Velodyne-64 message (64 x 1800, ~115k points, every time 0: the NCLT driver) and a non-dense Ouster-128-sized
message (128 x 1024 slots, uint32 ns times, ~4 % of the slots non-finite).  The conversion share is the model loop's own time inside
route (a).  Written to profiles/ingest_perf.json.

usage: python tools/gpu_ingest_perf.py [--calls N] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    q1, med, q3 = np.percentile(v, [25, 50, 75])
    return {"median_ms": round(float(med), 4), "p25_ms": round(float(q1), 4), "p75_ms": round(float(q3), 4), "n": int(v.size)}


def messages():
    """name -> (sensor, [messages], is_dense, vertical_scan_num)"""
    from funny_lidar_slam_amd import synth
    from tests import deskew_util as du
    velo, ouster = [], []
    for s in range(4):
        raw = du.raw_scan(s)[1]
        m = synth.driver_message("velodyne", raw)
        m["time"] = 0.0
        velo.append(m)
        cfg = synth.make_config(1, scale=1.0, with_map=False)
        lid = dict(n_rings=128, n_az=1024, elev0_deg=-22.5, elev_step_deg=0.35)
        r = synth.sweep_distort(synth.cast_raw_scan(cfg["scene"], cfg["T_gt"], rng=np.random.default_rng(700 + s), **lid), du.STAMP_US, du.STAMP_US)
        rng = np.random.default_rng(800 + s)
        ouster.append(synth.punch_nonfinite(synth.driver_message("ouster", r, rng=rng), np.nonzero(rng.uniform(size=r.shape[0]) < 0.04)[0], rng))
    return {"velodyne64_timeless": ("velodyne", velo, True, 64), "ouster128_nondense": ("ouster", ouster, False, 128)}


def routes(sensor, msgs, is_dense, vsn, t, q, calls):
    from funny_lidar_slam_amd import _lib, preprocess, registration as reg, synth
    from tests import deskew_util as du, ingest_util as iu
    L = _lib.lib()
    M = iu.model()
    cfg = synth.make_config(1)
    what = preprocess.ARRAYS["planar_filtered"][0]
    scale = synth.DRIVER_TIME_SCALE[sensor]
    dc = preprocess.driver_cloud(msgs[0].dtype, synth.SENSORS[sensor], is_dense)
    ip = preprocess.ingest_params(scale, vsn)
    off = np.array([dc.x_offset, dc.y_offset, dc.z_offset, dc.intensity_offset, dc.ring_offset, dc.time_offset, dc.tag_offset, dc.line_offset], np.uint32)
    lay = _lib.RawLayout(32, 0, 16, 20, 1, 24)
    tp, qp = t.ctypes.data_as(C.POINTER(C.c_uint64)), q.ctypes.data_as(C.POINTER(C.c_double))
    nmax = max(m.shape[0] for m in msgs)
    rows, idx, info, so = np.zeros(nmax, preprocess.CONVERTED_DTYPE), np.zeros(nmax, np.int32), np.zeros(6), C.c_uint64()
    legs = {}
    for leg in ("host_convert", "device_convert"):
        m = reg.make_matcher("PointToPlane_IVOX", reg.YAML_NCLT_IVOX)
        m.AddCloudToLocalMap([cfg["map"]])
        res = _lib.PreprocessResult()
        res.struct_size = C.sizeof(_lib.PreprocessResult)
        legs[leg] = (m, preprocess.ScanPreprocessor(4.0, 100.0, 6, 0.5, du.T_NCLT), res, np.zeros(16), _lib.Stats())
    T0 = np.ascontiguousarray(np.eye(4).reshape(-1))

    def run(leg, s):
        m, pre, res, T, st = legs[leg]
        T[:] = T0
        Tp = T.ctypes.data_as(C.POINTER(C.c_double))
        conv = 0.0
        t0 = time.perf_counter()
        if leg == "host_convert":
            n = M.im_convert(s.ctypes.data, s.shape[0], dc.sensor, dc.point_step, dc.is_dense, off.ctypes.data_as(C.POINTER(C.c_uint32)), scale, vsn, 0.0, 0.0,
                             du.STAMP_US, rows.ctypes.data, idx.ctypes.data_as(C.POINTER(C.c_int32)), info.ctypes.data_as(C.POINTER(C.c_double)),
                             C.byref(so), None)
            conv = (time.perf_counter() - t0) * 1e3
            rc = L.fls_preprocess_scan_device(pre._h, rows.ctypes.data, n, C.byref(lay), so.value, tp, qp, t.shape[0], C.byref(res))
        else:
            rc = L.fls_preprocess_scan_driver(pre._h, s.ctypes.data, s.shape[0], C.byref(dc), C.byref(ip), du.STAMP_US, tp, qp, t.shape[0], 1, C.byref(res),
                                              None, None)
        ra = L.fls_scan_attach_preprocessed(m._h, pre._h, what)
        rm = L.fls_match_resident(m._h, Tp, 0, C.byref(st))
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == _lib.FLS_OK and ra == _lib.FLS_OK and rm >= 0 and res.imu_status == _lib.FLS_IMU_OK and res.filter_on_device == 1
        return dt, T.copy(), rm, conv, int(res.n_raw)

    for s in msgs:  # warm-up of both routes: buffer growth, code objects
        for leg in legs:
            run(leg, s)
    wall = {k: [] for k in legs}
    conv, same, n_conv = [], True, 0
    for k in range(calls):
        s = msgs[k % len(msgs)]
        a = run("host_convert", s)
        b = run("device_convert", s)
        wall["host_convert"].append(a[0])
        wall["device_convert"].append(b[0])
        conv.append(a[3])
        same = same and a[2] == b[2] and a[1].tobytes() == b[1].tobytes() and a[4] == b[4]
        n_conv = b[4]
    out = {"n_message": [int(m.shape[0]) for m in msgs], "n_converted_last": n_conv, "host_convert": stats(wall["host_convert"]),
           "device_convert": stats(wall["device_convert"]), "host_conversion_alone": stats(conv), "poses_bit_identical": bool(same),
           "host_bytes_device_route": legs["device_convert"][1].host_bytes()}
    out["conversion_share_of_host_route"] = round(out["host_conversion_alone"]["median_ms"] / out["host_convert"]["median_ms"], 4)
    out["ratio_device_over_host"] = round(out["device_convert"]["median_ms"] / out["host_convert"]["median_ms"], 4)
    out["device_p75_below_host_p25"] = bool(out["device_convert"]["p75_ms"] < out["host_convert"]["p25_ms"])
    for m, pre, *_ in legs.values():
        m.close()
        pre.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=240)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from tests import deskew_util as du
    t, q = du.imu_for(after_us=300_000)
    r = {"tool": "gpu_ingest_perf", "calls": a.calls}
    for name, (sensor, msgs, dense, vsn) in messages().items():
        r[name] = routes(sensor, msgs, dense, vsn, t, q, a.calls)
    print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
