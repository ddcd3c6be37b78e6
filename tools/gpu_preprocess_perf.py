"""Timing of the per-scan preprocessing (include/fls_preprocess.h) on configs[1]-sized raw scans (Velodyne-64, 64 x 1800, ~115k points
with the per-point time) under a 200 Hz IMU trace, config_nclt settings (min / max distance 4 / 100 m, jump span 6, planar leaf 0.5 m).

  * per call, host buffers in and out: median and IQR of fls_preprocess_scan over >= 200 scans (wall clock), and the device times the
    library records ("device_deskew_compaction": the raw cloud's upload + the three de-skew / compaction kernels; the planar VoxelGrid);
  * the CPU comparison: the single-threaded test model (tests/host/deskew_model.cpp: the reference's loop restated, g++ -O2) plus the
    exact host VoxelGrid on the same host.  The reference's own PreProcessing cannot be compiled here (it needs Eigen, PCL and ROS).

  * raw cloud to pose (--handoff, written to profiles/preprocess_handoff_perf.json): two legs alternating in one process, wall clock around
    the whole sequence, update_map = 0 -- "raw_to_pose_host": fls_preprocess_scan + fls_preprocess_get + fls_match from the fetched cloud;
    "raw_to_pose_device": fls_preprocess_scan_device + fls_scan_attach_preprocessed + fls_match_resident.  For the iVox kind (planar
    filtered cloud, 1e6-point map) and for IncrementalNDT (ordered cloud, ~110k points through the in-Match VoxelGrid).

Kernel times: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/gpu_preprocess_perf.py --calls 50`.
usage: python tools/gpu_preprocess_perf.py [--calls N] [--json out.json] [--handoff [--handoff-json out.json]]"""
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
    return {"median_ms": round(float(med), 4), "iqr_ms": round(float(q3 - q1), 4), "p25_ms": round(float(q1), 4), "p75_ms": round(float(q3), 4),
            "n": int(v.size)}


def handoff_legs(mode, y, cid, which, scans, t, q, calls):
    """Alternating raw-to-pose legs for one kind; each leg has its own matcher (same map) and its own preprocessing handle."""
    from funny_lidar_slam_amd import _lib, preprocess, registration as reg, synth
    from tests import deskew_util as du
    L = _lib.lib()
    cfg = synth.make_config(cid)
    what = preprocess.ARRAYS[which][0]
    lay = preprocess.raw_layout(scans[0].dtype)
    tp, qp = t.ctypes.data_as(C.POINTER(C.c_uint64)), q.ctypes.data_as(C.POINTER(C.c_double))
    fp = C.POINTER(C.c_float)
    rows = np.zeros((max(s.shape[0] for s in scans), 4), np.float32)
    legs = {}
    for leg in ("host", "device"):
        m = reg.make_matcher(mode, y)
        m.AddCloudToLocalMap([cfg["map"]])
        pre = preprocess.ScanPreprocessor(4.0, 100.0, 6, 0.5, du.T_NCLT)
        res = _lib.PreprocessResult()
        res.struct_size = C.sizeof(_lib.PreprocessResult)
        legs[leg] = (m, pre, res, np.zeros(16), _lib.Stats())
    T0 = np.ascontiguousarray(np.eye(4).reshape(-1))

    def run(leg, s):
        m, pre, res, T, st = legs[leg]
        T[:] = T0
        Tp = T.ctypes.data_as(C.POINTER(C.c_double))
        t0 = time.perf_counter()
        if leg == "host":
            rc = L.fls_preprocess_scan(pre._h, s.ctypes.data, s.shape[0], C.byref(lay), du.STAMP_US, tp, qp, t.shape[0], C.byref(res))
            n = L.fls_preprocess_get(pre._h, what, rows.ctypes.data, rows.shape[0])
            rm = L.fls_match(m._h, rows.ctypes.data_as(fp), n, None, 0, 4, Tp, 0, C.byref(st))
        else:
            rc = L.fls_preprocess_scan_device(pre._h, s.ctypes.data, s.shape[0], C.byref(lay), du.STAMP_US, tp, qp, t.shape[0], C.byref(res))
            ra = L.fls_scan_attach_preprocessed(m._h, pre._h, what)
            assert ra == _lib.FLS_OK
            rm = L.fls_match_resident(m._h, Tp, 0, C.byref(st))
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == _lib.FLS_OK and rm >= 0 and res.filter_on_device == 1
        return dt, T.copy(), rm

    for s in scans:  # warm-up of both legs
        for leg in legs:
            run(leg, s)
    wall = {"host": [], "device": []}
    same = True
    for k in range(calls):
        s = scans[k % len(scans)]
        a = run("host", s)
        b = run("device", s)
        wall["host"].append(a[0])
        wall["device"].append(b[0])
        same = same and a[2] == b[2] and a[1].tobytes() == b[1].tobytes()
    out = {"raw_to_pose_host": stats(wall["host"]), "raw_to_pose_device": stats(wall["device"]), "poses_bit_identical": bool(same),
           "cloud": which, "host_bytes_device_leg": legs["device"][1].host_bytes(), "host_bytes_host_leg": legs["host"][1].host_bytes()}
    out["ratio_device_over_host"] = round(out["raw_to_pose_device"]["median_ms"] / out["raw_to_pose_host"]["median_ms"], 4)
    out["device_p75_below_host_p25"] = bool(out["raw_to_pose_device"]["p75_ms"] < out["raw_to_pose_host"]["p25_ms"])
    for m, pre, *_ in legs.values():
        m.close()
        pre.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=240)
    ap.add_argument("--cpu-calls", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--handoff", action="store_true", help="also time the raw-cloud-to-pose legs (host clouds vs device hand-off)")
    ap.add_argument("--handoff-json", default=None)
    a = ap.parse_args()
    from funny_lidar_slam_amd import _lib, preprocess
    from tests import deskew_util as du

    scans = [du.raw_scan(s)[1] for s in range(4)]
    t, q = du.imu_for()
    pre = preprocess.ScanPreprocessor(4.0, 100.0, 6, 0.5, du.T_NCLT)
    L = _lib.lib()
    lay = preprocess.raw_layout(scans[0].dtype)
    tp, qp = t.ctypes.data_as(C.POINTER(C.c_uint64)), q.ctypes.data_as(C.POINTER(C.c_double))
    res = _lib.PreprocessResult()
    res.struct_size = C.sizeof(_lib.PreprocessResult)
    for s in scans:  # warm-up: buffer growth, code objects
        pre.scan(s, du.STAMP_US, t, q)
    wall, dev_deskew, dev_filter = [], [], []
    for k in range(a.calls):
        s = scans[k % len(scans)]
        t0 = time.perf_counter()
        rc = L.fls_preprocess_scan(pre._h, s.ctypes.data, s.shape[0], C.byref(lay), du.STAMP_US, tp, qp, t.shape[0], C.byref(res))
        wall.append((time.perf_counter() - t0) * 1e3)
        assert rc == _lib.FLS_OK and res.imu_status == _lib.FLS_IMU_OK
        d, f = pre.times_ms()
        dev_deskew.append(d)
        dev_filter.append(f)
    cpu_loop, cpu_filter = [], []
    du.model()  # (compiles the model once, outside the timed loop)
    for k in range(a.cpu_calls):
        s = scans[k % len(scans)]
        t0 = time.perf_counter()
        m = du.preprocess(s, du.STAMP_US, t, q, du.T_NCLT, 4.0, 100.0, 6)
        t1 = time.perf_counter()
        pl = np.ascontiguousarray(m["planar"])
        out = np.zeros((pl.shape[0], 4), np.float32)
        n_out = C.c_size_t()
        assert L.fls_voxel_grid_cloud(0, 0, pl.ctypes.data_as(C.POINTER(C.c_float)), pl.shape[0], 4, np.float32(0.5),
                                      out.ctypes.data_as(C.POINTER(C.c_float)), out.shape[0], C.byref(n_out)) == _lib.FLS_OK
        t2 = time.perf_counter()
        cpu_loop.append((t1 - t0) * 1e3)
        cpu_filter.append((t2 - t1) * 1e3)
    r = {"tool": "gpu_preprocess_perf", "n_raw": [int(s.shape[0]) for s in scans], "n_ordered": int(res.n_ordered), "n_planar": int(res.n_planar),
         "n_planar_filtered": int(res.n_planar_filtered), "n_segment": int(res.n_segment), "filter_on_device": int(res.filter_on_device),
         "call_host_buffers": stats(wall), "device_deskew_compaction": stats(dev_deskew), "device_planar_voxelgrid": stats(dev_filter),
         "cpu_model_loop_single_thread": stats(cpu_loop), "cpu_exact_voxelgrid": stats(cpu_filter),
         "cpu_total_median_ms": round(float(np.median(np.asarray(cpu_loop) + np.asarray(cpu_filter))), 4)}
    print(json.dumps(r))
    if a.handoff:
        from funny_lidar_slam_amd import registration as reg
        ref = json.load(open(os.path.join(ROOT, "profiles", "preprocess_perf.json")))["call_host_buffers"]
        lo, hi = ref["p25_ms"] * 0.95, ref["p75_ms"] * 1.05
        h = {"tool": "gpu_preprocess_perf --handoff", "calls": a.calls,
             "ivox": handoff_legs("PointToPlane_IVOX", reg.YAML_NCLT_IVOX, 1, "planar_filtered", scans, t, q, a.calls),
             "ndt": handoff_legs("IncrementalNDT", reg.YAML_NCLT_NDT, 2, "ordered", scans, t, q, a.calls),
             "call_host_buffers": r["call_host_buffers"], "call_host_buffers_reference_band_ms": [round(lo, 4), round(hi, 4)],
             "call_host_buffers_in_band": bool(lo <= r["call_host_buffers"]["median_ms"] <= hi)}
        print(json.dumps(h))
        if a.handoff_json:
            with open(a.handoff_json, "w") as f:
                json.dump(h, f, indent=1)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
