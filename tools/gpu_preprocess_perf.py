"""Timing of the per-scan preprocessing (include/fls_preprocess.h) on configs[1]-sized raw scans (Velodyne-64, 64 x 1800, ~115k points
with the per-point time) under a 200 Hz IMU trace, config_nclt settings (min / max distance 4 / 100 m, jump span 6, planar leaf 0.5 m).

  * per call, host buffers in and out: median and IQR of fls_preprocess_scan over >= 200 scans (wall clock), and the device times the
    library records ("device_deskew_compaction": the raw cloud's upload + the three de-skew / compaction kernels; the planar VoxelGrid);
  * the CPU comparison: the single-threaded test model (tests/host/deskew_model.cpp: the reference's loop restated, g++ -O2) plus the
    exact host VoxelGrid on the same host.  The reference's own PreProcessing cannot be compiled here (it needs Eigen, PCL and ROS).

Kernel times: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/gpu_preprocess_perf.py --calls 50`.
usage: python tools/gpu_preprocess_perf.py [--calls N] [--json out.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=240)
    ap.add_argument("--cpu-calls", type=int, default=20)
    ap.add_argument("--json", default=None)
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
    if a.json:
        with open(a.json, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
