"""Timing of the device keyframe store (include/fls_keyframes.h) on the loop-closure workload of config/mapping/config_nclt.yaml:61-63:
72 keyframes of 115,200 points (Velodyne-64 scans of the synthetic scene; 12 distinct scans, each stored six times), assembled into the
candidate's sub-map of 41 keyframes and the loop-closure keyframe's of 31, leaf 0.2 m, no final filter (LoopClosure::GetSubMap).

Per call = both sub-maps, wall clock, rows on the host at the end; the legs alternate within one process:
  "parent_route"   what the library offered before the store: per keyframe fls_voxel_grid_cloud(DEVICE) from host rows, a float32 host
                   transform (numpy) and a concatenation
  "merge_cold"     fls_keyframes_merge on a store that has filtered nothing yet (72 device filters run; a fresh store per call, filled
                   outside the timed window)
  "merge_warm"     fls_keyframes_merge with every filtered cloud cached, new poses in every call
and, from the hipEvents around the launch (stat slot 7), the merge kernel's own time and its rate by algorithmic bytes (16 B read +
16 B written per point) against the 8 TB/s HBM peak.  "loop_match": fls_keyframes_loop_match against parent_route + fls_loop_match
(few repetitions: one LoopClosure::Match on sub-maps of this size takes seconds).

usage: python tools/gpu_keyframes_perf.py [--calls N] [--loop-reps N] [--json profiles/keyframes_perf.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
N_TGT, N_SRC, LEAF = 41, 31, 0.2


def stats(v, unit="ms"):
    v = np.asarray(v, dtype=np.float64)
    q1, med, q3 = np.percentile(v, [25, 50, 75])
    return {f"median_{unit}": round(float(med), 4), f"iqr_{unit}": round(float(q3 - q1), 4), f"p25_{unit}": round(float(q1), 4),
            f"p75_{unit}": round(float(q3), 4), "n": int(v.size)}


def xform(cloud, T):
    R, t = T[:3, :3].astype(np.float32), T[:3, 3].astype(np.float32)
    x, y, z = cloud[:, 0], cloud[:, 1], cloud[:, 2]
    out = np.empty((cloud.shape[0], 4), np.float32)
    for r in range(3):
        out[:, r] = (R[r, 0] * x + (R[r, 1] * y + R[r, 2] * z)) + t[r]
    out[:, 3] = cloud[:, 3]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=2)
    ap.add_argument("--scans", type=int, default=12)
    ap.add_argument("--n-az", type=int, default=1800)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "keyframes_perf.json"))
    a = ap.parse_args()
    from funny_lidar_slam_amd import _lib, keyframes, registration as reg, synth

    scene = synth.make_scene()
    rng = synth.rng_for(11, 1)
    base = []
    for k in range(a.scans):
        T = np.eye(4)
        T[0, 3] = 1.0 * k
        s = synth.cast_scan(scene, T, rng=rng, **dict(synth.VELODYNE_64, n_az=a.n_az))
        base.append(np.ascontiguousarray(np.concatenate([s, rng.uniform(0, 255, (s.shape[0], 1)).astype(np.float32)], axis=1)))
    clouds = [base[k % a.scans] for k in range(N_TGT + N_SRC)]
    tgt_ids, src_ids = np.arange(N_TGT, dtype=np.int32), np.arange(N_TGT, N_TGT + N_SRC, dtype=np.int32)

    def poses(ids, seed):  # where the scan was cast, jittered: new values in every call
        r = np.random.default_rng(seed)
        P = np.tile(np.eye(4), (len(ids), 1, 1))
        for k, i in enumerate(ids):
            P[k, :3, :3] = synth.so3_exp(r.normal(size=3) * 0.01)
            P[k, :3, 3] = [1.0 * (i % a.scans) + r.normal() * 0.05, r.normal() * 0.05, r.normal() * 0.01]
        return P

    def fill():
        s = keyframes.KeyframeStore()
        for c in clouds:
            s.add(c)
        return s

    def parent_route(ids, P):
        return np.concatenate([xform(reg.VoxelGridCloud(clouds[i], LEAF, on_device=True), P[k]) for k, i in enumerate(ids)])

    def both(f, seed):
        t0 = time.perf_counter()
        x, y = f(tgt_ids, poses(tgt_ids, seed)), f(src_ids, poses(src_ids, seed + 1))
        return (time.perf_counter() - t0) * 1e3, x, y

    if _lib.device_count() < 1:
        raise SystemExit("no gfx950 device: nothing is measured without one")
    warm = fill()
    kernel_ns, kernel_pts = [], []

    def merged(store):
        def f(ids, P):
            out = store.merge(ids, P, LEAF, 0.0)
            if store is warm:
                kernel_ns.append(store.stats()["last_merge_ns"])
                kernel_pts.append(out.shape[0])
            return out
        return f

    # warm-up: code objects, the filters' buffers, the cache of `warm`; and the legs agree bit for bit
    _, x0, y0 = both(parent_route, 0)
    _, x1, y1 = both(merged(warm), 0)
    identical = bool(np.array_equal(x0.view(np.uint32), x1.view(np.uint32)) and np.array_equal(y0.view(np.uint32), y1.view(np.uint32)))
    kernel_ns.clear(); kernel_pts.clear()
    t_parent, t_cold, t_warm = [], [], []
    for c in range(a.calls):
        cold = fill()
        t_parent.append(both(parent_route, 10 + 2 * c)[0])
        t_cold.append(both(merged(cold), 10 + 2 * c)[0])
        t_warm.append(both(merged(warm), 10 + 2 * c)[0])
        assert cold.stats()["filters_run"] == N_TGT + N_SRC and cold.stats()["filters_declined"] == 0
        cold.close()
    ns, pts = np.asarray(kernel_ns, np.float64), np.asarray(kernel_pts, np.float64)
    rate = 32.0 * pts / (ns * 1e-9)
    out = {"tool": "gpu_keyframes_perf", "calls": a.calls, "keyframes": N_TGT + N_SRC, "points_per_keyframe": int(clouds[0].shape[0]),
           "submaps": [N_TGT, N_SRC], "leaf_each": LEAF, "submap_points": [int(x1.shape[0]), int(y1.shape[0])],
           "legs_bit_identical": identical,
           "parent_route": stats(t_parent), "merge_cold": stats(t_cold), "merge_warm": stats(t_warm),
           "ratio_warm_over_parent": round(float(np.median(t_warm) / np.median(t_parent)), 4),
           "ratio_cold_over_parent": round(float(np.median(t_cold) / np.median(t_parent)), 4),
           "merge_kernel": dict(stats(ns * 1e-3, "us"), points_median=int(np.median(pts)),
                                algorithmic_bytes_per_point=32, bytes_per_s_median=float(f"{np.median(rate):.4g}"),
                                share_of_hbm_peak_8TBps=round(float(np.median(rate) / HBM_PEAK), 4)),
           "resident_bytes": warm.stats()["bytes_resident"]}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)

    write()  # (the loop-match leg below takes the longest: what is measured so far is kept)
    t_a, t_b, loop_same = [], [], True
    for r in range(a.loop_reps):
        Pt, Ps = poses(tgt_ids, 1000 + r), poses(src_ids, 2000 + r)
        t0 = time.perf_counter()
        tgt, src = parent_route(tgt_ids, Pt), parent_route(src_ids, Ps)
        T1 = np.eye(4)
        f1, _ = reg.LoopClosureMatch(src, tgt, T1)
        t_a.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        T2 = np.eye(4)
        f2, _ = warm.loop_match(src_ids, Ps, tgt_ids, Pt, T2)
        t_b.append((time.perf_counter() - t0) * 1e3)
        loop_same = loop_same and f1 == f2 and bool(np.array_equal(T1, T2))
    if a.loop_reps:
        out["loop_match"] = {"parent_route_plus_fls_loop_match": stats(t_a), "fls_keyframes_loop_match": stats(t_b), "results_bit_identical": loop_same}
    write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
