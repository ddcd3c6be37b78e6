"""What the reference neighbour order (include/fls_knn_order.h) costs: BASELINE configs[1] at full size (1,000,000-point iVox map, 115,200-point
scan), a default-order handle and a reference-order handle alternating in one process, `rounds` rounds after `warmup`.  Per handle: median and
quartiles of the whole Match (host clock around Match(..., update_map=False) from host buffers) and of the kNN launch alone (the dispatch events of
fls_set_profiling: kernel time per launch, averaged over the launches of one Match).  Also recorded: iterations, n_valid, whether the two poses
agree to 1e-4 m / 1e-4 rad, rows whose list differs as a set / in order, and the mode's counters (fls_map_size 177 / 178).

usage: python tools/gpu_knn_order_perf.py [--warmup 3] [--rounds 20] [--json profiles/knn_order_perf.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def q(v, scale, unit):
    v = np.asarray(v, dtype=np.float64) * scale
    q1, med, q3 = np.percentile(v, [25, 50, 75])
    return {f"median_{unit}": round(float(med), 3), f"p25_{unit}": round(float(q1), 3), f"p75_{unit}": round(float(q3), 3), "n": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "knn_order_perf.json"))
    a = ap.parse_args()
    from funny_lidar_slam_amd import _lib, registration as reg, synth
    assert _lib.device_count() >= 1, "needs an MI355X"
    cfg = synth.make_config(1, scale=1.0)
    cl = reg.PointcloudCluster(planar_cloud_=cfg["scan"])
    sides = ("default", "reference")
    hs = {}
    for s in sides:
        m = reg.make_matcher("PointToPlane_IVOX", reg.YAML_NCLT_IVOX)
        m.SetKnnOrder(s)
        m.AddCloudToLocalMap([cfg["map"]])
        m.set_profiling(True)
        hs[s] = m
    t_match = {s: [] for s in sides}
    t_knn = {s: [] for s in sides}
    last = {}
    for rnd in range(a.warmup + a.rounds):
        for s in (sides if rnd % 2 == 0 else tuple(reversed(sides))):
            m = hs[s]
            T = cfg["T_init"].copy()
            t0 = time.perf_counter()
            ok = m.Match(cl, T, update_map=False)
            t1 = time.perf_counter()
            ms, launches, _ = m.kernel_time()
            if rnd >= a.warmup:
                t_match[s].append(t1 - t0)
                t_knn[s].append(ms / max(1, launches))
            last[s] = (ok, T, int(m.stats.iterations), int(m.stats.n_valid), int(launches))
    out = {"config": "BASELINE configs[1], full size", "map_points": int(cfg["map"].shape[0]), "scan_points": int(cfg["scan"].shape[0]),
           "warmup": a.warmup, "rounds": a.rounds, "limit_w": _lib.knn_order_limit()}
    for s in sides:
        ok, T, it, nv, launches = last[s]
        out[s] = {"match": q(t_match[s], 1e3, "ms"), "knn_launch": q(t_knn[s], 1e3, "us"), "ok": bool(ok), "iterations": it, "n_valid": nv,
                  "knn_launches_of_a_match": launches}
    out["reference"]["reference_order_launches_slot_177"] = hs["reference"].map_size(177)
    out["reference"]["fallback_queries_slot_178"] = hs["reference"].map_size(178)
    out["ratio_of_medians_match"] = round(out["reference"]["match"]["median_ms"] / out["default"]["match"]["median_ms"], 2)
    out["ratio_of_medians_knn_launch"] = round(out["reference"]["knn_launch"]["median_us"] / out["default"]["knn_launch"]["median_us"], 2)
    dt, dr = synth.pose_error(last["default"][1], last["reference"][1])
    out["poses_agree_1e-4"] = bool(dt < 1e-4 and dr < 1e-4)
    ids_d, cnt_d, _ = hs["default"].correspondences()
    ids_r, cnt_r, _ = hs["reference"].correspondences()
    out["rows_with_another_set"] = int((np.sort(ids_d, 1) != np.sort(ids_r, 1)).any(1).sum())
    out["rows_in_another_order"] = int((ids_d != ids_r).any(1).sum())
    for m in hs.values():
        m.close()
    print(json.dumps(out, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.json)


if __name__ == "__main__":
    main()
