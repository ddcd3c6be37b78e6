"""Throughput of the fused batch (include/fls_batch.h) against fls_match_batch on BASELINE configs[0] shapes: 64 full-size IcpOptimized jobs
(synth.make_config(0, job=j): 16 x 900 scans, localization mode) from the identity against one resident 50k-point map.

Variants, alternating within one process (a round = every variant once, in a rotating order):
  "batch_lanes8" / "batch_lanes16"   MatchBatch(lanes=8 / 16): one lane clone, stream and host thread per job in flight, launches per job
  "fused_slots8" / "fused_slots16"   MatchBatchFused(slots=8 / 16): one icp_knn_fit_jobs_kernel launch per iteration for a group of 8 / 16 jobs
Per round and variant: the wall clock of the whole call -> jobs per second.  Reported: median, p25, p75 per variant, the counters of
fls_batch_stat of the fused variants (per call), whether every variant returned the same poses / iteration counts, and the bar of the issue that
asked for the fused form: fused p25 above the better fls_match_batch variant's p75.

--kind ivox: the shared-launch batch of the iVox point-to-plane kind (include/fls_batch_ivox.h) instead: 64 BASELINE configs[1] jobs
(synth.make_config(1, job=j): 64 x 1800 planar scans, 1e6-point map) at full size, and again with every scan cut to about 9.8 k points (the
planar cloud the pipeline feeds).  Variants "batch_lanes8" / "batch_lanes16" as above against "shared_slots8" / "shared_slots16" =
MatchBatchSharedIvox(slots=8 / 16); per size the same figures, the counters of fls_batch_ivox_stat per call (launches per call = kNN + fit
launches) and whether the shared form's p25 lies above the better fls_match_batch variant's p75.  Writes profiles/batch_ivox_perf.json.

usage: python tools/gpu_batch_fused_perf.py [--kind icp|ivox] [--jobs 64] [--warmup 3] [--rounds 20] [--json profiles/batch_fused_perf.json]"""
import argparse
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
    return {"median_jobs_per_s": round(float(med), 1), "p25_jobs_per_s": round(float(q1), 1), "p75_jobs_per_s": round(float(q3), 1), "n": int(v.size)}


IVOX_STATS = ("knn_launches", "fit_launches", "jobs_shared", "jobs_outside", "groups")


def measure_ivox(m, reg, scans, a):
    """one size of the --kind ivox run: the four variants alternating over warmup + rounds rounds"""
    n = len(scans)
    clusters = [reg.PointcloudCluster(planar_cloud_=s) for s in scans]
    T0 = [np.eye(4)] * n
    variants = {"batch_lanes8": lambda: m.MatchBatch(clusters, T0, lanes=8), "batch_lanes16": lambda: m.MatchBatch(clusters, T0, lanes=16),
                "shared_slots8": lambda: m.MatchBatchSharedIvox(clusters, T0, slots=8), "shared_slots16": lambda: m.MatchBatchSharedIvox(clusters, T0, slots=16)}
    names = list(variants)
    rate = {k: [] for k in names}
    counters, result = {}, {}
    for rnd in range(a.warmup + a.rounds):
        order = names[rnd % len(names):] + names[:rnd % len(names)]
        for k in order:
            before = [m.BatchIvoxStat(s) for s in range(5)]
            t = time.perf_counter()
            oks, Ts, st = variants[k]()
            dt = time.perf_counter() - t
            if rnd >= a.warmup:
                rate[k].append(n / dt)
            if k.startswith("shared"):
                counters[k] = dict(zip(IVOX_STATS, [m.BatchIvoxStat(s) - b for s, b in enumerate(before)]))
                counters[k]["launches_per_call"] = counters[k]["knn_launches"] + counters[k]["fit_launches"]
            row = (tuple(oks), np.ascontiguousarray(Ts).tobytes(), tuple(s.iterations for s in st), tuple(s.n_valid for s in st))
            result.setdefault(k, row)
            assert result[k] == row, f"{k}: a repeated call returned something else"
    its = result[names[0]][2]
    out = {"points_per_scan": int(scans[0].shape[0]), "iterations_per_job": {"min": int(min(its)), "max": int(max(its)), "sum": int(sum(its))},
           # fls_match_batch: two launches per iteration of every job
           "batch_launches_per_call": 2 * int(sum(its)),
           "variants": {k: stats(rate[k]) for k in names}, "shared_counters_per_call": counters,
           "all_variants_bit_identical": all(result[k] == result[names[0]] for k in names)}
    best_batch = max(("batch_lanes8", "batch_lanes16"), key=lambda k: out["variants"][k]["median_jobs_per_s"])
    best_shared = max(("shared_slots8", "shared_slots16"), key=lambda k: out["variants"][k]["median_jobs_per_s"])
    out["best_batch"], out["best_shared"] = best_batch, best_shared
    out["ratio_shared_over_batch_median"] = round(out["variants"][best_shared]["median_jobs_per_s"] / out["variants"][best_batch]["median_jobs_per_s"], 3)
    out["shared_p25_above_batch_p75"] = bool(out["variants"][best_shared]["p25_jobs_per_s"] > out["variants"][best_batch]["p75_jobs_per_s"])
    return out


def main_ivox(a):
    from funny_lidar_slam_amd import registration as reg, synth

    cfg0 = synth.make_config(1, job=0)
    scans = [cfg0["scan"]] + [synth.make_config(1, job=j, with_map=False)["scan"] for j in range(1, a.jobs)]
    m = reg.make_matcher("PointToPlane_IVOX", reg.YAML_NCLT_IVOX)
    m.AddCloudToLocalMap([cfg0["map"]])
    step = max(1, int(round(scans[0].shape[0] / 9800.0)))  # (every step-th point: the rings stay, the azimuth thins)
    out = {"tool": "gpu_batch_fused_perf --kind ivox", "jobs": a.jobs, "rounds": a.rounds, "warmup": a.warmup,
           "full_size": measure_ivox(m, reg, scans, a), "pipeline_size": measure_ivox(m, reg, [s[::step].copy() for s in scans], a)}
    m.close()
    print(json.dumps(out, indent=1))
    path = a.json or os.path.join(ROOT, "profiles", "batch_ivox_perf.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=("icp", "ivox"), default="icp")
    ap.add_argument("--jobs", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.kind == "ivox":
        return main_ivox(a)
    a.json = a.json or os.path.join(ROOT, "profiles", "batch_fused_perf.json")
    from funny_lidar_slam_amd import registration as reg, synth

    cfg0 = synth.make_config(0, job=0)
    scans = [cfg0["scan"]] + [synth.make_config(0, job=j, with_map=False)["scan"] for j in range(1, a.jobs)]
    clusters = [reg.PointcloudCluster(ordered_cloud_=s) for s in scans]
    T0 = [np.eye(4)] * a.jobs
    m = reg.make_matcher("IcpOptimized", reg.YAML_NCLT_ICP, is_localization_mode=True)
    m.AddCloudToLocalMap([cfg0["map"]])

    variants = {"batch_lanes8": lambda: m.MatchBatch(clusters, T0, lanes=8), "batch_lanes16": lambda: m.MatchBatch(clusters, T0, lanes=16),
                "fused_slots8": lambda: m.MatchBatchFused(clusters, T0, slots=8), "fused_slots16": lambda: m.MatchBatchFused(clusters, T0, slots=16)}
    names = list(variants)
    rate = {k: [] for k in names}
    counters, result = {}, {}
    for rnd in range(a.warmup + a.rounds):
        order = names[rnd % len(names):] + names[:rnd % len(names)]
        for k in order:
            before = [m.BatchStat(s) for s in range(4)]
            t = time.perf_counter()
            oks, Ts, st = variants[k]()
            dt = time.perf_counter() - t
            if rnd >= a.warmup:
                rate[k].append(a.jobs / dt)
            if k.startswith("fused"):
                counters[k] = dict(zip(("shared_launches", "jobs_shared", "jobs_per_lane", "groups"), [m.BatchStat(s) - b for s, b in enumerate(before)]))
            row = (tuple(oks), np.ascontiguousarray(Ts).tobytes(), tuple(s.iterations for s in st), tuple(s.n_valid for s in st))
            result.setdefault(k, row)
            assert result[k] == row, f"{k}: a repeated call returned something else"
    out = {"tool": "gpu_batch_fused_perf", "jobs": a.jobs, "rounds": a.rounds, "warmup": a.warmup,
           "iterations_per_job": {"min": int(min(result[names[0]][2])), "max": int(max(result[names[0]][2])), "sum": int(sum(result[names[0]][2]))},
           "variants": {k: stats(rate[k]) for k in names}, "fused_counters_per_call": counters,
           "all_variants_bit_identical": all(result[k] == result[names[0]] for k in names)}
    best_batch = max(("batch_lanes8", "batch_lanes16"), key=lambda k: out["variants"][k]["median_jobs_per_s"])
    best_fused = max(("fused_slots8", "fused_slots16"), key=lambda k: out["variants"][k]["median_jobs_per_s"])
    out["best_batch"], out["best_fused"] = best_batch, best_fused
    out["ratio_fused_over_batch_median"] = round(out["variants"][best_fused]["median_jobs_per_s"] / out["variants"][best_batch]["median_jobs_per_s"], 3)
    out["fused_p25_above_batch_p75"] = bool(out["variants"][best_fused]["p25_jobs_per_s"] > out["variants"][best_batch]["p75_jobs_per_s"])
    m.close()
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
