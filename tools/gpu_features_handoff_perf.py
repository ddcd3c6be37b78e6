"""What a LoamFull frame costs from the raw driver cloud to the pose, with the feature clouds visiting the host and without.

One full-size BASELINE configs[3] frame (64 x 1800 Velodyne scan) against the configs[3] map, leaves 0.2 / 0.4 (config_nclt_loam_full.yaml).
    host-cloud path : project, extract, fetch the two filtered clouds, fls_match                          (the default mode)
    device path     : keep_on_device, project, extract, fls_scan_attach_features, fls_match_resident       (include/fls_features_device.h)
Both paths alternate in one process over warmup + rounds rounds, update_map = 0, timed with a host clock around the whole frame (every call
returns with its streams idle).  Reported: median, p25, p75 in ms of the whole frame and of the extract call alone on both paths, the
filtered cloud sizes, the ratio of the medians and the bar "the device path's p75 below the host path's p25".  The poses of the two paths
must be bit-equal or the tool fails.

--parent-lib PATH: the host-cloud path of that library (the parent commit's build) timed in a child process of this tool, same frame, same
rounds; reported beside the bar "this library's host-path median inside the parent's p25-p75" (the default mode must not have become slower).
This library's host-cloud path is timed alone in child processes of its own as well: --pairs pairs of processes alternate (parent / this /
parent / this ...), every process's median is reported, and the frames of all processes of a library are pooled, because the medians of
two processes of ONE library differ by more than a single process's quartile range.

usage: python tools/gpu_features_handoff_perf.py [--warmup 5] [--rounds 20] [--parent-lib parent.so] [--pairs 6] [--json profiles/features_handoff_perf.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def q(v):
    v = np.asarray(v, dtype=np.float64) * 1e3
    q1, med, q3 = np.percentile(v, [25, 50, 75])
    return {"median_ms": round(float(med), 3), "p25_ms": round(float(q1), 3), "p75_ms": round(float(q3), 3), "n": int(v.size)}


def run(a):
    from funny_lidar_slam_amd import _lib, features, registration as reg, synth
    cfg = synth.make_config(3)
    scene = synth.make_scene()
    raw = synth.cast_raw_scan(scene, cfg["T_gt"], rng=synth.rng_for(3, 0, 77), max_range=cfg["radius"], **synth.VELODYNE_64)
    h_res = float(np.float32(0.2 / 180.0 * np.pi))
    mk = lambda keep: features.FeatureFrontEnd(1800, 64, h_res, 4.0, 100.0, 1.0, 0.1, 0.2, 0.4, keep_on_device=keep) if keep else \
        features.FeatureFrontEnd(1800, 64, h_res, 4.0, 100.0, 1.0, 0.1, 0.2, 0.4)
    m = reg.make_matcher("LoamFull_KdTree", reg.YAML_NCLT_LOAM_FULL)
    m.AddCloudToLocalMap([cfg["map"], cfg["corner_map"]])
    host = mk(False)
    dev = None if a.only_host else mk(True)
    T0 = np.asarray(cfg["T_init"], dtype=np.float64)
    times = {"host_frame": [], "host_extract": [], "device_frame": [], "device_extract": []}
    poses, sizes = {}, {}

    def host_frame():
        t0 = time.perf_counter()
        host.project(raw)
        t1 = time.perf_counter()
        host.extract()
        t2 = time.perf_counter()
        pl, co = host.get("planar_filtered"), host.get("corner_filtered")
        T = T0.copy()
        m.Match(reg.PointcloudCluster(planar_cloud_=pl, corner_cloud_=co), T, update_map=False)
        t3 = time.perf_counter()
        sizes["host"] = (len(pl), len(co))
        poses["host"] = T
        return t3 - t0, t2 - t1

    def device_frame():
        t0 = time.perf_counter()
        dev.project(raw)
        t1 = time.perf_counter()
        dev.extract()
        t2 = time.perf_counter()
        rc = dev.attach_to(m)
        if rc != _lib.FLS_OK:
            raise _lib.FlsError(rc, "fls_scan_attach_features")
        T = T0.copy()
        m.MatchResident(T, update_map=False)
        t3 = time.perf_counter()
        poses["device"] = T
        return t3 - t0, t2 - t1

    for r in range(a.warmup + a.rounds):
        f, e = host_frame()
        if r >= a.warmup:
            times["host_frame"].append(f)
            times["host_extract"].append(e)
        if dev is not None:
            f, e = device_frame()
            if r >= a.warmup:
                times["device_frame"].append(f)
                times["device_extract"].append(e)
    out = {"library": os.path.basename(os.environ.get("FLS_REG_LIB", "libfls_reg.so")), "warmup": a.warmup, "rounds": a.rounds, "raw_points": int(raw.shape[0]),
           "filtered_planar": sizes["host"][0], "filtered_corner": sizes["host"][1], "iterations": int(m.stats.iterations),
           "host_path": {"frame": q(times["host_frame"]), "extract": q(times["host_extract"])}}
    if a.only_host:  # (the parent process pools the frames of several child processes)
        out["host_path"]["frame_samples_ms"] = [round(1e3 * t, 4) for t in times["host_frame"]]
        out["host_path"]["extract_samples_ms"] = [round(1e3 * t, 4) for t in times["host_extract"]]
    if dev is not None:
        if not np.array_equal(poses["host"].view(np.uint64), poses["device"].view(np.uint64)):
            raise SystemExit("the two paths disagree on the pose")
        out["device_path"] = {"frame": q(times["device_frame"]), "extract": q(times["device_extract"]), "host_bytes_per_frame": dev.host_bytes(), "stat": dev.stat()}
        h, d = out["host_path"]["frame"], out["device_path"]["frame"]
        out["ratio_of_medians_host_over_device"] = round(h["median_ms"] / d["median_ms"], 3)
        out["device_p75_below_host_p25"] = bool(d["p75_ms"] < h["p25_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--pairs", type=int, default=6, help="pairs of child processes (parent library / this library) of --parent-lib")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "features_handoff_perf.json"))
    ap.add_argument("--only-host", action="store_true", help="(the child process of --parent-lib) the host-cloud path alone, the result on stdout")
    a = ap.parse_args()
    if a.only_host:
        print("RESULT " + json.dumps(run(a)))
        return
    out = run(a)
    if a.parent_lib:
        def child(env):
            c = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-host", "--warmup", str(a.warmup), "--rounds", str(a.rounds)], env=env,
                               capture_output=True, text=True, timeout=900)
            if c.returncode != 0:
                raise SystemExit("a child run failed:\n" + c.stdout + c.stderr)
            line = [l for l in c.stdout.splitlines() if l.startswith("RESULT ")][-1]
            return json.loads(line[len("RESULT "):])["host_path"]
        # The parent's host path runs alone in its process; this library's host path is timed the same way beside it (in the alternating run above
        # the device path's launches and allocations sit between two host frames): --pairs pairs of processes, parent / this / parent / this ...
        # One process's quartile range is narrower than the spread between processes, so the comparison that counts is the pooled one: every
        # frame of every parent process against every frame of every process of this library.
        penv = dict(os.environ, FLS_REG_LIB=os.path.abspath(a.parent_lib))
        parent, mine = [], []
        for k in range(a.pairs):  # parent / this, this / parent, ...: neither library always runs behind the other
            if k % 2 == 0:
                parent.append(child(penv))
                mine.append(child(dict(os.environ)))
            else:
                mine.append(child(dict(os.environ)))
                parent.append(child(penv))
        pool = lambda runs, key: np.concatenate([np.asarray(r[key + "_samples_ms"]) for r in runs]) * 1e-3
        strip = lambda r: {k: v for k, v in r.items() if not k.endswith("_samples_ms")}
        out["parent_host_path_processes"] = [strip(r) for r in parent]
        out["host_path_alone_processes"] = [strip(r) for r in mine]
        out["parent_host_path_pooled"] = {"frame": q(pool(parent, "frame")), "extract": q(pool(parent, "extract"))}
        out["host_path_alone_pooled"] = {"frame": q(pool(mine, "frame")), "extract": q(pool(mine, "extract"))}
        med = lambda runs: [r["frame"]["median_ms"] for r in runs]
        out["process_medians_ms"] = {"parent": med(parent), "this": med(mine)}
        p1, pp = parent[0]["frame"], out["parent_host_path_pooled"]["frame"]
        out["host_median_inside_first_parent_process_p25_p75"] = bool(p1["p25_ms"] <= out["host_path"]["frame"]["median_ms"] <= p1["p75_ms"])
        out["host_alone_pooled_median_inside_parent_pooled_p25_p75"] = bool(pp["p25_ms"] <= out["host_path_alone_pooled"]["frame"]["median_ms"] <= pp["p75_ms"])
        out["host_alone_pooled_median_not_above_parent_pooled_p75"] = bool(out["host_path_alone_pooled"]["frame"]["median_ms"] <= pp["p75_ms"])
    os.makedirs(os.path.dirname(a.json), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
