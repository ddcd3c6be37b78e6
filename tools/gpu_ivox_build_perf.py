"""What AddCloudToLocalMap costs when the iVox map starts from nothing: the first insert of a mapping handle and every reload of a
localization handle (FLS_P2PLANE_IVOX).  A = FLS_IVOX_DEVICE_BUILD=0 (sequential host insert + full flatten + upload, the only path before
the device build existed), B = the default (IvoxMap::bulk_build, kernels_ivox_build.hpp).

Three clouds: the 1,000,000-point map of BASELINE configs[1], a 100,000-point cut of it (the points nearest the origin), the 10,000-point
planar scan the pipeline feeds.  Per cloud and mode, A and B alternate in one process over warmup + rounds rounds: a localization pair reloads
the same two handles, a mapping pair is created afresh every round (a mapping handle takes a whole cloud once; creation is not timed).  Timed
with a host clock: the AddCloudToLocalMap call (it returns with the stream idle), the first Match behind it (update_map=False: nothing may have
been deferred into it), and on B the first ExportMap (the lazy mirror's price).  Reported: median, p25, p75 in ms, the ratio of the medians, and
the bar "B's p75 below A's p25".  The FLS_HOST_TIMING phase lines of one call per path come from a child process (--phases).

--label NAME --only-a: time A alone (e.g. with FLS_REG_LIB naming the parent commit's library, to show that A has not changed) and store it
under NAME in the same json.

usage: python tools/gpu_ivox_build_perf.py [--warmup 3] [--rounds 20] [--json profiles/ivox_build_perf.json] [--only-a --label parent_lib]"""
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


def make(reg, loc, build):
    os.environ["FLS_IVOX_DEVICE_BUILD"] = "1" if build else "0"  # read when the handle is created
    try:
        return reg.make_matcher("PointToPlane_IVOX", reg.YAML_NCLT_IVOX, is_localization_mode=loc)
    finally:
        del os.environ["FLS_IVOX_DEVICE_BUILD"]


def clouds_and_scan():
    from funny_lidar_slam_amd import synth
    cfg = synth.make_config(1, scale=1.0)
    full = cfg["map"]
    near = np.argsort(np.einsum("ij,ij->i", full[:, :2], full[:, :2]), kind="stable")[:100000]
    cut = np.ascontiguousarray(full[np.sort(near)])
    scan = cfg["scan"]
    planar = np.ascontiguousarray(scan[:: max(1, len(scan) // 10000)][:10000])
    return {"map_1000000": full, "cut_100000": cut, "planar_scan_10000": planar}, planar, cfg["T_init"]


def measure(reg, cloud, scan, T_init, loc, sides, warmup, rounds):
    t_add = {s: [] for s in sides}
    t_match = {s: [] for s in sides}
    t_export, result = [], {}
    held = {s: make(reg, True, s == "B") for s in sides} if loc else {}
    for rnd in range(warmup + rounds):
        order = list(sides) if rnd % 2 == 0 else list(reversed(sides))
        for s in order:
            m = held[s] if loc else make(reg, False, s == "B")
            t0 = time.perf_counter()
            m.AddCloudToLocalMap([cloud])
            t1 = time.perf_counter()
            T = T_init.copy()
            ok = m.Match(reg.PointcloudCluster(planar_cloud_=scan), T, update_map=False)
            t2 = time.perf_counter()
            if rnd >= warmup:
                t_add[s].append(t1 - t0)
                t_match[s].append(t2 - t1)
            result[s] = (ok, T, m.stats.iterations, m.stats.n_valid, m.map_size(), m.map_size(102), m.map_size(140), m.map_size(141))
            if s == "B" and rnd >= warmup and rnd % 4 == 0:
                t3 = time.perf_counter()
                m.ExportMap()
                t_export.append(time.perf_counter() - t3)
            if not loc:
                m.close()
    for m in held.values():
        m.close()
    out = {s: {"add_cloud": q(t_add[s]), "first_match": q(t_match[s]), "points": int(result[s][4]), "voxels": int(result[s][5]),
               "device_builds": int(result[s][6]), "declined": int(result[s][7])} for s in sides}
    if "B" not in out:  # (--only-a may run a library that has no slots 140 / 141)
        for s in sides:
            del out[s]["device_builds"], out[s]["declined"]
    if "A" in out and "B" in out:
        ra, rb = result["A"], result["B"]
        out["same_result"] = bool(ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and ra[2:6] == rb[2:6])
        out["ratio_of_medians_A_over_B"] = round(out["A"]["add_cloud"]["median_ms"] / out["B"]["add_cloud"]["median_ms"], 2)
        out["separated_B_p75_below_A_p25"] = bool(out["B"]["add_cloud"]["p75_ms"] < out["A"]["add_cloud"]["p25_ms"])
        out["B_first_export"] = q(t_export)
    return out


def phases_child(name, loc, build):
    """one AddCloudToLocalMap with FLS_HOST_TIMING=1 in a child process: its [fls host] lines"""
    env = dict(os.environ, FLS_HOST_TIMING="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--phases", name, "--loc", str(int(loc)), "--build", str(int(build))],
                       capture_output=True, text=True, env=env, timeout=600)
    return [ln.strip() for ln in r.stderr.splitlines() if ln.startswith("[fls host]")][-4:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "ivox_build_perf.json"))
    ap.add_argument("--only-a", action="store_true")
    ap.add_argument("--label", default="this_build")
    ap.add_argument("--phases", default=None)
    ap.add_argument("--loc", type=int, default=0)
    ap.add_argument("--build", type=int, default=1)
    a = ap.parse_args()
    from funny_lidar_slam_amd import _lib, registration as reg
    assert _lib.device_count() >= 1, "needs an MI355X"
    clouds, scan, T_init = clouds_and_scan()
    if a.phases:  # child: two calls (the second one is warm), the lines go to stderr
        m = make(reg, bool(a.loc), bool(a.build))
        m.AddCloudToLocalMap([clouds[a.phases]])
        if a.loc:
            sys.stderr.write("---- warm ----\n")
            sys.stderr.flush()
            m.AddCloudToLocalMap([clouds[a.phases]])
        m.close()
        return
    sides = ("A",) if a.only_a else ("A", "B")
    doc = {}
    if os.path.exists(a.json):
        with open(a.json) as f:
            doc = json.load(f)
    run = {"warmup": a.warmup, "rounds": a.rounds, "library": os.environ.get("FLS_REG_LIB", "libfls_reg.so"), "clouds": {}}
    for name, cloud in clouds.items():
        run["clouds"][name] = {}
        for loc in (True, False):
            mode = "localization_reload" if loc else "mapping_first_insert"
            r = measure(reg, cloud, scan, T_init, loc, sides, a.warmup, a.rounds)
            if not a.only_a:
                r["host_timing_A"] = phases_child(name, loc, False)
                r["host_timing_B"] = phases_child(name, loc, True)
            run["clouds"][name][mode] = r
            print(name, mode, json.dumps({k: v for k, v in r.items() if not k.startswith("host_timing")}), flush=True)
    doc[a.label] = run
    os.makedirs(os.path.dirname(a.json), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.json)


if __name__ == "__main__":
    main()
