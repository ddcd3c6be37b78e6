"""What AddCloudToLocalMap costs when the NDT map takes a whole cloud: the first insert of a mapping handle and every reload of a localization
handle (FLS_INCREMENTAL_NDT).  A = FLS_NDT_DEVICE_BUILD=0 (host VoxelGrid, sequential insert + LRU, UpdateVoxel on one thread, image rebuild; a
mapping handle then uploads the mirror to enter device mode: the only path before the device build existed), B = the default
(NdtMatcher::add_cloud_build -> NdtMap::build: device VoxelGrid + the update chain with ndt_upd_voxel_first, kernels_ndt_update.hpp).

Three clouds: the 1,000,000-point map of BASELINE configs[2], a 100,000-point cut of it (the points nearest the origin), one 64 x 1800 scan.
Per cloud and scenario, A and B alternate in one process over warmup + rounds rounds: a localization pair reloads the same two handles (from the
second round on the map is populated), a mapping pair is created afresh every round (a mapping handle takes a whole cloud once; creation is not
timed).  Timed with a host clock: the whole AddCloudToLocalMap call (it returns with the stream idle) and the first Match behind it
(update_map=False: nothing may have been deferred into it).  Reported: median, p25, p75 in ms, the ratio of the medians, and the project's
separation rule "B's p75 below A's p25" -- a gain is claimed only where it holds.

--label NAME --only-a: time A alone (e.g. with FLS_REG_LIB naming the parent commit's library, to show that the host path has not changed) and
store it under NAME in the same json.

usage: python tools/gpu_ndt_build_perf.py [--warmup 3] [--rounds 20] [--json profiles/ndt_build_perf.json] [--only-a --label parent_lib]"""
import argparse
import json
import os
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
    os.environ["FLS_NDT_DEVICE_BUILD"] = "1" if build else "0"  # read when the handle is created
    try:
        return reg.make_matcher("IncrementalNDT", reg.YAML_NCLT_NDT, is_localization_mode=loc)
    finally:
        del os.environ["FLS_NDT_DEVICE_BUILD"]


def clouds_and_scan():
    from funny_lidar_slam_amd import synth
    cfg = synth.make_config(2, scale=1.0)
    full = cfg["map"]
    near = np.argsort(np.einsum("ij,ij->i", full[:, :2], full[:, :2]), kind="stable")[:100000]
    cut = np.ascontiguousarray(full[np.sort(near)])
    scan = np.ascontiguousarray(cfg["scan"])
    return {"map_%d" % len(full): full, "cut_100000": cut, "scan_%d" % len(scan): scan}, scan, cfg["T_init"]


def measure(reg, cloud, scan, T_init, loc, sides, warmup, rounds):
    t_add = {s: [] for s in sides}
    t_match = {s: [] for s in sides}
    result = {}
    held = {s: make(reg, True, s == "B") for s in sides} if loc else {}
    for rnd in range(warmup + rounds):
        order = list(sides) if rnd % 2 == 0 else list(reversed(sides))
        for s in order:
            m = held[s] if loc else make(reg, False, s == "B")
            t0 = time.perf_counter()
            m.AddCloudToLocalMap([cloud])
            t1 = time.perf_counter()
            T = T_init.copy()
            ok = m.Match(reg.PointcloudCluster(ordered_cloud_=scan), T, update_map=False)
            t2 = time.perf_counter()
            if rnd >= warmup:
                t_add[s].append(t1 - t0)
                t_match[s].append(t2 - t1)
            result[s] = (ok, T, m.stats.iterations, m.stats.n_valid, m.map_size(), m.map_size(150), m.map_size(151))
            if not loc:
                m.close()
    for m in held.values():
        m.close()
    out = {s: {"add_cloud": q(t_add[s]), "first_match": q(t_match[s]), "voxels": int(result[s][4])} for s in sides}
    if "B" in out:  # (--only-a may run a library that has no slots 150 / 151)
        for s in sides:
            out[s]["device_builds"], out[s]["declined"] = int(result[s][5]), int(result[s][6])
    if "A" in out and "B" in out:
        ra, rb = result["A"], result["B"]
        out["same_result"] = bool(ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and ra[2:5] == rb[2:5])
        out["ratio_of_medians_A_over_B"] = round(out["A"]["add_cloud"]["median_ms"] / out["B"]["add_cloud"]["median_ms"], 2)
        out["separated_B_p75_below_A_p25"] = bool(out["B"]["add_cloud"]["p75_ms"] < out["A"]["add_cloud"]["p25_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "ndt_build_perf.json"))
    ap.add_argument("--only-a", action="store_true")
    ap.add_argument("--label", default="this_build")
    a = ap.parse_args()
    from funny_lidar_slam_amd import _lib, registration as reg
    assert _lib.device_count() >= 1, "needs an MI355X"
    clouds, scan, T_init = clouds_and_scan()
    sides = ("A",) if a.only_a else ("A", "B")
    doc = {}
    if os.path.exists(a.json):
        with open(a.json) as f:
            doc = json.load(f)
    other = os.environ.get("FLS_REG_LIB")  # (another build's library: only its file name is recorded)
    run = {"warmup": a.warmup, "rounds": a.rounds, "library": "FLS_REG_LIB=" + os.path.basename(other) if other else "libfls_reg.so", "clouds": {}}
    for name, cloud in clouds.items():
        run["clouds"][name] = {}
        for loc in (True, False):
            scenario = "localization_reload" if loc else "mapping_first_insert"
            r = measure(reg, cloud, scan, T_init, loc, sides, a.warmup, a.rounds)
            run["clouds"][name][scenario] = r
            print(name, scenario, json.dumps(r), flush=True)
    doc[a.label] = run
    os.makedirs(os.path.dirname(a.json), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.json)


if __name__ == "__main__":
    main()
