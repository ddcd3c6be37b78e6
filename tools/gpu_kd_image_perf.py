"""What moving the local map of a kd-tree kind costs (FLS_ICP_OPTIMIZED, FLS_LOAM_FULL; include/fls_map_kd.h): the flat image exported on the
device (kd_image_pack_kernel) into a device buffer and into pinned host memory, imported from either (kd_image_unpack_kernel + the kind's own
filter and grid rebuild) and a replica-set refresh with one replica -- beside the only way such a map could be copied before the image existed:
a second handle that is fed the deque's clouds through AddCloudToLocalMap one by one (which does not reproduce the keyframe gate).

Two maps: an IcpOptimized mapping handle that got the BASELINE configs[0] map as its first cloud and then a replay of cast scans, in the world
frame, until its deque of 50 is full, with two Matches at the end so that the gate is set; and a LoamFull handle that got the configs[3] pair of
maps and then eight frames of planar and corner scans (more than 5 clouds: its maps are filtered).  The imports go into one handle per map, round
after round: from its second import on it reuses the planes it unpacked the previous image into.  All operations alternate in one process over
warmup + rounds rounds, in an order that is reversed every other round.  Timed with a host clock, the whole call (every call returns with the
stream idle).  Reported: median, p25, p75 in ms and the project's separation rule "new p75 below old p25" -- a gain is claimed only where it holds.

Also: fls_replicas_match_batch_fused on the device list [0, 0] against fls_match_batch_fused on the owner alone, 64 configs[0] jobs on the
configs[0] map.  On one GPU the expectation is "no loss beyond noise", not a gain.

usage: python tools/gpu_kd_image_perf.py [--warmup 3] [--rounds 20] [--json profiles/kd_image_perf.json]"""
import argparse
import ctypes as C
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


def world(c, T):
    return (c.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def trajectory(synth, cid, n, corner_points=0):
    """n frames 1.2 m / 3 degrees apart (beyond the keyframe gate): (scan, corner scan or None, pose)"""
    cfg = synth.make_config(cid)
    rng = synth.rng_for(cid, 778)
    lid = synth.VELODYNE_16 if cid == 0 else synth.VELODYNE_64
    T, out = np.eye(4), []
    step = np.eye(4)
    step[:3, :3] = synth.so3_exp(np.deg2rad([0.0, 0.0, 3.0]))
    step[:3, 3] = [1.2, 0.1, 0.0]
    for _ in range(n):
        scan = synth.cast_scan(cfg["scene"], T, rng=rng, **lid)
        corner = synth.cast_edge_scan(cfg["scene"], T, corner_points, rng) if corner_points else None
        out.append((scan[::2].copy() if corner_points else scan, corner, T.copy()))
        T = T @ step
    return cfg, out


def build_icp(reg, synth):
    y = dict(reg.YAML_NCLT_ICP)
    cfg, frames = trajectory(synth, 0, 14)
    fed = [cfg["map"]] + [world(frames[k % 12][0], frames[k % 12][2]) for k in range(y["local_map_size"] - 1)]
    matches = [(reg.PointcloudCluster(ordered_cloud_=s), T) for s, _, T in frames[12:]]

    def fresh():
        return reg.make_matcher("IcpOptimized", y)

    def feed(m):
        for c in fed:
            m.AddCloudToLocalMap([c])
    return fresh, feed, matches, [fed[-1]]


def build_loam(reg, synth):
    y = dict(reg.YAML_NCLT_LOAM_FULL)
    cfg, frames = trajectory(synth, 3, 10, corner_points=7680)
    fed = [(cfg["map"], cfg["corner_map"])] + [(world(s, T), world(c, T)) for s, c, T in frames[:8]]
    matches = [(reg.PointcloudCluster(planar_cloud_=s, corner_cloud_=c), T) for s, c, T in frames[8:]]

    def fresh():
        return reg.make_matcher("LoamFull_KdTree", y)

    def feed(m):
        for p, c in fed:
            m.AddCloudToLocalMap([p, c])
    return fresh, feed, matches, list(fed[-1])


def measure(hip, fresh, feed, matches, one_more, warmup, rounds):
    owner, taker = fresh(), fresh()
    feed(owner)
    updated = 0
    for cl, T in matches:  # the gate: the first Match sets it, the second takes a keyframe
        owner.Match(cl, T.copy(), update_map=True)
        updated += int(owner.stats.map_updated)
    n = owner.MapImageBytes()
    dev, pinned = C.c_void_p(), C.c_void_p()
    assert n > 0 and hip.hipMalloc(C.byref(dev), n) == 0 and hip.hipHostMalloc(C.byref(pinned), n, 0) == 0
    owner.ExportMapImage(dev.value, n, True)
    owner.ExportMapImage(pinned.value, n, False)
    rs = owner.Replicas([0, 0])

    def op_export_device():
        t0 = time.perf_counter(); owner.ExportMapImage(dev.value, n, True); return time.perf_counter() - t0

    def op_export_pinned():
        t0 = time.perf_counter(); owner.ExportMapImage(pinned.value, n, False); return time.perf_counter() - t0

    def op_import_device():
        t0 = time.perf_counter(); taker.ImportMapImage(dev.value, n, True); return time.perf_counter() - t0

    def op_import_pinned():
        t0 = time.perf_counter(); taker.ImportMapImage(pinned.value, n, False); return time.perf_counter() - t0

    def op_replica_refresh():
        t0 = time.perf_counter(); rs.Refresh(); return time.perf_counter() - t0

    def op_refeed():
        m = fresh()  # (creation is not timed)
        t0 = time.perf_counter(); feed(m); dt = time.perf_counter() - t0
        sizes["refed"] = [int(m.map_size(0)), int(m.map_size(1))]
        m.close()
        return dt

    def op_keyframe_update():  # for scale: what one more keyframe costs the taker (deque push + filter + grid), undone by the next import
        t0 = time.perf_counter(); taker.AddCloudToLocalMap(one_more); return time.perf_counter() - t0

    sizes = {}
    ops = {"export_to_device_buffer": op_export_device, "export_to_pinned_host": op_export_pinned, "import_from_device_buffer": op_import_device,
           "import_from_pinned_host": op_import_pinned, "replica_set_refresh_one_replica": op_replica_refresh, "second_handle_refed_cloud_by_cloud": op_refeed}
    times = {k: [] for k in list(ops) + ["one_keyframe_update_for_scale"]}
    for rnd in range(warmup + rounds):
        if rnd == warmup:
            for v in times.values():
                v.clear()
        for name in (list(ops) if rnd % 2 == 0 else list(reversed(ops))):
            times[name].append(ops[name]())
            if name == "import_from_device_buffer":
                times["one_keyframe_update_for_scale"].append(op_keyframe_update())
    taker.ImportMapImage(dev.value, n, True)
    out = {k: q(v) for k, v in times.items()}
    out["image_MB"] = round(n / 1e6, 3)
    out["map_points"] = [int(owner.map_size(0)), int(owner.map_size(1))]
    out["keyframes_taken_by_the_closing_matches"] = updated
    out["importer_map_points_equal_the_owners"] = bool([int(taker.map_size(0)), int(taker.map_size(1))] == out["map_points"])
    out["owner_counters_160_161_115_116"] = [int(owner.map_size(s)) for s in (160, 161, 115, 116)]
    out["taker_counters_162_163"] = [int(taker.map_size(s)) for s in (162, 163)]

    def separated(new, old):
        return bool(out[new]["p75_ms"] < out[old]["p25_ms"])
    out["separated_new_p75_below_old_p25"] = {k + " vs second_handle_refed_cloud_by_cloud": separated(k, "second_handle_refed_cloud_by_cloud")
                                              for k in ("import_from_device_buffer", "import_from_pinned_host", "replica_set_refresh_one_replica")}
    rs.close(); owner.close(); taker.close()
    hip.hipFree(dev); hip.hipHostFree(pinned)
    return out


def measure_fused_batch(reg, synth, warmup, rounds, n_jobs=64, slots=8):
    cfg = synth.make_config(0, job=0)
    scans = [cfg["scan"]] + [synth.make_config(0, job=j, with_map=False)["scan"] for j in range(1, n_jobs)]
    clusters = [reg.PointcloudCluster(ordered_cloud_=s) for s in scans]
    T0 = [np.eye(4)] * n_jobs
    m = reg.make_matcher("IcpOptimized", dict(reg.YAML_NCLT_ICP))
    m.AddCloudToLocalMap([cfg["map"]])
    rs = m.Replicas([0, 0])
    times = {"owner_alone_match_batch_fused": [], "replicas_0_0_match_batch_fused": []}
    same = True
    for rnd in range(warmup + rounds):
        if rnd == warmup:
            for v in times.values():
                v.clear()
        order = ("owner", "set") if rnd % 2 == 0 else ("set", "owner")
        got = {}
        for who in order:
            t0 = time.perf_counter()
            r = m.MatchBatchFused(clusters, T0, slots=slots) if who == "owner" else rs.MatchBatchFused(clusters, T0, slots=slots)
            times["owner_alone_match_batch_fused" if who == "owner" else "replicas_0_0_match_batch_fused"].append(time.perf_counter() - t0)
            got[who] = (r[0], r[1].tobytes(), [(s.iterations, s.n_valid) for s in r[2]])
        same = same and got["owner"] == got["set"]
    out = {k: q(v) for k, v in times.items()}
    out["jobs"], out["slots_per_entry"] = n_jobs, slots
    out["same_table"] = bool(same)
    a, b = out["replicas_0_0_match_batch_fused"], out["owner_alone_match_batch_fused"]
    out["set_faster_separated"] = bool(a["p75_ms"] < b["p25_ms"])
    out["set_slower_separated"] = bool(a["p25_ms"] > b["p75_ms"])
    rs.close(); m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "kd_image_perf.json"))
    a = ap.parse_args()
    from funny_lidar_slam_amd import _lib, registration as reg, synth
    assert _lib.device_count() >= 1, "needs an MI355X"
    hip = C.CDLL("libamdhip64.so")  # the runtime libfls_reg.so itself is linked against
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipHostFree.argtypes = [C.c_void_p]
    doc = {"warmup": a.warmup, "rounds": a.rounds, "maps": {}}
    for name, build in (("icp_configs0_deque_of_50", build_icp), ("loam_full_configs3_pair", build_loam)):
        doc["maps"][name] = measure(hip, *build(reg, synth), a.warmup, a.rounds)
        print(name, json.dumps(doc["maps"][name]), flush=True)
    doc["fused_batch_64_jobs"] = measure_fused_batch(reg, synth, a.warmup, a.rounds)
    print("fused_batch_64_jobs", json.dumps(doc["fused_batch_64_jobs"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.json)


if __name__ == "__main__":
    main()
