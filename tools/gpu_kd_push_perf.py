"""What a keyframe costs the kd-tree kinds with the push into the device deque on the device (csrc/kernels_kd_push.hpp, the default) and through
the host (FLS_KD_DEVICE_PUSH=0: download of the matched scan, host transform, upload, one more wait).  The keyframe update is timed as bench.py
defines it (bench_kd_mapping_mode, ms_keyframe_update_only): the same scan from host buffers through Match(update_map=False) and then
Match(update_map=True), every frame beyond the keyframe gate, the deque pre-filled to production size; the update is the difference.

  icp_configs0_full_deque      IcpOptimized, configs[0] scans (VELODYNE_16, 14,400 points), deque of 50 full
  loam_full_configs3           LoamFull, configs[3] scans (57,600 planar + 7,680 corner points), deques of 25
  p2plane_kd_configs1_scan     LoamPointToPlaneKdtree in mapping mode (local_map_size 20, gate 1.0 m / 0.2 rad), configs[1]'s scan size (115,200 points)

Two handles, one created with FLS_KD_DEVICE_PUSH=0 and one with the default, alternate in one process (the order is reversed every other
round); both see the same calls.  The deque is pre-filled with copies of the first cloud, as bench.py does; the rounds before the timed ones
(--warmup plus one per deque slot) replace every copy by a real keyframe, so the timed rounds run on a full deque that no longer drifts.  Reported per handle: median, p25 and p75 in ms of the whole Match(update_map=True)
call, of the keyframe update alone and of the Match without a keyframe (which must not move), and the project's separation rule "new p75
below old p25" on the whole call.  --baseline-lib PATH runs the same rounds once more in a child process on another build of the library
(FLS_REG_LIB, e.g. the parent commit's), one default handle: the switch-off handle is the baseline, that run confirms it.

usage: python tools/gpu_kd_push_perf.py [--warmup 3] [--rounds 20] [--baseline-lib PATH] [--json profiles/kd_push_perf.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SWITCH = "FLS_KD_DEVICE_PUSH"


def q(v):
    v = np.asarray(v, dtype=np.float64) * 1e3
    q1, med, q3 = np.percentile(v, [25, 50, 75])
    return {"median_ms": round(float(med), 3), "p25_ms": round(float(q1), 3), "p75_ms": round(float(q3), 3), "n": int(v.size)}


def world(c, T):
    return (c.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def trajectory(synth, cid, n, corner_points=0):
    """n frames 1.2 m / 3 degrees apart (beyond the keyframe gate): (scan, corner scan or None, pose)"""
    cfg = {"scene": synth.make_scene()}
    rng = synth.rng_for(cid, 779)
    lid = synth.VELODYNE_16 if cid == 0 else synth.VELODYNE_64  # (as synth.make_config: configs[0] alone is a 16-ring sensor)
    T, out = np.eye(4), []
    step = np.eye(4)
    step[:3, :3] = synth.so3_exp(np.deg2rad([0.0, 0.0, 3.0]))
    step[:3, 3] = [1.2, 0.1, 0.0]
    for _ in range(n):
        scan = synth.cast_scan(cfg["scene"], T, rng=rng, **lid)
        corner = synth.cast_edge_scan(cfg["scene"], T, corner_points, rng) if corner_points else None
        out.append((scan[::2].copy() if corner_points else scan, corner, T.copy()))
        T = T @ step
    return out


def cases(reg):
    return [("icp_configs0_full_deque", "IcpOptimized", dict(reg.YAML_NCLT_ICP), 0, 49, 0),
            ("loam_full_configs3", "LoamFull_KdTree", dict(reg.YAML_NCLT_LOAM_FULL), 3, 24, 7680),
            ("p2plane_kd_configs1_scan", "PointToPlane_KdTree", dict(reg.YAML_NCLT_LOC_KDTREE, local_map_size=20, keyframe_delta_distance=1.0, keyframe_delta_rotation=0.2), 1, 19, 0)]


def cluster(reg, mode, scan, corner):
    if mode == "IcpOptimized":
        return reg.PointcloudCluster(ordered_cloud_=scan)
    if mode == "LoamFull_KdTree":
        return reg.PointcloudCluster(planar_cloud_=scan, corner_cloud_=corner)
    return reg.PointcloudCluster(planar_cloud_=scan)


def measure(reg, mode, y, frames, prefill, handles, warmup, rounds):
    """handles: {name: value of the switch or None}"""
    ms = {}
    for name, switch in handles.items():
        prev = os.environ.get(SWITCH)
        if switch is not None:
            os.environ[SWITCH] = switch
        ms[name] = reg.make_matcher(mode, y)
        os.environ.pop(SWITCH, None)
        if prev is not None:
            os.environ[SWITCH] = prev
    s0, c0, T0 = frames[0]
    init = [world(s0, T0)] + ([world(c0, T0)] if c0 is not None else [])
    for m in ms.values():
        for _ in range(prefill + 1):
            m.AddCloudToLocalMap(init)
    t = {name: {"match": [], "both": []} for name in ms}
    keyframes = {name: 0 for name in ms}
    same = True
    # the pre-fill is one cloud many times over (the filter merges the copies); every keyframe replaces one copy by a real cloud and the map
    # grows with it.  The warm-up therefore runs until the deque holds keyframes only: the timed rounds see a deque that no longer drifts
    warmup = warmup + prefill + 1
    for rnd in range(warmup + rounds):
        if rnd == warmup:
            for v in t.values():
                v["match"].clear(); v["both"].clear()
        scan, corner, Tk = frames[1 + rnd % (len(frames) - 1)]
        cl = cluster(reg, mode, scan, corner)
        got = {}
        for name in (list(ms) if rnd % 2 == 0 else list(reversed(ms))):
            m = ms[name]
            T = Tk.copy(); t0 = time.perf_counter(); m.Match(cl, T, update_map=False); t[name]["match"].append(time.perf_counter() - t0)
            T = Tk.copy(); t0 = time.perf_counter(); m.Match(cl, T, update_map=True); t[name]["both"].append(time.perf_counter() - t0)
            keyframes[name] += int(m.stats.map_updated)
            got[name] = (T.tobytes(), int(m.stats.iterations), int(m.stats.n_valid), int(m.map_size(0)))
        same = same and len(set(got.values())) == 1
    out = {"scan_points": int(frames[1][0].shape[0]) + (int(frames[1][1].shape[0]) if frames[1][1] is not None else 0), "deque_clouds_at_timing": prefill + 1,
           "handles_agree_bit_for_bit": bool(same)}
    for name, m in ms.items():
        both, match = np.array(t[name]["both"]), np.array(t[name]["match"])
        out[name] = {"match_plus_keyframe_update": q(both), "keyframe_update_only": q(both - match), "match_without_keyframe": q(match),
                     "keyframes": keyframes[name], "rounds_with_warmup": warmup + rounds,
                     "counters_164_165_166_167": [int(m.map_size(s)) for s in (164, 165, 166, 167)], "map_points": int(m.map_size(0))}
        m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--child", action="store_true", help="(internal) one default handle per kind, the result as one JSON line")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "kd_push_perf.json"))
    a = ap.parse_args()
    from funny_lidar_slam_amd import _lib, registration as reg, synth
    assert _lib.device_count() >= 1, "needs an MI355X"
    handles = {"library_default": None} if a.child else {"host_push_switch_off": "0", "device_push_default": None}
    doc = {"warmup": a.warmup, "rounds": a.rounds, "kinds": {}}
    for label, mode, y, cid, prefill, corner_points in cases(reg):
        frames = trajectory(synth, cid, a.frames, corner_points)
        r = measure(reg, mode, y, frames, prefill, handles, a.warmup, a.rounds)
        if not a.child:
            new, old = r["device_push_default"], r["host_push_switch_off"]
            r["device_push_faster_separated_p75_below_p25"] = bool(new["match_plus_keyframe_update"]["p75_ms"] < old["match_plus_keyframe_update"]["p25_ms"])
            r["device_push_slower_separated"] = bool(new["match_plus_keyframe_update"]["p25_ms"] > old["match_plus_keyframe_update"]["p75_ms"])
            r["match_without_keyframe_moved_separated"] = bool(new["match_without_keyframe"]["p25_ms"] > old["match_without_keyframe"]["p75_ms"]
                                                               or new["match_without_keyframe"]["p75_ms"] < old["match_without_keyframe"]["p25_ms"])
        doc["kinds"][label] = r
        print(label, json.dumps(r), file=sys.stderr if a.child else sys.stdout, flush=True)
    if a.child:
        print("CHILD_RESULT " + json.dumps(doc["kinds"]), flush=True)
        return
    if a.baseline_lib:
        env = dict(os.environ, FLS_REG_LIB=os.path.abspath(a.baseline_lib))
        env.pop(SWITCH, None)
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--warmup", str(a.warmup), "--rounds", str(a.rounds), "--frames", str(a.frames)],
                             env=env, capture_output=True, text=True, timeout=900)
        line = [ln for ln in run.stdout.splitlines() if ln.startswith("CHILD_RESULT ")]
        assert run.returncode == 0 and line, run.stdout[-2000:] + run.stderr[-4000:]
        doc["baseline_library_one_default_handle"] = json.loads(line[-1][len("CHILD_RESULT "):])
        print("baseline library", json.dumps(doc["baseline_library_one_default_handle"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.json)


if __name__ == "__main__":
    main()
