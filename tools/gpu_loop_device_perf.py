#!/usr/bin/env python3
"""Wall time of the loop-closure Match started from host sub-maps and from device sub-maps, on one MI355X -> profiles/loop_device_perf.json.

Three legs, all through a KeyframeStore (GetSubMap twice, leaf 0.2, then LoopClosure::Match):
  host          fls_keyframes_loop_match: both sub-maps downloaded, ten exact host filters, host leaf builds (the default)
  host_devvg    the same call in a child process with FLS_DEVICE_VOXELGRID=1: the ten filters on the device, each uploading its input
  device        fls_keyframes_loop_match_device: the sub-maps stay on the device (include/fls_loop_device.h)
`host` and `device` alternate in this process, `host_devvg` and `device` alternate in the child; 20 rounds after one warm-up each; median and
quartiles of the whole call.  The three results are checked equal on bits in the run.  One extra round of each leg runs in a child with
FLS_HOST_TIMING=1 for the stage split the library prints.

Two shapes:
  bench         the pair bench.py's loop_ms leg times, make_pair(job=1, n_az=450, n_t=5, n_s=3): 3 + 5 keyframes of 64 x 450 scans
  submap        a GetSubMap shape: 41 + 41 keyframes of full-size 64 x 1800 scans one metre apart along a path

  python tools/gpu_loop_device_perf.py [--rounds 20] [--shapes bench,submap] [--out profiles/loop_device_perf.json]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from funny_lidar_slam_amd import _lib, keyframes, registration as reg, synth  # noqa: E402

SHAPES = {"bench": dict(job=1, n_az=450, n_t=5, n_s=3), "submap": dict(job=2, n_az=1800, n_t=41, n_s=41)}
T_TRUE_ROT_DEG, T_TRUE_TRANS = (0.5, -0.4, 3.0), (0.8, -0.5, 0.1)  # tests/loopdata.py's displacement


def make_keyframes(job, n_az, n_t, n_s):
    """raw scans in their own frames and the poses that place them: the target around the origin, the source the same path seen from a frame
    displaced by T_true (so that the Match should return ~T_true)"""
    scene = synth.make_scene()
    rng = synth.rng_for(7, job)
    Tt = np.eye(4)
    Tt[:3, :3] = synth.so3_exp(np.deg2rad(np.asarray(T_TRUE_ROT_DEG, float)))
    Tt[:3, 3] = T_TRUE_TRANS
    Ti = np.linalg.inv(Tt)
    scans, poses = [], []
    for n, frame in ((n_t, np.eye(4)), (n_s, Ti)):
        for k in range(n):
            T = np.eye(4)
            T[0, 3] = (k - n // 2) * 1.0
            scans.append(synth.cast_scan(scene, T, rng=rng, **dict(synth.VELODYNE_64, n_az=n_az)).astype(np.float32)[:, :3])
            poses.append(frame @ T)
    return scans, np.asarray(poses), n_t, Tt


def save_shape(path, scans, poses, n_t, Tt):
    np.savez(path, poses=poses, n_t=n_t, Tt=Tt, sizes=np.asarray([len(s) for s in scans]), points=np.concatenate(scans))


def load_store(path):
    z = np.load(path)
    cuts = np.cumsum(z["sizes"])[:-1]
    store = keyframes.KeyframeStore()
    ids = [store.add(np.ascontiguousarray(s)) for s in np.split(z["points"], cuts)]
    n_t = int(z["n_t"])
    return store, (ids[n_t:], z["poses"][n_t:]), (ids[:n_t], z["poses"][:n_t]), z["Tt"]


def one(store, src, tgt, on_device):
    T = np.eye(4)
    t0 = time.perf_counter()
    f, st = store.loop_match(src[0], src[1], tgt[0], tgt[1], T, on_device=on_device)
    ms = (time.perf_counter() - t0) * 1e3
    digest = hashlib.sha256(T.tobytes() + np.float32(f).tobytes() + bytes(st)).hexdigest()[:16]
    return ms, digest, T, st


def quartiles(ms):
    a = np.sort(np.asarray(ms))
    return {"p25": round(float(np.percentile(a, 25)), 3), "median": round(float(np.median(a)), 3), "p75": round(float(np.percentile(a, 75)), 3),
            "min": round(float(a[0]), 3), "max": round(float(a[-1]), 3)}


def alternate(path, rounds, first_name):
    """(first leg = fls_keyframes_loop_match under this process's environment, `device` leg) alternating"""
    store, src, tgt, Tt = load_store(path)
    legs = {first_name: False, "device": True}
    out = {k: {"ms": [], "digest": None} for k in legs}
    for k, dev in legs.items():  # warm-up: allocations, the keyframes' cached 0.2 m filters
        _, out[k]["digest"], T, st = one(store, src, tgt, dev)
    et, er = synth.pose_error(T, Tt)
    info = {"pose_error_m_rad": [float(et), float(er)], "gicp_source_points": int(st.gicp_source_points), "gicp_target_points": int(st.gicp_target_points),
            "ndt_source_points": [int(v) for v in st.ndt_source_points], "ndt_target_leaves": [int(v) for v in st.ndt_target_leaves]}
    a = store.merge(src[0], src[1], 0.2, 0.0).shape[0]
    b = store.merge(tgt[0], tgt[1], 0.2, 0.0).shape[0]
    info["submap_points"] = [int(a), int(b)]
    before = reg.loop_device_stats()
    for _ in range(rounds):
        for k, dev in legs.items():
            ms, digest, _, _ = one(store, src, tgt, dev)
            assert digest == out[k]["digest"], (k, "a leg's result changed between rounds")
            out[k]["ms"].append(ms)
    after = reg.loop_device_stats()
    info["device_counters_per_call"] = {k: (after[k] - before[k]) / rounds for k in after}
    store.close()
    return out, info


def child_main(args):
    if args.child == "alternate":
        out, _ = alternate(args.data, args.rounds, "host_devvg")
        print("RESULT " + json.dumps(out))
    else:  # one timed round of one leg: the library prints the stage split on stderr
        store, src, tgt, _ = load_store(args.data)
        dev = args.child == "device"
        one(store, src, tgt, dev)
        sys.stderr.write("[perf] timed round\n")
        one(store, src, tgt, dev)
        store.close()


def stage_split(path, leg):
    env = dict(os.environ, FLS_HOST_TIMING="1")
    if leg == "host_devvg":
        env["FLS_DEVICE_VOXELGRID"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--data", path], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    tail = r.stderr.split("[perf] timed round\n")[-1]
    return [l.strip() for l in tail.splitlines() if l.startswith("[fls loop] ms:")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--shapes", default="bench,submap")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_device_perf.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--data", default=None)
    args = ap.parse_args()
    if args.child:
        return child_main(args)
    if _lib.device_count() < 1:
        raise SystemExit("no gfx950 device")
    result = {"tool": "tools/gpu_loop_device_perf.py", "rounds": args.rounds, "unit": "ms, wall time of the whole call", "shapes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in args.shapes.split(","):
            path = os.path.join(tmp, name + ".npz")
            t0 = time.perf_counter()
            save_shape(path, *make_keyframes(**SHAPES[name]))
            print(f"[{name}] keyframes cast in {time.perf_counter() - t0:.1f} s", flush=True)
            mine, info = alternate(path, args.rounds, "host")
            env = dict(os.environ, FLS_DEVICE_VOXELGRID="1")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "alternate", "--data", path, "--rounds", str(args.rounds)], env=env,
                               capture_output=True, text=True, timeout=1500)
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-2000:])
            theirs = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
            digests = {mine["host"]["digest"], mine["device"]["digest"], theirs["host_devvg"]["digest"], theirs["device"]["digest"]}
            assert len(digests) == 1, ("the legs disagree", digests)
            legs = {"host": quartiles(mine["host"]["ms"]), "host_devvg": quartiles(theirs["host_devvg"]["ms"]), "device": quartiles(mine["device"]["ms"]),
                    "device_in_child": quartiles(theirs["device"]["ms"])}
            shape = dict(SHAPES[name], **info, legs=legs, results_equal=True,
                         device_faster_than_host=legs["device"]["p75"] < legs["host"]["p25"],
                         device_faster_than_host_devvg=legs["device_in_child"]["p75"] < legs["host_devvg"]["p25"],
                         stage_split={leg: stage_split(path, leg) for leg in ("host", "host_devvg", "device")})
            result["shapes"][name] = shape
            print(f"[{name}] " + json.dumps(legs), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
