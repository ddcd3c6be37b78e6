"""What a localization reload costs from "the pose needs a new local map" to "the matcher holds it": the parent commit's way -- the caller
has the already-cropped cloud on the host and calls fls_add_cloud_to_local_map (the host crop itself is NOT counted, which favours that side)
-- against the device local-map source (include/fls_localmap.h): fls_localmap_crop + fls_add_localmap_to_local_map, and
fls_localmap_load_tiles + the add.  PointToPlane_IVOX and IncrementalNDT localization handles.

Three crops: the 1,000,000-point maps of BASELINE configs[1] and configs[2], each the crop result out of a global map four times larger (the
map and three copies of it 250 m away), and a 100,000-point cut (the same construction on the points nearest the origin).  One tile walk:
the four-copy configs[1] map split into 100 m tiles, the pose alternating between two places 150 m apart so that every call changes the
resident set (leaf 0.4).  A = host cloud + fls_add_cloud_to_local_map, B = the device source; A and B alternate in one process over
warmup + rounds rounds, timed with a host clock around the whole call(s) (every call returns with its streams idle).  Reported: median, p25,
p75 in ms, the ratio of the medians, and the bar "B's p75 below A's p25".

--label NAME --only-a: time A alone (e.g. with FLS_REG_LIB naming the parent commit's library; its cloud is cropped with numpy) and store
it under NAME in the same json.

usage: python tools/gpu_localmap_perf.py [--warmup 3] [--rounds 20] [--json profiles/localmap_perf.json] [--only-a --label parent_lib]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = {"ivox": "PointToPlane_IVOX", "ndt": "IncrementalNDT"}
SHIFTS = ((0.0, 0.0), (250.0, 0.0), (0.0, 250.0), (250.0, 250.0))


def q(v):
    v = np.asarray(v, dtype=np.float64) * 1e3
    q1, med, q3 = np.percentile(v, [25, 50, 75])
    return {"median_ms": round(float(med), 3), "p25_ms": round(float(q1), 3), "p75_ms": round(float(q3), 3), "n": int(v.size)}


def four_copies(cloud):
    rows = np.zeros((4 * len(cloud), 4), np.float32)
    for k, (dx, dy) in enumerate(SHIFTS):
        part = rows[k * len(cloud):(k + 1) * len(cloud)]
        part[:, :3] = cloud[:, :3]
        part[:, 0] += np.float32(dx)
        part[:, 1] += np.float32(dy)
    rows[:, 3] = np.arange(len(rows)) % 256
    return rows[np.random.default_rng(1).permutation(len(rows))]  # a map file is not sorted by copy


def numpy_crop(rows, t):
    mn, mx = (np.asarray(t) - 100.0).astype(np.float32), (np.asarray(t) + 100.0).astype(np.float32)
    return np.ascontiguousarray(rows[~((rows[:, :3] < mn).any(1) | (rows[:, :3] > mx).any(1))])


def numpy_tiles(rows, g, t, leaf, reg):
    """the stitched local map of a fresh resident set at t: VoxelGridCloud of the 3 x 3 tiles around it, in (gx, gy) order"""
    gx = np.floor((rows[:, 0].astype(np.float64) - g / 2) / g).astype(np.int64)
    gy = np.floor((rows[:, 1].astype(np.float64) - g / 2) / g).astype(np.int64)
    cx, cy = int(np.floor((t[0] - g / 2) / g)), int(np.floor((t[1] - g / 2) / g))
    parts = []
    for a in range(cx - 1, cx + 2):
        for b in range(cy - 1, cy + 2):
            tile = rows[(gx == a) & (gy == b)]
            if len(tile):
                parts.append(reg.VoxelGridCloud(tile, leaf, on_device=False))
    return np.ascontiguousarray(np.concatenate(parts))


def pose(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def measure(reg, kind, host_clouds, device_step, warmup, rounds, only_a):
    """host_clouds[i % len]: what A adds in round i; device_step(i): B's store call of round i (returns the points of its local map)"""
    sides = ("A",) if only_a else ("A", "B")
    held = {s: reg.make_matcher(KINDS[kind], reg.YAML_NCLT_IVOX if kind == "ivox" else reg.YAML_NCLT_NDT, is_localization_mode=True) for s in sides}
    times = {s: [] for s in sides}
    n_b = 0
    for rnd in range(warmup + rounds):
        for s in (sides if rnd % 2 == 0 else tuple(reversed(sides))):
            m = held[s]
            t0 = time.perf_counter()
            if s == "A":
                m.AddCloudToLocalMap([host_clouds[rnd % len(host_clouds)]])
            else:
                n_b = device_step(rnd, m)
            t1 = time.perf_counter()
            if rnd >= warmup:
                times[s].append(t1 - t0)
    out = {s: dict(q(times[s]), map_points=int(held[s].map_size())) for s in sides}
    if not only_a:
        out["B"]["local_map_points"] = int(n_b)
        out["same_map_size"] = bool(held["A"].map_size() == held["B"].map_size())
        out["ratio_of_medians_A_over_B"] = round(out["A"]["median_ms"] / out["B"]["median_ms"], 2)
        out["separated_B_p75_below_A_p25"] = bool(out["B"]["p75_ms"] < out["A"]["p25_ms"])
    for m in held.values():
        m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "localmap_perf.json"))
    ap.add_argument("--only-a", action="store_true")
    ap.add_argument("--label", default="this_build")
    a = ap.parse_args()
    from funny_lidar_slam_amd import _lib, registration as reg, synth
    assert _lib.device_count() >= 1, "needs an MI355X"
    LocalMapSource = None
    if not a.only_a:
        from funny_lidar_slam_amd.localmap import LocalMapSource
    maps = {"configs1_map_1000000": synth.make_config(1, scale=1.0)["map"], "configs2_map_1000000": synth.make_config(2, scale=1.0)["map"]}
    full = maps["configs1_map_1000000"]
    near = np.argsort(np.einsum("ij,ij->i", full[:, :2], full[:, :2]), kind="stable")[:100000]
    maps["cut_100000"] = np.ascontiguousarray(full[np.sort(near)])
    doc = {}
    if os.path.exists(a.json):
        with open(a.json) as f:
            doc = json.load(f)
    run = {"warmup": a.warmup, "rounds": a.rounds, "library": os.environ.get("FLS_REG_LIB", "libfls_reg.so"), "crop": {}, "tile_walk": {}}
    origin = np.array([0.37, -0.21, 0.11])
    for name, cloud in maps.items():
        rows = four_copies(cloud)
        host = numpy_crop(rows, origin)
        src = None
        if not a.only_a:
            src = LocalMapSource()
            src.SetGlobal(rows)
            assert src.Crop(pose(origin), force=True) == (True, len(host)) and np.array_equal(src.Local(), host)

        def device_step(rnd, m, src=src):
            n = src.Crop(pose(origin), force=True)[1]  # every round cuts anew, as a reload does
            src.AddTo(m)
            return n
        run["crop"][name] = {"global_points": int(len(rows)), "local_points": int(len(host))}
        for kind in KINDS:
            r = measure(reg, kind, [host], device_step, a.warmup, a.rounds, a.only_a)
            if src is not None:
                r["store"] = src.stats()
            run["crop"][name][kind] = r
            print(name, kind, json.dumps(r), flush=True)
        if src is not None:
            src.close()
    # the tile walk
    rows = four_copies(maps["configs1_map_1000000"])
    g, leaf = 100.0, 0.4
    places = [np.array([20.0, 10.0, 0.1]), np.array([170.0, 10.0, 0.1])]
    host = [numpy_tiles(rows, g, t, leaf, reg) for t in places]
    src = None
    if not a.only_a:
        src = LocalMapSource()
        src.SetGlobal(rows)
        src.Split(g)

    def tile_step(rnd, m, src=src):
        src.Reset()  # a fresh resident set, as A's clouds are: the tiles' filtered forms come from the cache after the first visit
        upd, n = src.LoadTiles(pose(places[rnd % 2]), leaf)
        assert upd and n == len(host[rnd % 2])
        src.AddTo(m)
        return n
    run["tile_walk"] = {"global_points": int(len(rows)), "grid_size": g, "leaf": leaf, "local_points": [int(len(h)) for h in host]}
    for kind in KINDS:
        r = measure(reg, kind, host, tile_step, a.warmup, a.rounds, a.only_a)
        if src is not None:
            r["store"] = src.stats()
        run["tile_walk"][kind] = r
        print("tile_walk", kind, json.dumps(r), flush=True)
    if src is not None:
        src.close()
    doc[a.label] = run
    os.makedirs(os.path.dirname(a.json), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.json)


if __name__ == "__main__":
    main()
