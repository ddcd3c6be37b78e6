"""What checkpointing and resuming an iVox map costs (FLS_P2PLANE_IVOX): the FLSIVOX1 blob packed from and built into the device image
(include/fls_map_ivox.h: fls_ivox_map_export / _import, kernels_ivox_blob.hpp) beside fls_map_export / fls_map_import on the same handles, which
go through the host mirror (to_mirror, load_mirror + a full re-flatten).  The new calls on handles created with FLS_IVOX_DEVICE_IMAGE=0 run
alongside: they take the host writer and fls_map_import's path, so they show that path unchanged.

Two maps: the 1,000,000-point map of BASELINE configs[1] and its 100,000-point cut (the points nearest the origin).  Two kinds of exporter per
map: a mapping handle built on the device and updated by three Match(update_map=True) scans, and a localization handle.  The repeated imports
go into one handle per path, round after round (from its second import on a handle reuses its buffers); a handle's FIRST import, which
allocates them, is measured apart on a fresh handle per round.  All operations alternate in one process over warmup + rounds rounds, in an
order that is reversed every other round.  Timed with a host clock, the whole call (every call returns with the stream idle).  Also timed:
the first Match (update_map=False) after each kind of import -- nothing may have been deferred into it -- and the first fls_map_export after an
import built on the device, which pays for the mirror.  Reported: median, p25, p75 in ms and the project's separation rule "new p75 below old
p25" -- a gain is claimed only where it holds.

usage: python tools/gpu_ivox_blob_perf.py [--warmup 3] [--rounds 20] [--json profiles/ivox_blob_perf.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODE = "PointToPlane_IVOX"


def q(v):
    v = np.asarray(v, dtype=np.float64) * 1e3
    q1, med, q3 = np.percentile(v, [25, 50, 75])
    return {"median_ms": round(float(med), 3), "p25_ms": round(float(q1), 3), "p75_ms": round(float(q3), 3), "n": int(v.size)}


def maps_and_scan():
    from funny_lidar_slam_amd import synth
    cfg = synth.make_config(1, scale=1.0)
    full = cfg["map"]
    near = np.argsort(np.einsum("ij,ij->i", full[:, :2], full[:, :2]), kind="stable")[:100000]
    cut = np.ascontiguousarray(full[np.sort(near)])
    return {"map_%d" % len(full): full, "cut_100000": cut}, np.ascontiguousarray(cfg["scan"]), cfg["T_init"]


def timed(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def measure(reg, lib, hip, cloud, scan, T_init, loc, warmup, rounds):
    def fresh(off=False):
        if off:
            os.environ["FLS_IVOX_DEVICE_IMAGE"] = "0"
        m = reg.make_matcher(MODE, reg.YAML_NCLT_IVOX, is_localization_mode=loc)
        os.environ.pop("FLS_IVOX_DEVICE_IMAGE", None)
        return m
    cl = reg.PointcloudCluster(planar_cloud_=scan)
    # (one exporter per path: fls_map_export builds the mirror, and a localization handle then keeps its map on the host)
    owner, owner_old, owner_off = fresh(), fresh(), fresh(off=True)
    for m in (owner, owner_old, owner_off):
        m.AddCloudToLocalMap([cloud])
        for _ in range(0 if loc else 3):
            T = T_init.copy()
            m.Match(cl, T, update_map=True)
    n = owner.MapBlobBytes()
    assert n == owner_off.MapBlobBytes()
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), n) == 0
    host, host_old = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    owner.ExportMapBlob(dev.value, n, True)
    owner.ExportMapBlob(host.ctypes.data, n, False)
    assert lib.fls_map_export(owner_old._h, host_old.ctypes.data, n) == n and np.array_equal(host, host_old)
    takers = {"old": fresh(), "new_host": fresh(), "new_device": fresh(), "off": fresh(off=True)}
    results = {}

    def first_match(m, key):
        T = T_init.copy()
        t0 = time.perf_counter()
        ok = m.Match(cl, T, update_map=False)
        dt = time.perf_counter() - t0
        results[key] = (ok, T.tobytes(), m.stats.iterations, m.stats.n_valid, m.map_size())
        return dt

    def op_old_import(m=None, key="old"):
        m = m or takers["old"]
        dt = timed(lambda: m.ImportMap(host))
        times["first_match_after_" + key + "_import"].append(first_match(m, key))
        return dt

    def op_new_import_host():
        dt = timed(lambda: takers["new_host"].ImportMapBlob(host.ctypes.data, n, False))
        times["first_match_after_new_import"].append(first_match(takers["new_host"], "new"))
        return dt

    def op_new_import_device():
        m = takers["new_device"]
        dt = timed(lambda: m.ImportMapBlob(dev.value, n, True))
        times["first_map_export_after_device_import"].append(timed(lambda: lib.fls_map_export(m._h, host_old.ctypes.data, n)))
        return dt

    def op_off_import():
        return timed(lambda: takers["off"].ImportMapBlob(host.ctypes.data, n, False))

    def op_first_old_import():
        m = fresh()  # (creation is not timed)
        dt = timed(lambda: m.ImportMap(host))
        m.close()
        return dt

    def op_first_new_import():
        m = fresh()
        dt = timed(lambda: m.ImportMapBlob(dev.value, n, True))
        m.close()
        return dt

    ops = {"old_export_fls_map_export": lambda: timed(lambda: lib.fls_map_export(owner_old._h, host_old.ctypes.data, n)),
           "new_export_to_host": lambda: timed(lambda: owner.ExportMapBlob(host.ctypes.data, n, False)),
           "new_export_to_device_buffer": lambda: timed(lambda: owner.ExportMapBlob(dev.value, n, True)),
           "switch_off_export_to_host": lambda: timed(lambda: owner_off.ExportMapBlob(host_old.ctypes.data, n, False)),
           "old_import_fls_map_import": op_old_import, "new_import_from_host": op_new_import_host, "new_import_from_device_buffer": op_new_import_device,
           "switch_off_import_from_host": op_off_import, "first_old_import_fresh_handle": op_first_old_import, "first_new_import_fresh_handle": op_first_new_import}
    times = {k: [] for k in list(ops) + ["first_match_after_old_import", "first_match_after_new_import", "first_map_export_after_device_import"]}
    for rnd in range(warmup + rounds):
        if rnd == warmup:
            for v in times.values():
                v.clear()
        for name in (list(ops) if rnd % 2 == 0 else list(reversed(ops))):
            times[name].append(ops[name]())
    out = {k: q(v) for k, v in times.items()}
    out["blob_MB"] = round(n / 1e6, 3)
    out["points"], out["voxels"] = int(owner.map_size()), int(owner.map_size(102))
    out["owner_counters_168_169_147"] = [int(owner.map_size(s)) for s in (168, 169, 147)]
    out["new_device_taker_counters_170_171"] = [int(takers["new_device"].map_size(s)) for s in (170, 171)]
    out["same_first_match_after_old_and_new_import"] = bool(results["old"] == results["new"])
    out["same_bytes_old_and_new_export"] = bool(np.array_equal(host, host_old))

    def separated(new, old):
        return bool(out[new]["p75_ms"] < out[old]["p25_ms"])
    out["separated_new_p75_below_old_p25"] = {
        "new_export_to_host vs old_export_fls_map_export": separated("new_export_to_host", "old_export_fls_map_export"),
        "new_export_to_device_buffer vs old_export_fls_map_export": separated("new_export_to_device_buffer", "old_export_fls_map_export"),
        "new_import_from_host vs old_import_fls_map_import": separated("new_import_from_host", "old_import_fls_map_import"),
        "new_import_from_device_buffer vs old_import_fls_map_import": separated("new_import_from_device_buffer", "old_import_fls_map_import"),
        "first_new_import_fresh_handle vs first_old_import_fresh_handle": separated("first_new_import_fresh_handle", "first_old_import_fresh_handle"),
        "first_match_after_new_import vs first_match_after_old_import": separated("first_match_after_new_import", "first_match_after_old_import"),
    }
    for m in [owner, owner_old, owner_off] + list(takers.values()):
        m.close()
    hip.hipFree(dev)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "ivox_blob_perf.json"))
    a = ap.parse_args()
    from funny_lidar_slam_amd import _lib, registration as reg
    assert _lib.device_count() >= 1, "needs an MI355X"
    hip = C.CDLL("libamdhip64.so")  # the runtime libfls_reg.so itself is linked against
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    maps, scan, T_init = maps_and_scan()
    doc = {"warmup": a.warmup, "rounds": a.rounds, "maps": {}}
    for name, cloud in maps.items():
        for loc in (False, True):
            key = name + ("/localization_handle" if loc else "/mapping_handle_after_3_updates")
            doc["maps"][key] = measure(reg, _lib.lib(), hip, cloud, scan, T_init, loc, a.warmup, a.rounds)
            print(key, json.dumps(doc["maps"][key]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.json)


if __name__ == "__main__":
    main()
