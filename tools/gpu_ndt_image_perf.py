"""What moving an NDT voxel map costs (FLS_INCREMENTAL_NDT, include/fls_map_ndt.h): the flat image exported on the device
(ndt_image_pack_kernel) into a device buffer and into pinned host memory, imported from either (ndt_image_check_unpack_kernel + the table
build), and a replica-set refresh -- beside the only ways a map could be taken off or handed on before the image existed: the debug read-out of a
device-mode handle (fls_debug_ndt_voxels: every row downloaded and ordered on one host thread) and a second handle built by
AddCloudToLocalMap of the same cloud (possible for a one-cloud map only).

Two maps: the 1,000,000-point map of BASELINE configs[2] and its 100,000-point cut (the points nearest the origin), each built once on a
mapping handle.  The imports go into one handle per map, round after round: from its second import on it reuses the rows and the table it
checked the previous image in (a handle's first import also allocates them).  All operations alternate in one process over warmup + rounds rounds, in an order that is reversed every other round.  Timed
with a host clock, the whole call (every call returns with the stream idle).  The first Match after an import and after a build are timed the
same way (update_map=False): nothing may have been deferred into it.  Reported: median, p25, p75 in ms and the project's separation rule
"new p75 below old p25" -- a gain is claimed only where it holds.

usage: python tools/gpu_ndt_image_perf.py [--warmup 3] [--rounds 20] [--json profiles/ndt_image_perf.json]"""
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


def maps_and_scan():
    from funny_lidar_slam_amd import synth
    cfg = synth.make_config(2, scale=1.0)
    full = cfg["map"]
    near = np.argsort(np.einsum("ij,ij->i", full[:, :2], full[:, :2]), kind="stable")[:100000]
    cut = np.ascontiguousarray(full[np.sort(near)])
    return {"map_%d" % len(full): full, "cut_100000": cut}, np.ascontiguousarray(cfg["scan"]), cfg["T_init"]


def measure(reg, hip, cloud, scan, T_init, warmup, rounds):
    def fresh():
        return reg.make_matcher("IncrementalNDT", reg.YAML_NCLT_NDT)
    owner, taker = fresh(), fresh()
    owner.AddCloudToLocalMap([cloud])
    n = owner.MapImageBytes()
    dev, pinned = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), n) == 0 and hip.hipHostMalloc(C.byref(pinned), n, 0) == 0
    owner.ExportMapImage(dev.value, n, True)
    owner.ExportMapImage(pinned.value, n, False)
    rs = owner.Replicas([0, 0])
    cl = reg.PointcloudCluster(ordered_cloud_=scan)
    results = {}

    def first_match(m, key):
        T = T_init.copy()
        t0 = time.perf_counter()
        ok = m.Match(cl, T, update_map=False)
        dt = time.perf_counter() - t0
        results[key] = (ok, T.tobytes(), m.stats.iterations, m.stats.n_valid, m.map_size())
        return dt

    def op_export_device():
        t0 = time.perf_counter(); owner.ExportMapImage(dev.value, n, True); return time.perf_counter() - t0

    def op_export_pinned():
        t0 = time.perf_counter(); owner.ExportMapImage(pinned.value, n, False); return time.perf_counter() - t0

    def op_import_device():
        t0 = time.perf_counter(); taker.ImportMapImage(dev.value, n, True); dt = time.perf_counter() - t0
        times["first_match_after_import"].append(first_match(taker, "import"))
        return dt

    def op_import_pinned():
        t0 = time.perf_counter(); taker.ImportMapImage(pinned.value, n, False); return time.perf_counter() - t0

    def op_replica_refresh():
        t0 = time.perf_counter(); rs.Refresh(); return time.perf_counter() - t0

    def op_debug_read_out():
        t0 = time.perf_counter(); owner.ndt_voxels(); return time.perf_counter() - t0

    def op_rebuild():
        m = fresh()  # (creation is not timed)
        t0 = time.perf_counter(); m.AddCloudToLocalMap([cloud]); dt = time.perf_counter() - t0
        times["first_match_after_build"].append(first_match(m, "build"))
        m.close()
        return dt

    ops = {"export_to_device_buffer": op_export_device, "export_to_pinned_host": op_export_pinned, "import_from_device_buffer": op_import_device,
           "import_from_pinned_host": op_import_pinned, "replica_set_refresh_one_replica": op_replica_refresh, "debug_read_out_of_device_rows": op_debug_read_out,
           "second_handle_add_cloud": op_rebuild}
    times = {k: [] for k in list(ops) + ["first_match_after_import", "first_match_after_build"]}
    for rnd in range(warmup + rounds):
        if rnd == warmup:
            for v in times.values():
                v.clear()
        for name in (list(ops) if rnd % 2 == 0 else list(reversed(ops))):
            times[name].append(ops[name]())
    out = {k: q(v) for k, v in times.items()}
    out["image_MB"] = round(n / 1e6, 3)
    out["voxels"] = int(owner.map_size())
    out["points"] = int(len(cloud))
    out["owner_counters_156_157_107_118"] = [int(owner.map_size(s)) for s in (156, 157, 107, 118)]
    out["same_first_match_after_import_and_after_build"] = bool(results["import"] == results["build"])

    def separated(new, old):
        return bool(out[new]["p75_ms"] < out[old]["p25_ms"])
    out["separated_new_p75_below_old_p25"] = {
        "export_to_pinned_host vs debug_read_out_of_device_rows": separated("export_to_pinned_host", "debug_read_out_of_device_rows"),
        "export_to_device_buffer vs debug_read_out_of_device_rows": separated("export_to_device_buffer", "debug_read_out_of_device_rows"),
        "import_from_device_buffer vs second_handle_add_cloud": separated("import_from_device_buffer", "second_handle_add_cloud"),
        "import_from_pinned_host vs second_handle_add_cloud": separated("import_from_pinned_host", "second_handle_add_cloud"),
        "replica_set_refresh_one_replica vs second_handle_add_cloud": separated("replica_set_refresh_one_replica", "second_handle_add_cloud"),
        "first_match_after_import vs first_match_after_build": separated("first_match_after_import", "first_match_after_build"),
    }
    rs.close(); owner.close(); taker.close()
    hip.hipFree(dev); hip.hipHostFree(pinned)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "ndt_image_perf.json"))
    a = ap.parse_args()
    from funny_lidar_slam_amd import _lib, registration as reg
    assert _lib.device_count() >= 1, "needs an MI355X"
    hip = C.CDLL("libamdhip64.so")  # the runtime libfls_reg.so itself is linked against
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipHostFree.argtypes = [C.c_void_p]
    maps, scan, T_init = maps_and_scan()
    doc = {"warmup": a.warmup, "rounds": a.rounds, "maps": {}}
    for name, cloud in maps.items():
        doc["maps"][name] = measure(reg, hip, cloud, scan, T_init, a.warmup, a.rounds)
        print(name, json.dumps(doc["maps"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.json)


if __name__ == "__main__":
    main()
