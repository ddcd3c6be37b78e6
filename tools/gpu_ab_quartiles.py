"""A/B of two builds of libfls_reg.so on single-job BASELINE configs[1] Matches (PointToPlane_IVOX, 64 x 1800 scan, 1e6-point map), for kernel
changes that must not move the headline: `python tools/gpu_ab_quartiles.py <libA> <libB> [matches=300] [passes=2]`.
Alternating sub-processes (A B A B ...), per process `matches` timed resident Matches (fls_match_resident) and as many whole Matches from host
memory (fls_match: the first kNN launch reads the staging buffer) after 40 untimed ones.  Per process one line: median, p25 and p75 in microseconds,
iterations, n_valid and the pose bits.  The last lines say whether the results are equal and whether the quartile ranges of A and B overlap."""
import json, os, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if len(sys.argv) > 2 and sys.argv[1] == "one":
    import time
    import numpy as np
    from funny_lidar_slam_amd import registration as reg, synth
    reps = int(sys.argv[2])
    cfg = synth.make_config(1)
    m = reg.make_matcher("PointToPlane_IVOX", reg.YAML_NCLT_IVOX)
    m.AddCloudToLocalMap([cfg["map"]])
    cl = reg.PointcloudCluster(planar_cloud_=cfg["scan"])
    m.UploadScan(cl)
    run, Tv = m.resident_call(cfg["T_init"])
    out = {}

    def whole():
        T = cfg["T_init"].copy()
        m.Match(cl, T, update_map=False)
        return T

    for name, call in (("resident", run), ("whole", whole)):
        for _ in range(40):
            call()
        ts = []
        for _ in range(reps):
            t = time.perf_counter(); r = call(); ts.append(time.perf_counter() - t)
        T = np.array(Tv if name == "resident" else r, dtype=np.float64)
        q1, med, q3 = (1e6 * float(v) for v in np.percentile(ts, [25, 50, 75]))
        out[name] = {"median_us": round(med, 1), "p25_us": round(q1, 1), "p75_us": round(q3, 1), "iterations": int(m.stats.iterations),
                     "n_valid": int(m.stats.n_valid), "pose": T.tobytes().hex()}
    m.close()
    print("ONE " + json.dumps(out), flush=True)
else:
    a, b = sys.argv[1], sys.argv[2]
    reps = sys.argv[3] if len(sys.argv) > 3 else "300"
    passes = int(sys.argv[4]) if len(sys.argv) > 4 else 2
    rows = {"A": [], "B": []}
    for k in range(2 * passes):
        side = "AB"[k % 2]
        lib = a if side == "A" else b
        env = dict(os.environ, FLS_REG_LIB=os.path.abspath(lib))
        p = subprocess.run([sys.executable, __file__, "one", reps], env=env, capture_output=True, text=True, timeout=600)
        line = [l for l in p.stdout.splitlines() if l.startswith("ONE ")]
        if p.returncode != 0 or not line:
            print(f"{side} {lib}: failed ({p.returncode}) {p.stderr.strip()[-400:]}", flush=True)
            sys.exit(1)
        r = json.loads(line[0][4:])
        rows[side].append(r)
        for leg in ("resident", "whole"):
            v = r[leg]
            print(f"{side} {os.path.basename(lib)} {leg:8s}: median {v['median_us']:8.1f} us  p25 {v['p25_us']:8.1f}  p75 {v['p75_us']:8.1f}  iterations {v['iterations']}  "
                  f"n_valid {v['n_valid']}  pose {v['pose'][:16]}..{v['pose'][-16:]}", flush=True)
    for leg in ("resident", "whole"):
        results = {(r[leg]["iterations"], r[leg]["n_valid"], r[leg]["pose"]) for side in rows for r in rows[side]}
        lo = {s: min(r[leg]["p25_us"] for r in rows[s]) for s in rows}
        hi = {s: max(r[leg]["p75_us"] for r in rows[s]) for s in rows}
        overlap = lo["A"] <= hi["B"] and lo["B"] <= hi["A"]
        print(f"{leg}: results equal: {len(results) == 1}; quartile ranges A [{lo['A']}, {hi['A']}] B [{lo['B']}, {hi['B']}] overlap: {overlap}", flush=True)
