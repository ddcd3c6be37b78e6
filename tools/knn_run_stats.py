"""How much of the iVox kNN kernel's voxel work the 16 queries of a wave share (csrc/kernels_ivox_coop.hpp, the shared-run path of the brick image).
CPU only, numpy.  A wave holds the 16 consecutive queries [16 w, 16 w + 16) of the scan; a RUN is a maximal stretch of consecutive queries of a wave
with the same (kx, ky, kz, have); the wave takes the shared path when it has at most R_MAX runs and the 19-voxel neighbourhoods of its runs hold at most
CAP map points together.  `predict_waves` is that gate from pose, scan and map, and the GPU tests compare the kernel's shared-wave count with it.

usage: python tools/knn_run_stats.py [R_MAX CAP]      (make_config(1) at T_init and T_gt; default: the tables of several gates)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEY_LIMIT = (1 << 20) - 2   # csrc/device_common.hpp kKeyLimit
BRICK_LOG = 3               # kBrickLog: bricks of 8 x 8 x 8 voxels
WAVE_QUERIES = 16           # four lanes per query, 64 lanes
# NEARBY18 (csrc/kernels_ivox_coop.hpp nearby18)
DX = (0, -1, 1, 0, 0, 0, 0, 1, -1, 1, -1, 1, -1, 1, -1, 0, 0, 0, 0)
DY = (0, 0, 0, 1, -1, 0, 0, 1, 1, -1, -1, 0, 0, 0, 0, 1, -1, 1, -1)
DZ = (0, 0, 0, 0, 0, -1, 1, 0, 0, 0, 0, 1, 1, -1, -1, 1, 1, -1, -1)
NEARBY = np.stack([DX, DY, DZ], 1).astype(np.int64)


def roundf(x):
    """C roundf on float32 (halves away from zero); x - trunc(x) is exact"""
    x = np.asarray(x, np.float32)
    t = np.trunc(x)
    return t + np.where(np.abs(x - t) >= np.float32(0.5), np.copysign(np.float32(1.0), x), np.float32(0.0)).astype(np.float32)


def pack(k):
    """int64 (..., 3) voxel keys, each |k| < 2^20 + 1 -> one int64 (order preserving per axis, collision free)"""
    k = np.asarray(k, np.int64) + (1 << 21)
    return (k[..., 0] << 44) | (k[..., 1] << 22) | k[..., 2]


def transform_keys(scan, T, inv_res=2.0):
    """the kernel's query keys: float(T x) in float64 products summed left to right, roundf(p * inv_res), in_range"""
    s = np.asarray(scan, np.float32)[:, :3].astype(np.float64)
    T = np.asarray(T, np.float64)
    p = np.stack([((T[r, 0] * s[:, 0] + T[r, 1] * s[:, 1]) + T[r, 2] * s[:, 2]) + T[r, 3] for r in range(3)], 1).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        f = roundf(p * np.float32(inv_res))
        in_range = (np.abs(f) < np.float32(KEY_LIMIT)).all(1)
    k = np.where(in_range[:, None], f, np.float32(0.0)).astype(np.int64)
    return k, in_range


class VoxelMap:
    """occupied voxels of a map cloud (every point kept: the first insertion into an empty iVox map) and the bricks the image holds"""

    def __init__(self, map_pts, inv_res=2.0):
        m = np.asarray(map_pts, np.float32)[:, :3]
        k = roundf(m * np.float32(inv_res)).astype(np.int64)
        self.keys, self.counts = np.unique(pack(k), return_counts=True)
        vox = np.unique(k, axis=0)
        # a brick exists where one of its interior or face / edge halo cells is occupied (device_common.hpp brick_for_each_mirror; no corners)
        loc = vox & 7
        e = np.where(loc == 0, -1, np.where(loc == 7, 1, 0))
        bricks = [vox >> BRICK_LOG]
        for msk in range(1, 7):
            use = np.array([(msk >> a) & 1 for a in range(3)], np.int64)
            ok = ((use == 0) | (e != 0)).all(1)
            bricks.append((vox[ok] >> BRICK_LOG) + e[ok] * use)
        self.bricks = np.unique(pack(np.vstack(bricks)))

    def count(self, k):
        p = pack(k)
        i = np.clip(np.searchsorted(self.keys, p), 0, len(self.keys) - 1)
        return np.where(self.keys[i] == p, self.counts[i], 0)

    def has_brick(self, k):
        p = pack(np.asarray(k, np.int64) >> BRICK_LOG)
        i = np.clip(np.searchsorted(self.bricks, p), 0, len(self.bricks) - 1)
        return self.bricks[i] == p


def wave_table(scan, T, vmap, inv_res=2.0):
    """per wave: runs, staged entries (sum over the runs of their 19 cell counts), cell probes / candidate rows the per-query code makes, and what the
    run-wise form makes; per query: hit voxels and candidates"""
    k, in_range = transform_keys(scan, T, inv_res)
    n = len(k)
    have = in_range & vmap.has_brick(k)
    cells = np.where(have[:, None], vmap.count(k[:, None, :] + NEARBY[None]), 0)   # (n, 19)
    cand, hits = cells.sum(1), (cells > 0).sum(1)
    nw = (n + WAVE_QUERIES - 1) // WAVE_QUERIES
    pad = nw * WAVE_QUERIES - n                                  # lanes past the scan: key 0, no brick
    kk = np.vstack([k, np.zeros((pad, 3), np.int64)]).reshape(nw, WAVE_QUERIES, 3)
    hv = np.concatenate([have, np.zeros(pad, bool)]).reshape(nw, WAVE_QUERIES)
    cd = np.concatenate([cand, np.zeros(pad, np.int64)]).reshape(nw, WAVE_QUERIES)
    start = np.ones((nw, WAVE_QUERIES), bool)
    start[:, 1:] = (kk[:, 1:] != kk[:, :-1]).any(2) | (hv[:, 1:] != hv[:, :-1])
    act = np.concatenate([np.ones(n, bool), np.zeros(pad, bool)]).reshape(nw, WAVE_QUERIES)
    return dict(runs=start.sum(1), entries=(cd * start).sum(1), cand_now=cd.sum(1), probes_now=19 * act.sum(1), probes_run=19 * start.sum(1),
                cand=cand, hits=hits)


def predict_waves(scan, T, map_or_vmap, r_max, cap, inv_res=2.0):
    """bool per wave of the launch that has at least one query: it takes the shared path"""
    vmap = map_or_vmap if isinstance(map_or_vmap, VoxelMap) else VoxelMap(map_or_vmap, inv_res)
    if len(scan) == 0:
        return np.zeros(0, bool)
    w = wave_table(scan, T, vmap, inv_res)
    return (w["runs"] <= r_max) & (w["entries"] <= cap)


def _report(out, cfg, vmap, gates):
    poses = (("T_init (iteration 1)", cfg["T_init"]), ("T_gt (iterations 2-3)", cfg["T_gt"]))
    tabs = [(name, wave_table(cfg["scan"], T, vmap)) for name, T in poses]
    out("scan %d points, map %d points in %d voxels, %d waves" % (len(cfg["scan"]), len(cfg["map"]), len(vmap.keys), len(tabs[0][1]["runs"])))
    out("")
    out("| pose | candidates / hit voxels per query | runs per wave: mean, median | candidate rows per wave now | fetched once per run |")
    out("|---|---|---|---|---|")
    for name, w in tabs:
        out("| %s | %.1f / %.1f | %.2f, %d | %.0f | %.0f |" % (name, w["cand"].mean(), w["hits"].mean(), w["runs"].mean(), int(np.median(w["runs"])), w["cand_now"].mean(),
                                                          w["entries"].mean()))
    out("")
    out("| runs <= / entries <= | waves that qualify | candidate fetches left, vs per-query | cell probes left |")
    out("|---|---|---|---|")
    for r_max, cap in gates:
        cols = []
        for _, w in tabs:
            sh = (w["runs"] <= r_max) & (w["entries"] <= cap)
            cols.append((sh.mean(), (np.where(sh, w["entries"], w["cand_now"]).sum()) / w["cand_now"].sum(),
                         np.where(sh, w["probes_run"], w["probes_now"]).sum() / w["probes_now"].sum()))
        out("| %d / %d | %s | %s | %s |" % (r_max, cap, " / ".join("%.0f %%" % (100 * c[0]) for c in cols), " / ".join("%.0f %%" % (100 * c[1]) for c in cols),
                                           " / ".join("%.0f %%" % (100 * c[2]) for c in cols)))


if __name__ == "__main__":
    from funny_lidar_slam_amd import synth

    gates = [(int(sys.argv[1]), int(sys.argv[2]))] if len(sys.argv) > 2 else [(3, 256), (4, 256), (6, 320)]
    cfg = synth.make_config(1)
    _report(print, cfg, VoxelMap(cfg["map"]), gates)
