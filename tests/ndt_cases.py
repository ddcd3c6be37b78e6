"""Constructed inputs for the IncrementalNDT kernels: voxel maps written as images (include/fls_map_ndt.h), probe clouds and voxel histories.

Scoring cases (scoring_cases()): an image + a probe cloud + a pose, voxel size 1.0, one Gauss-Newton iteration, update_map = False.  Every point of a
probe cloud sits in a 0.2 m leaf cell of its own, so the source VoxelGrid hands every point on as itself; what changes is the order (ascending leaf
index), and `filtered()` gives it.  The named cases place points AT the decisions of ndt_kernel / ndt_lanes_kernel (csrc/kernels_knn.hpp); each carries a
backbone of well-separated estimated voxels with one point each, which keeps H conditioned.

Histories (histories()): a start image (or none) + clouds handed to AddCloudToLocalMap one by one.  A mapping handle that imported an image with
flag_first_scan = 0, or that has taken its first cloud, runs every cloud as a batch of UpdateVoxel (incremental_ndt.h:130-179; ndt_upd_voxel in
csrc/kernels_ndt_update.hpp on the device, NdtMirror::update_voxel on the host).  Every voxel of a history follows a script: points per batch.

tests/test_ndt_cases.py shows on the oracle alone that every case is what it says; tests/test_gpu_ndt_stages.py runs them on the device."""
import functools

import numpy as np

from funny_lidar_slam_amd import registration as reg
from oracle import oracle as O

MODE = "IncrementalNDT"
LEAF = 0.2
KEY_LIMIT = O.NDT_KEY_LIMIT
NB = np.array([(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1)])  # incremental_ndt.h:122-127
Y = dict(reg.YAML_NCLT_NDT, optimization_iter_num=1, ndt_capacity=20000)
THR = Y["ndt_outlier_threshold"]
SIZES = (1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4097)
I3 = np.eye(3).reshape(-1)

POSE_ID = np.eye(4)


def _general_pose():
    w = np.array([0.03, -0.02, 0.05])
    T = np.eye(4)
    T[:3, :3] = O.so3_exp(w)
    T[:3, 3] = [0.4, -0.3, 0.2]
    return T


POSE_GEN = _general_pose()


def filtered(cloud):
    """what the source VoxelGrid hands on (the oracle's filter; test_ndt_cases.py holds the library's host filter against it)"""
    return O.voxel_grid(np.ascontiguousarray(cloud, np.float32), LEAF)[:, :3].copy()


def key_of(q):
    """cast<int>(q / voxel size), voxel size 1.0: truncation toward zero"""
    return np.trunc(np.asarray(q, np.float64)).astype(np.int64)


def centre(key):
    """the middle of voxel `key` (key 0 spans (-1, 1))"""
    k = np.asarray(key, np.float64)
    return np.where(k > 0, k + 0.5, np.where(k < 0, k - 0.5, 0.0))


def voxel(key, mu=None, info=None, sigma=None, est=1, num_points=10, points=()):
    pts = np.zeros(24)
    p = np.asarray(points, np.float64).reshape(-1)
    pts[:p.size] = p
    return dict(key=tuple(int(k) for k in key), mu=centre(key) if mu is None else np.asarray(mu, np.float64),
                info=(4.0 * I3 if info is None else np.asarray(info, np.float64).reshape(-1)),
                sigma=(np.zeros(9) if sigma is None else np.asarray(sigma, np.float64).reshape(-1)), est=int(est), num_points=int(num_points),
                pending=p.size // 3, points=pts)


def image_of(voxels, y, next_vid=None, first_scan=0, vids=None):
    """voxels, OLDEST first -> image bytes (voxel ids: the position, or `vids`)"""
    n = len(voxels)
    vids = np.arange(n, dtype=np.int32) if vids is None else np.asarray(vids, np.int32)
    d = dict(keys=np.array([v["key"] for v in voxels], np.int32).reshape(n, 3), vid=vids, num_points=np.array([v["num_points"] for v in voxels], np.int32),
             estimated=np.array([v["est"] for v in voxels], np.uint8), pending=np.array([v["pending"] for v in voxels], np.int32),
             points=np.array([v["points"] for v in voxels]).reshape(n, 24), mu=np.array([v["mu"] for v in voxels]).reshape(n, 3),
             sigma=np.array([v["sigma"] for v in voxels]).reshape(n, 9), info=np.array([v["info"] for v in voxels]).reshape(n, 9),
             next_vid=(int(vids.max()) + 1 if n else 0) if next_vid is None else next_vid, flag_first_scan=first_scan)
    assert len(set(v["key"] for v in voxels)) == n, "a key twice"
    return O.ndt_encode_image(d, y["ndt_voxel_size"], y["ndt_min_points_in_voxel"], y["ndt_max_points_in_voxel"], y["ndt_capacity"])


def source_for(targets, T):
    """float32 source points whose images under T lie next to `targets` (exactly on them for the identity)"""
    t = np.asarray(targets, np.float64).reshape(-1, 3)
    return ((t - T[:3, 3]) @ T[:3, :3]).astype(np.float32)  # R^T (t - trans), row form


# ---- the backbone: 84 estimated voxels three keys apart (no voxel is another's neighbour), one point each ----
@functools.lru_cache(maxsize=None)
def backbone():
    rng = np.random.default_rng(5)
    vox, tgt = [], []
    for i in range(-3, 4):
        for j in range(4):
            for k in range(-1, 2):
                key = (3 * i, 20 + 3 * j, 3 * k)
                A = rng.normal(size=(3, 3))
                info = A @ A.T + 4.0 * np.eye(3)  # SPD, eigenvalues 4 .. ~15
                mu = centre(key) + rng.uniform(-0.1, 0.1, 3)
                vox.append(voxel(key, mu=mu, info=info.reshape(-1, order="F")))
                tgt.append(mu + rng.uniform(-0.2, 0.2, 3))
    order = rng.permutation(len(vox))
    return [vox[i] for i in order], np.array(tgt)[order]


def _case(name, voxels, targets, T=POSE_ID, y=Y, **kw):
    bv, bt = backbone()
    vox = list(bv) + list(voxels)
    tg = np.concatenate([bt, np.asarray(targets, np.float64).reshape(-1, 3)])
    c = dict(name=name, y=y, T=T.copy(), image=image_of(vox, y), voxels=vox, cloud=source_for(tg, T), conditioned=True, out_of_range=0)
    c.update(kw)
    return c


def _gate(nextfloat):
    """seven stations, one per neighbour slot s: a point in voxel K, ONE voxel near it, at K + NB[s], info = 20 I and mu half a metre below the point
    in x: e = (0.5, 0, 0), r = (0.5 * 20) * 0.5 = 5.0 == ndt_outlier_threshold to the bit -- kept (the reference rejects r > threshold only).
    nextfloat: the point's x is the next float32 up, e0 > 0.5, r > 5.0 -- rejected."""
    vox, tgt = [], []
    for s in range(7):
        K = np.array([40 + 6 * s, 2, 2])
        p = (K + np.array([0.75, 0.5, 0.5])).astype(np.float32)  # exact in float32
        if nextfloat:
            p[0] = np.nextafter(p[0], np.float32(np.inf))
        mu = np.array([float(K[0]) + 0.25, 2.5, 2.5])
        vox.append(voxel(K + NB[s], mu=mu, info=20.0 * I3))
        tgt.append(p.astype(np.float64))
    return _case("gate_next" if nextfloat else "gate_eq", vox, tgt, gate_points=np.array(tgt, np.float32))


def _nan_residual():
    """voxel A: info[0] = 1e308, info[1] = -1e308 (finite, so the importer takes them), mu four metres from the point in x and y: e0 info[0] = +inf,
    e1 info[1] = -inf, their sum NaN, r NaN.  Voxel B: info = 1e308 I, r = +inf.  Both rejected; the backbone points around them in the cloud are not."""
    KA, KB = np.array([40, 2, 2]), np.array([46, 2, 2])
    pA, pB = centre(KA), centre(KB)
    iA = np.zeros(9); iA[0], iA[1], iA[4], iA[8] = 1e308, -1e308, 1.0, 1.0
    vox = [voxel(KA, mu=pA - np.array([4.0, 4.0, 0.0]), info=iA), voxel(KB, mu=pB - np.array([4.0, 0.0, 0.0]), info=1e308 * I3)]
    return _case("nan_residual", vox, [pA, pB], nan_points=np.array([pA, pB], np.float32))


def _truncation(which):
    """voxels at keys -2..2 on every axis (info 0.8 .. 2 I: a point reaches its own voxel and most of its six neighbours), points at every combination of the
    listed coordinates.  -0.9 and -1.0 share a leaf cell of the source filter, so the list comes in two halves (a: +-0.9, b: +-1.0).  (-0.0 reaches the
    kernel as +0.0: the filter's centroid of one point is 0.0 + -0.0.)"""
    vals = [0.3, -0.3, -0.0, 1.3, -1.3] + ([0.9, -0.9] if which == "a" else [1.0, -1.0])
    vox = []
    for n, key in enumerate((a, b, c) for a in range(-2, 3) for b in range(-2, 3) for c in range(-2, 3)):
        vox.append(voxel(key, info=(0.8 + 0.3 * (n % 5)) * I3))
    tgt = np.array([(a, b, c) for a in vals for b in vals for c in vals])
    return _case("truncation_" + which, vox, tgt)


def _key_edge():
    """the largest keys the importer admits, +-(KEY_LIMIT - 1), on every axis; a point inside each (its outward neighbour KEY_LIMIT cannot exist) and a point
    one voxel further out, where fabs(f) < kKeyLimit fails: count 0, ids -1 (no voxel near it on the oracle's side either).  info = 1e-8 I keeps the
    rotation block of H, which grows with |p|^2 = 1e12, in proportion.  (An extent of > INT_MAX leaves: the source filter hands the cloud on unfiltered.)"""
    vox, tgt, n_out = [], [], 0
    for a in range(3):
        for sgn in (1.0, -1.0):
            key = np.array([40 + a, 2, 2]); key[a] = int(sgn) * (KEY_LIMIT - 1)
            c = centre(key)
            vox.append(voxel(key, mu=c, info=1e-8 * I3))
            out = np.array([50.0 + a, 8.5, 8.5]); out[a] = sgn * (KEY_LIMIT + 0.5)
            tgt += [c, out]
            n_out += 1
    return _case("key_edge", vox, tgt, out_of_range=n_out)


def _unestimated():
    """a row of voxels along x, every second one waiting (estimated = 0, three pending points) -- with a mean and an information matrix in place that
    WOULD score, so only the estimated flag keeps them out"""
    vox, tgt = [], []
    for i in range(9):
        key = (40 + i, 2, 2)
        if i % 2:
            pts = centre(key) + np.array([[0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1]])
            vox.append(voxel(key, est=0, num_points=3, points=pts))
        else:
            vox.append(voxel(key))
        tgt.append(centre(key) + np.array([0.1, -0.1, 0.05]))
    return _case("unestimated", vox, tgt, T=POSE_GEN, waiting_vids=[84 + i for i in range(9) if i % 2])


@functools.lru_cache(maxsize=None)
def sizes_map():
    """17 x 17 x 15 adjacent voxels (4335), and a point in each of 4097 of them, in an order that spreads every prefix over the block"""
    rng = np.random.default_rng(9)
    keys = [(a, b, c) for a in range(30, 47) for b in range(-8, 9) for c in range(-7, 8)]
    vox = [voxel(k, mu=centre(k) + rng.uniform(-0.05, 0.05, 3), info=(3.0 + 0.25 * (n % 7)) * I3) for n, k in enumerate(keys)]
    pick = rng.permutation(len(keys))[:max(SIZES)]
    tgt = np.array([centre(keys[i]) + rng.uniform(-0.3, 0.3, 3) for i in pick])
    return image_of(vox, Y), vox, tgt


def sizes_case(n):
    image, vox, tgt = sizes_map()
    return dict(name="sizes_%d" % n, y=Y, T=POSE_GEN.copy(), image=image, voxels=vox, cloud=source_for(tgt[:n], POSE_GEN), conditioned=n >= 63, out_of_range=0)


def effective_floor(n_pairs):
    """the backbone alone, its first n_pairs points: each point meets exactly one voxel, so n_pairs effective (point, voxel) pairs"""
    bv, bt = backbone()
    return dict(name="effective_%d" % n_pairs, y=Y, T=POSE_ID.copy(), image=image_of(bv, Y), voxels=bv, cloud=source_for(bt[:n_pairs], POSE_ID),
                conditioned=False, out_of_range=0)


def hash_key(packed):
    """csrc/device_common.hpp::hash_key (the 64-bit finaliser of MurmurHash3, low 32 bits) on packed keys"""
    k = np.asarray(packed, np.uint64).copy()
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xff51afd7ed558ccd)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xc4ceb9fe1a85ec53)
    k ^= k >> np.uint64(33)
    return (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def colliding_keys():
    """three voxel keys, three apart from everything, whose hashes agree in the low 20 bits: they start their probe chains in one slot of every table of up to
    2^20 entries"""
    keys = np.array([(a, b, c) for a in range(100, 400, 3) for b in range(100, 400, 3) for c in range(-30, 31, 3)], np.int64)
    h = hash_key(O.ndt_pack_keys(keys)) & np.uint32((1 << 20) - 1)
    order = np.argsort(h, kind="stable")
    hs = h[order]
    i = int(np.flatnonzero((hs[2:] == hs[:-2]))[0])
    return [tuple(int(v) for v in keys[order[i + j]]) for j in range(3)]


def after_eviction():
    """capacity 120, an image of 119 voxels: 35 in a row along x, oldest first, then the backbone (every one estimated).  Cloud 1 creates ten voxels of forty
    points each (estimated at once): the ten oldest go.  Cloud 2 puts six points into the key of the oldest: created again, with a new voxel id (and entry 10
    goes).  Probes: in the evicted keys 0..10, in the survivors next to them, in the ten new voxels.  Tombstones on a probe chain: colliding_keys() gives A
    (old, evicted by cloud 1), B (old, survives) and D (created by cloud 1): D's entry lies behind A's and B's, and after the batch A's is a tombstone."""
    y = dict(Y, ndt_capacity=120)
    rng = np.random.default_rng(13)
    A, B, D = colliding_keys()
    old_keys = [(20 + i, 2, 0) for i in range(35)]
    new_keys = [(20 + i, 8, 0) for i in range(10)]
    old_keys[3], old_keys[20], new_keys[4] = A, B, D
    old = [voxel(k, info=(3.0 + 0.5 * (i % 5)) * I3) for i, k in enumerate(old_keys)]
    new = [history_points(k, 40, rng) for k in new_keys]  # (400 points: without slack the table is rebuilt for them)
    c1 = np.concatenate(new)
    c2 = history_points(old_keys[0], 6, rng)
    # (a voxel estimated from a few points is narrow: its probe sits on their mean)
    tgt = [c2.astype(np.float64).mean(0)] + [centre(k) + np.array([0.1, 0.1, 0.1]) for k in old_keys[1:14] + [B]] + [p.astype(np.float64).mean(0) for p in new]
    bv, bt = backbone()  # the backbone is touched by neither cloud: it must not be what is evicted, so it is the YOUNGEST part of the image
    vox = old + list(bv)
    tg = np.concatenate([bt, np.array(tgt)])
    return dict(name="after_eviction", y=y, T=POSE_ID.copy(), image=image_of(vox, y), voxels=vox, cloud=source_for(tg, POSE_ID), conditioned=True, out_of_range=0,
                pre_clouds=[c1, c2], evicted_keys=old_keys[1:11], recreated_key=old_keys[0], chain=(A, B, D))


def scoring_cases():
    out = [_gate(False), _gate(True), _nan_residual(), _truncation("a"), _truncation("b"), _key_edge(), _unestimated(),
           _case("backbone_general", [], np.zeros((0, 3)), T=POSE_GEN)]
    return {c["name"]: c for c in out}


SCORING_NAMES = ("gate_eq", "gate_next", "nan_residual", "truncation_a", "truncation_b", "key_edge", "unestimated", "backbone_general")
COND_EXEMPT = ("nan_residual",)  # (and effective_floor, which is built by effective_floor())


HY = dict(Y, ndt_min_effective_pts=1)  # a history's probe has one point per voxel: the effective-point floor is not what it is about


# ---- histories ------------------------------------------------------------------------------------------------------------------------------------------
def _cells(key):
    """centres of the 0.2 m leaf cells of voxel `key` per axis (key 0 spans (-1, 1): ten cells; z is kept inside (-0.8, 0.8))"""
    ax = []
    for a, k in enumerate(key):
        if k == 0:
            c = [-0.9 + 0.2 * i for i in range(10)]
            if a == 2:
                c = c[1:-1]
        else:
            c = [abs(k) + 0.1 + 0.2 * i for i in range(5)]
            c = c if k > 0 else [-v for v in c]
        ax.append(c)
    return ax


def history_points(key, n, rng, shape="ball"):
    """n points of voxel `key`, each in a leaf cell of its own, within 0.05 of the cell's centre.  shape: "ball" any cells, "plane" z fixed,
    "line" y and z fixed."""
    ax = _cells(key)
    grid = np.array([(a, b, c) for c in ax[2] for b in ax[1] for a in ax[0]])
    if shape == "plane":
        grid = grid[grid[:, 2] == ax[2][len(ax[2]) // 2]]
    if shape == "line":
        grid = grid[(grid[:, 2] == ax[2][len(ax[2]) // 2]) & (grid[:, 1] == ax[1][2])]
    assert n <= len(grid), (key, n, shape)
    g = grid[rng.permutation(len(grid))[:n]]
    j = rng.uniform(-0.05, 0.05, g.shape)
    if shape == "plane":
        j[:, 2] = 0.0
    if shape == "line":
        j[:, 1:] = 0.0
    return (g + j).astype(np.float32)


def _scripted(name, y, scripts, n_batches, start=None, seed=3, extra=None):
    """scripts: {key: (shape, [points in batch 0, 1, ...])}"""
    rng = np.random.default_rng(seed)
    clouds = []
    for b in range(n_batches):
        parts = [history_points(k, cnt[b], rng, shape) for k, (shape, cnt) in scripts.items() if b < len(cnt) and cnt[b] > 0]
        if extra and b in extra:
            parts.append(np.asarray(extra[b], np.float32).reshape(-1, 3))
        c = np.concatenate(parts)
        clouds.append(c[rng.permutation(len(c))])
    keys = list(scripts) + [tuple(int(v) for v in key_of(p)) for b in (extra or {}) for p in np.asarray(extra[b]).reshape(-1, 3)]
    start_keys = [v["key"] for v in (start or [])]
    probe = np.array([centre(k) + 0.05 for k in dict.fromkeys(keys + start_keys)], np.float32)
    return dict(name=name, y=y, start=None if start is None else image_of(start, y), clouds=clouds, probe=probe, scripts=scripts)


def _main_history(minp):
    """a few dozen voxels, max_points 20.  The first cloud of a handle without a start image would run under the first-scan rule, so the history starts from
    an image of one estimated voxel far away (flag_first_scan = 0): every cloud is a batch of UpdateVoxel."""
    y = dict(HY, ndt_min_points_in_voxel=minp, ndt_max_points_in_voxel=20, ndt_capacity=5000)
    m1 = minp + 1
    S = {}
    x = iter(range(2, 400, 2))  # keys two apart along x (and a second row): no voxel shares points with another
    def key():
        return (next(x), 4, 0)
    n_b = max(minp + 4, 6)
    S[key()] = ("ball", [1] * n_b)                              # waits at 1 .. min points, the estimate at min + 1, then pending beside the estimate
    S[key()] = ("ball", [minp, 1, 0, minp, 1])                  # waits at exactly min, estimate exactly at min + 1; later min pending, then a merge of min + 1
    S[key()] = ("ball", [m1, m1, m1])                           # estimate at once, merges of min + 1
    S[key()] = ("ball", [0, m1, 1, 1, minp - 1 if minp > 1 else 1, 2])
    S[(0, 8, 0)] = ("ball", [150, 150, 3])                      # a 0.2 m leaf fills the voxel: estimate from 150, then frozen (150 > 20): the 150 change nothing
    S[(0, 12, 0)] = ("ball", [10, 150, 2, 7])                   # estimate from 10, a merge of 150 (num_points 160), frozen
    S[key()] = ("ball", [10, 10, m1, m1])                       # 10 + 10 = 20 == max: still merges the next batch; beyond max after that: frozen
    S[key()] = ("ball", [10, 11, m1, 1])                        # 21 == max + 1: frozen at once
    S[key()] = ("plane", [m1 + 2, m1 + 3, 0, m1])               # coplanar all along: the clamp on S[2] fires in every merge
    S[(0, 16, 0)] = ("line", [m1, m1, 0, m1])                   # collinear all along (key 0 on x: ten cells on the line): both clamps fire
    S[(2500, 4, 0)] = ("ball", [m1, m1 + 4, 2, m1])             # coordinates near 2.5 km
    rs = np.random.default_rng(100 + minp)
    for q in range(20):                                         # twenty more with drawn scripts, 0 .. min + 3 points per batch
        S[(2 * q + 2, -8, 0)] = ("ball", [int(v) for v in rs.integers(0, m1 + 3, n_b)])
    S[(-2499, -3, 0)] = ("plane", [m1, m1, m1])
    # the same coordinates again and again, one per batch (the filter would merge them inside one cloud): sigma = 0 at the estimate
    dup_key = key()
    dup = (centre(dup_key) + 0.03).astype(np.float32)
    extra = {b: [dup] for b in range(minp + 1)}
    S[dup_key] = ("ball", [0] * (minp + 1) + [m1, m1])          # ... then merges of distinct points on a sigma of exactly zero
    # first and last point of a batch (the filter orders by leaf index, z first): z = -0.9 and +0.9, outside every other voxel's (-0.8, 0.8)
    fl = key()
    for b in (1, 2, 3):
        extra.setdefault(b, [])
        extra[b] = list(extra[b]) + [np.array([fl[0] + 0.5, 4.5, -0.9], np.float32), np.array([fl[0] + 0.3, 4.3, 0.9], np.float32)]
    h = _scripted("main_min%d" % minp, y, S, n_b, start=[voxel((900, 900, 0))], extra=extra)
    h["dup_key"], h["first_last_key"] = dup_key, fl
    return h


def _started_history():
    """begins at chosen states: num_points == max (still merges), eight pending points (min_points 8: the carry buffer full), a prior sigma; pending beside
    an estimate"""
    y = dict(HY, ndt_min_points_in_voxel=8, ndt_max_points_in_voxel=20, ndt_capacity=5000)
    rng = np.random.default_rng(21)
    def prior(key, num_points, pend=0, est=1):
        pts = history_points(key, 12, rng).astype(np.float64)
        mu = pts.mean(0)
        sg = np.cov(pts.T)
        return voxel(key, mu=mu, sigma=sg.reshape(-1, order="F"), info=np.linalg.inv(sg + 1e-3 * np.eye(3)).reshape(-1, order="F"), est=est,
                     num_points=num_points, points=history_points(key, pend, rng).astype(np.float64) if pend else ())
    start = [prior((2, 4, 0), 20), prior((4, 4, 0), 20, pend=8), prior((6, 4, 0), 12, pend=8),
             voxel((8, 4, 0), est=0, num_points=8, points=history_points((8, 4, 0), 8, rng).astype(np.float64), mu=np.zeros(3), info=np.zeros(9)),
             prior((10, 4, 0), 21), prior((12, 4, 0), 19, pend=3)]
    S = {(2, 4, 0): ("ball", [9, 9]), (4, 4, 0): ("ball", [1, 9]), (6, 4, 0): ("ball", [0, 1, 9]), (8, 4, 0): ("ball", [0, 1, 1]),
         (10, 4, 0): ("ball", [9, 0, 9]), (12, 4, 0): ("ball", [5, 1, 9]), (14, 4, 0): ("ball", [4, 4, 1])}
    return _scripted("started_min8", y, S, 3, start=start, seed=22)


def _eviction_history():
    """capacity 40, a start image of 39 voxels along x (oldest first).  Batch 0 (filter order = ascending z): the oldest voxel A is touched at z = -0.9,
    BEFORE the creations -- it has moved to the front when they come and is skipped; six voxels are created in the middle layers, each evicting the then
    oldest (B, D, E, ...); voxel C, next in line, is touched at z = +0.9, AFTER it went: created again from that point alone -- fresh state, a new voxel id
    -- which evicts one more.  Batch 1 goes on from there."""
    y = dict(HY, ndt_capacity=40, ndt_max_points_in_voxel=20)
    rng = np.random.default_rng(31)
    start = [voxel((2 * i, 4, 0), info=(3.0 + 0.5 * (i % 5)) * I3, num_points=10) for i in range(39)]
    A, C = (0, 4, 0), (4, 4, 0)
    new = [(2 * i, 10, 0) for i in range(6)]
    b0 = [np.array([0.5, 4.5, -0.9], np.float32)] + [history_points(k, 6, rng) for k in new] + [np.array([4.5, 4.5, 0.9], np.float32)]
    b1 = [history_points(C, 6, rng), history_points(A, 6, rng), history_points((50, 10, 0), 2, rng)]
    clouds = [np.concatenate([np.atleast_2d(p) for p in b0]), np.concatenate(b1)]
    probe = np.array([centre(v["key"]) + 0.05 for v in start] + [centre(k) + 0.05 for k in new], np.float32)
    return dict(name="eviction_cap40", y=y, start=image_of(start, y), clouds=clouds, probe=probe, scripts={}, skipped_key=A, recreated_key=C,
                evicted_keys=[(2, 4, 0), (6, 4, 0), (8, 4, 0)])


def histories():
    out = [_main_history(5), _main_history(8), _main_history(1), _started_history(), _eviction_history()]
    return {h["name"]: h for h in out}


HISTORY_NAMES = ("main_min5", "main_min8", "main_min1", "started_min8", "eviction_cap40")
