"""Inputs, hook wrappers and the brute-force model for tests/test_gpu_knn_stages.py (include/fls_debug_knn.h): small maps and query sets that reach
the branches of grid_knn_body (csrc/kernels_grid_coop.hpp) and of its serial hand-off knn_grid (csrc/kernels_knn.hpp) which whole Matches reach
rarely or never.  tests/test_knn_cases.py checks, without a GPU, that the model agrees with the oracle and that every case has the property it is
named for.  Every cached array is read-only: the tests share it.

The model is the kernels' own arithmetic in numpy: the query transform in the kernel's expression order, d2 = (dx dx + dy dy) + dz dz in float32
(numpy's element-wise float32 products and sums are single IEEE operations, like the device code built with -ffp-contract=off), candidates ordered
by (d2, map index)."""
from __future__ import annotations

import ctypes as C
import functools
import itertools
from typing import NamedTuple

import numpy as np

from funny_lidar_slam_amd import _lib
from tests.fit_cases import xform_f_model

FP, DP, IP, BP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
F32, F64 = np.float32, np.float64
INF = float("inf")

K_KEY_LIMIT = (1 << 20) - 2            # kKeyLimit (device_common.hpp)
K_MAX_RING = 4                         # kMaxRing (kernels_knn.hpp)
K_MAX_WINDOW_CELLS = 48 << 20          # GridImage::kMaxWindowCells (host_maps.hpp)
CELL1 = F32(np.sqrt(1.0) * 1.0001)     # cell_for_gate(1.0): IcpOptimized, LoamPointToPlaneKdtree
CELL2 = F32(0.5) * CELL1               # LoamFull's half cells
GATE = 1.0                             # point_search_thres of the shipped configurations (a squared distance)
# name -> (cell, rings, gate): the gated ring-1 search, LoamFull's two-stage search, the un-gated search with its ring walk
SETTINGS = {"g1": (CELL1, 1, GATE), "g2": (CELL2, 2, GATE), "u1": (CELL1, 1, INF)}
IDENTITY = np.eye(4).T.reshape(16).copy()


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


class Case(NamedTuple):
    map: np.ndarray       # (nm, 3) float32
    query: np.ndarray     # (nq, 3) float32, in the source frame
    T: np.ndarray         # (16,) float64, column-major
    settings: tuple       # the SETTINGS the case runs at
    info: dict            # what the property tests need (cluster layout, intended rings, ...)


def _case(m, q, T, settings, **info):
    return Case(_ro(np.asarray(m, F32).reshape(-1, 3)), _ro(np.asarray(q, F32).reshape(-1, 3)), _ro(np.asarray(T, F64)), tuple(settings), info)


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def transform5(T, q):
    """grid_knn_body, FLOAT_XFORM = false: float64 ((T0 x + T4 y) + T8 z) + T12, rounded to float32"""
    x, y, z = (q[:, k].astype(F64) for k in range(3))
    return np.stack([(((T[r] * x + T[4 + r] * y) + T[8 + r] * z) + T[12 + r]).astype(F32) for r in range(3)], axis=1)


def transform1(T, q):
    """grid_knn_body, FLOAT_XFORM = true (the fused ICP search): xform_f in float32"""
    return xform_f_model(np.broadcast_to(np.asarray(T, F64), (len(q), 16)), q).astype(F32)


def d2_f32(Q, M):
    """(nq, nm) float32: flann::L2_Simple<float> as the kernels write it"""
    Q, M = np.asarray(Q, F32), np.asarray(M, F32)
    with np.errstate(over="ignore"):  # (a query 3e37 m away: d2 is inf, as on the device)
        dx, dy, dz = (Q[:, None, k] - M[None, :, k] for k in range(3))
        return (dx * dx + dy * dy) + dz * dz


def brute_knn(Q, M, k):
    """the k candidates of lowest (d2, map index) per query -> ids (nq, k) int32 padded with -1, d2 (nq, k) float32 padded with inf.  (d2 >= 0 and
    never NaN here, so the order of the values is the order of their bit patterns; a stable sort breaks ties by the lower index.)"""
    nq, nm = len(Q), len(M)
    ids = np.full((nq, k), -1, np.int32)
    dd = np.full((nq, k), np.inf, F32)
    kk = min(k, nm)
    for a in range(0, nq, 512):
        d2 = d2_f32(Q[a:a + 512], M)
        assert not np.isnan(d2).any()
        o = np.argsort(d2, axis=1, kind="stable")[:, :kk]
        ids[a:a + 512, :kk] = o
        dd[a:a + 512, :kk] = np.take_along_axis(d2, o, axis=1)
    return ids, dd


def file_query(x, cell):
    """the cell of a coordinate as grid_knn_body and knn_grid file the QUERY: floor(double(x) * (1.0 / double(cell)))"""
    return np.floor(np.asarray(x, F32).astype(F64) * (1.0 / F64(cell)))


def file_float(x, cell):
    """floorf(x * inv_cell) in float with inv_cell = 1.0f / cell: how the grid builders filed MAP points before they took the query's expression"""
    inv = F32(1.0) / F32(cell)
    return np.floor((np.asarray(x, F32) * inv).astype(F32)).astype(F64)


def certify_limit(cell, rho=1):
    """(rho cell)^2 (1 - 1e-5) in double: a list whose K-th d2 is not above it is final after the rings up to rho"""
    r = float(rho) * float(F64(cell))
    return r * r * (1.0 - 1e-5)


def out_of_key_range(Qt, cell):
    """queries the search kernels answer with nothing: a cell index beyond the key range on some axis"""
    return (np.abs(file_query(Qt, cell)) >= K_KEY_LIMIT - 3).any(axis=1)


@functools.lru_cache(maxsize=None)
def model5(name):
    """the case's transformed queries, model ids (nq, 5) and d2 (nq, 5)"""
    c = CASES[name]()
    Qt = transform5(c.T, c.query)
    ids, dd = brute_knn(Qt, c.map, 5)
    return _ro(Qt), _ro(ids), _ro(dd)


@functools.lru_cache(maxsize=None)
def model1(name):
    c = CASES[name]()
    Qt = transform1(c.T, c.query)
    ids, dd = brute_knn(Qt, c.map, 1)
    return _ro(Qt), _ro(ids[:, 0]), _ro(dd[:, 0])


def fifth_ring(name, setting):
    """per query, the Chebyshev cell distance between the query's cell and the cell of the model's 5th neighbour (-1: fewer than 5 points)"""
    c = CASES[name]()
    cell = SETTINGS[setting][0]
    Qt, ids, _ = model5(name)
    out = np.full(len(Qt), -1, np.int64)
    has = ids[:, 4] >= 0
    out[has] = np.minimum(np.abs(file_query(c.map[ids[has, 4]], cell) - file_query(Qt[has], cell)).max(axis=1), 2.0 ** 40).astype(np.int64)  # (a query 3e37 m away)
    return out


def gated_classes(dd, gate):
    """the contract's two gated classes: full (the model's 5th d2 is within the gate: the list must be the model's) / rest (the kernel must report
    cnt < 5 or kth > gate, its entries within the gate the model's).  Together they are every query."""
    full = dd[:, 4] <= F32(gate)
    return full, ~full


# ---- hooks -----------------------------------------------------------------------------------------------------------------------------
def _f(a):
    a = np.ascontiguousarray(a, F32)
    assert a.ndim == 2 and a.shape[1] >= 3
    return a, a.ctypes.data_as(FP), a.shape[0], a.shape[1]


def _ok(rc, what):
    assert rc == _lib.FLS_OK, (what, rc, _lib.status_string(rc))


def _unpack(pts, cnt, kth, win):
    return {"ids": pts.view(np.int32)[:, :, 3].copy(), "xyz": pts[:, :, :3].copy(), "cnt": cnt.astype(np.int32), "kth": kth, "has_window": int(win[0])}


def _outs(nq):
    return np.full((nq, 5, 4), 7.0, F32), np.full(nq, 77, np.uint8), np.full(nq, 7.0, F32), np.full(1, 7, np.int32)


def grid_knn5(m, q, cell, rings, gate, T, host_grid):
    mm, pm, nm, sm = _f(m)
    qq, pq, nq, sq = _f(q)
    assert sm == sq
    T = np.ascontiguousarray(T, F64)
    pts, cnt, kth, win = _outs(nq)
    _ok(_lib.lib().fls_debug_grid_knn5(0, pm, nm, pq, nq, sm, float(cell), rings, float(gate), T.ctypes.data_as(DP), int(host_grid), pts.ctypes.data_as(FP),
                                       cnt.ctypes.data_as(BP), kth.ctypes.data_as(FP), win.ctypes.data_as(IP)), "fls_debug_grid_knn5")
    return _unpack(pts, cnt, kth, win)


def grid_knn5_dual(a, b, T, host_grid):
    """a, b: (map, query, cell, rings, gate)"""
    ma, pma, nma, s = _f(a[0]); qa, pqa, nqa, _ = _f(a[1])
    mb, pmb, nmb, _ = _f(b[0]); qb, pqb, nqb, _ = _f(b[1])
    T = np.ascontiguousarray(T, F64)
    oa, ob = _outs(nqa), _outs(nqb)
    _ok(_lib.lib().fls_debug_grid_knn5_dual(0, pma, nma, pqa, nqa, float(a[2]), a[3], float(a[4]), pmb, nmb, pqb, nqb, float(b[2]), b[3], float(b[4]), s,
                                            T.ctypes.data_as(DP), int(host_grid), oa[0].ctypes.data_as(FP), oa[1].ctypes.data_as(BP), oa[2].ctypes.data_as(FP),
                                            oa[3].ctypes.data_as(IP), ob[0].ctypes.data_as(FP), ob[1].ctypes.data_as(BP), ob[2].ctypes.data_as(FP),
                                            ob[3].ctypes.data_as(IP)), "fls_debug_grid_knn5_dual")
    return _unpack(*oa), _unpack(*ob)


def icp_knn1(m, q, cell, max_corr_sq, T, host_grid):
    mm, pm, nm, sm = _f(m)
    qq, pq, nq, _ = _f(q)
    T = np.ascontiguousarray(T, F64)
    ids, eff, win = np.full(nq, 7, np.int32), np.full(nq, 77, np.uint8), np.full(1, 7, np.int32)
    _ok(_lib.lib().fls_debug_icp_knn1(0, pm, nm, pq, nq, sm, float(cell), float(max_corr_sq), T.ctypes.data_as(DP), int(host_grid), ids.ctypes.data_as(IP),
                                      eff.ctypes.data_as(BP), win.ctypes.data_as(IP)), "fls_debug_icp_knn1")
    return {"id": ids, "eff": eff.astype(np.int32), "has_window": int(win[0])}


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
UNIFORM_COUNTS = (1, 31, 32, 33, 257, 2081)  # 2081 queries are 66 workgroups: the XCD re-map of the block index leaves the identity at 65


def _rot(axis, angle):
    a = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


@functools.lru_cache(maxsize=None)
def uniform():
    """~3000 points in a 12 m cube, a non-identity pose; the queries cover a 14 m cube in the map frame (some outside the map's bounding box)"""
    rng = np.random.default_rng(11)
    m = rng.uniform(-6.0, 6.0, (3000, 3)).astype(F32)
    R, t = _rot([0.3, -0.5, 0.8], 0.35), np.array([0.4, -0.25, 0.15])
    T4 = np.eye(4); T4[:3, :3] = R; T4[:3, 3] = t
    qt = rng.uniform(-7.0, 7.0, (UNIFORM_COUNTS[-1], 3))
    q = ((qt - t) @ R).astype(F32)  # R^T (qt - t)
    return _case(m, q, T4.T.reshape(16), ("g1", "g2", "u1"))


@functools.lru_cache(maxsize=None)
def lattice_ties():
    """a 0.25 m lattice (13^3 points, exact coordinates, shuffled indices) with 40 of its points duplicated two to nine times under other indices;
    queries on lattice points, edge midpoints and cell centres; the pose is a translation by exact amounts, so every list is decided by exact ties"""
    rng = np.random.default_rng(12)
    g = np.arange(-6, 7) * 0.25
    lat = np.array(list(itertools.product(g, g, g)))
    dup_of = rng.choice(len(lat), 40, replace=False)
    extra = np.concatenate([np.repeat(lat[i:i + 1], 1 + k % 8 + 0, axis=0) for k, i in enumerate(dup_of)])  # 1 .. 8 more copies: 2 .. 9 in all
    m = np.concatenate([lat, extra])
    m = m[rng.permutation(len(m))]
    t = np.array([0.5, -0.25, 0.75])
    on = lat[rng.choice(len(lat), 150, replace=False)]
    on = np.concatenate([on, lat[dup_of[:20]]])
    mid = lat[rng.choice(len(lat), 100, replace=False)] + np.array([0.125, 0.0, 0.0])
    ctr = lat[rng.choice(len(lat), 100, replace=False)] + 0.125
    qt = np.concatenate([on, mid, ctr])
    T4 = np.eye(4); T4[:3, 3] = t
    return _case(m, qt - t, T4.T.reshape(16), ("g1", "g2", "u1"), n_dup=len(dup_of))


# quad_tails: (label, [(cell offset from the query's cell, points as a function of n)]); the first entry is the cell that holds exactly n points.
# Raster codes of kCellOrder / kShellOrder in brackets: which round and lane of grid_knn_body meets the cell.
QUAD_CLASSES = (
    ("centre", [((0, 0, 0), lambda n: n)]),                                  # round 0, lane 0
    ("face", [((1, 0, 0), lambda n: n)]),                                    # round 0 [14]
    ("edge_r1", [((1, 1, 0), lambda n: n)]),                                 # [17]: index 14, round 1, lane 6
    ("edge_r2", [((-1, 0, 1), lambda n: n)]),                                # [21]: index 16, round 2, lane 0
    ("corner_r3", [((1, 1, 1), lambda n: n)]),                               # [26]: index 26, round 3, lane 2
    ("two_cells_one_lane", [((1, 1, 0), lambda n: n), ((1, 1, -1), lambda n: n % 4 + 1)]),  # [17] and [8]: lane 6's rounds 1 and 2, one flattened loop
    ("shell_first", [((0, 0, -2), lambda n: n)]),                            # shell [12]: index 0, batch 0, lane 0
    ("shell_two_cells", [((0, 0, -2), lambda n: n), ((1, 0, -2), lambda n: n % 4 + 1)]),    # shell [12] and [13]: indices 0 and 8, lane 0, batch 0
    ("shell_mid", [((2, 2, 1), lambda n: n)]),                               # shell [99]: index 81, batch 2 (r = 10), lane 1
    ("shell_corner", [((-2, -2, -2), lambda n: n)]),                         # shell [0]: index 90, batch 2 (r = 11), lane 2
)


@functools.lru_cache(maxsize=None)
def quad_tails(setting):
    """isolated cells holding exactly 1, 2, ..., 9 points, one query per cluster at the centre of its own cell, for the cell size of `setting`; the
    clusters are 12 cells apart"""
    cell = F64(SETTINGS[setting][0])
    rng = np.random.default_rng(13)
    m, q, layout = [], [], []
    for ci, (label, parts) in enumerate(QUAD_CLASSES):
        for n in range(1, 10):
            base = np.array([12 * n, 12 * ci, 0.0])
            q.append((base + 0.5) * cell)
            for off, count in parts:
                for _ in range(count(n)):
                    m.append((base + np.array(off) + 0.5 + rng.uniform(-0.3, 0.3, 3)) * cell)
            layout.append((label, n, tuple(int(v) for v in base), parts[0][0]))
    m = np.array(m)
    m = m[rng.permutation(len(m))]
    return _case(m, np.array(q), IDENTITY, (setting,), layout=layout, cell=F32(cell))


@functools.lru_cache(maxsize=None)
def small_map():
    """a map of 3 points: every list is short"""
    m = [[0.1, 0.2, 0.3], [0.4, -0.3, 0.2], [-0.6, 0.1, 0.0]]
    q = [[0.0, 0.0, 0.0], [0.9, 0.9, 0.9], [2.5, 0.1, 0.0], [-7.0, 3.0, 1.0]]
    return _case(m, q, IDENTITY, ("g1", "g2", "u1"))


PRUNE_D = 2.0 ** -13  # 1.22e-4: just beyond the 1.0002e-4 between the queries and the cell faces at +-1.0001


@functools.lru_cache(maxsize=None)
def prune_edges():
    """26 queries at (+-1 | 0.25)^3: 1.0002e-4 from the faces at +-1.0001 of both cell sizes, next to 6 faces, 12 edges and 8 corners.  With s the
    direction to the near face(s) and d = 2^-13: own-side points at q - s d f, across points at q + s d g, variant by variant:
      0  f = 1/4, 1/2, 3/4, 7/8, 1 and g = 1: the 5th place is an exact tie between an own point and the point across (the lower index wins)
      1  the same with g = 1 - 2^-5: the point across is strictly closer than the 5th own point
      2  the same with g = 1 + 2^-5: strictly farther
      3  f = 1/16 .. 5/16 and g = 1: the 5th distance is below the distance to the cell across, which may be skipped
      4  the point across on the first float beyond the face (m = 840 ulps of 1.0 from the query per near axis, the face itself at m - 1), own
         points at m/4, m/2, 3m/4, 7m/8 and m + 8 ulps: the point across is the 5th neighbour, and the bound after round 0 (the 5th own point)
         exceeds the box distance of its cell by 2 % only -- a pruning test that is a little too eager skips the cell
    The cell across a face is scanned in round 0; across an edge or a corner in rounds 1 to 3, behind the pruning test."""
    qs, m, layout = [], [], []
    combos = [s for s in itertools.product((-1, 0, 1), repeat=3) if any(s)]
    ulp = 2.0 ** -23
    m_ulps = int(round((float(np.nextafter(CELL1, F32(2.0))) - 1.0) / ulp))  # the first float beyond the face at 1.0001, in ulps of 1.0 from 1.0
    for i, s in enumerate(combos):
        s = np.array(s, F64)
        q = np.where(s != 0, s * 1.0, 0.25)
        v = i % 5
        if v == 4:
            own = [q - s * (k * ulp) for k in (m_ulps // 4, m_ulps // 2, 3 * m_ulps // 4, 7 * m_ulps // 8, m_ulps + 8)]
            across = q + s * (m_ulps * ulp)
        else:
            fs = (1 / 16, 2 / 16, 3 / 16, 4 / 16, 5 / 16) if v == 3 else (1 / 4, 1 / 2, 3 / 4, 7 / 8, 1.0)
            g = {0: 1.0, 1: 1.0 - 2.0 ** -5, 2: 1.0 + 2.0 ** -5, 3: 1.0}[v]
            own = [q - s * PRUNE_D * f for f in fs]
            across = q + s * PRUNE_D * g
        # half of the clusters list the point across first: its index is then the lower one of the tie
        first = (i // 5) % 2 == 0
        pts = [across] + own if first else own + [across]
        layout.append((tuple(int(x) for x in s), v, len(m) + (0 if first else 5)))
        m += pts
        qs.append(q)
    m, qs = np.array(m), np.array(qs)
    assert (m.astype(F32).astype(F64) == m).all() and (qs.astype(F32).astype(F64) == qs).all()
    return _case(m, qs, IDENTITY, ("g1", "g2", "u1"), layout=layout)


@functools.lru_cache(maxsize=None)
def shell():
    """12 queries at the centre region of a half cell with 0 .. 4 points in the inner 27 half cells and the rest in the 98 shell cells, out to the
    corners; along x one point at exactly the gate radius (accepted), one an ulp of d2 inside and one an ulp outside"""
    rng = np.random.default_rng(15)
    c = F64(CELL2)
    offs = [o for o in itertools.product(range(-2, 3), repeat=3) if max(abs(v) for v in o) == 2]
    qs, m, inner = [], [], []
    for i in range(12):
        q = np.array([0.25, 0.25, 8.0 * i + 0.25])
        qs.append(q)
        for _ in range(i % 5):
            m.append(q + (rng.integers(-1, 2, 3) + rng.uniform(-0.2, 0.2, 3)) * c)
        inner.append(i % 5)
        for k in rng.choice(len(offs), 40, replace=False):
            m.append(q + (np.array(offs[k]) + rng.uniform(-0.2, 0.2, 3)) * c)
        m.append(q + np.array([1.0, 0.0, 0.0]))
        m.append(q + np.array([-(1.0 - 2.0 ** -20), 0.0, 0.0]))
        m.append(q + np.array([0.0, 1.0 + 2.0 ** -20, 0.0]))
    m = np.array(m)
    m = m[rng.permutation(len(m))]
    return _case(m, np.array(qs), IDENTITY, ("g1", "g2", "u1"), inner=inner)


RINGS_OUT = (2, 3, 4, 6, 9, 2, 3, 4, 7, 3)  # the Chebyshev cell distance of the 5th neighbour, query by query
FAR_POINTS = np.array([[300.0, 300.0, 300.0], [-300.0, -300.0, -300.0]])  # a bounding box of 600^3 cells: no dense window


@functools.lru_cache(maxsize=None)
def rings_out(hashed):
    """un-gated: the 5th neighbour lies 2, 3, 4 and more than 4 cells away (the ring walk, then knn_grid's window walk); the last query has 2 points in
    its own cell and the rest 3 cells away.  hashed: two far points make the bounding box exceed kMaxWindowCells, the grid has a hash table only and
    the queries beyond kMaxRing end in the brute-force scan."""
    rng = np.random.default_rng(16)
    c = F64(CELL1)
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, -1), (-1, 1, 1), (0, -1, 0), (1, 0, 1), (0, 0, 1), (1, -1, 0)]
    qs, m = [], []
    for i, r in enumerate(RINGS_OUT):
        base = np.array([24.0 * i, 0.0, 0.0])
        q = (base + 0.5) * c
        qs.append(q)
        for _ in range(6):
            m.append((base + r * np.array(dirs[i]) + 0.5 + rng.uniform(-0.3, 0.3, 3)) * c)
        if i == len(RINGS_OUT) - 1:
            for _ in range(2):
                m.append((base + 0.5 + rng.uniform(-0.3, 0.3, 3)) * c)
    m = np.array(m)
    m = m[rng.permutation(len(m))]
    if hashed:
        m = np.concatenate([m, FAR_POINTS])
    return _case(m, np.array(qs), IDENTITY, ("u1",), hashed=bool(hashed))


@functools.lru_cache(maxsize=None)
def out_of_range():
    """finite queries whose cell index is beyond the key range of both cell sizes on at least one axis, on both sides"""
    rng = np.random.default_rng(17)
    m = rng.uniform(-3.0, 3.0, (200, 3))
    big = 1.2e6  # 1.2e6 and 2.4e6 cells
    q = [[big, 0, 0], [-big, 0, 0], [0, big, 0], [0, -big, 0], [0.5, 0.5, big], [0.5, 0.5, -big], [big, -big, big], [3.0e7, 1.0, 1.0], [1.0, -3.0e37, 1.0]]
    return _case(m, q, IDENTITY, ("g1", "g2", "u1"))


# ---- boundary_filing ---------------------------------------------------------------------------------------------------------------------
def _step(x, j):
    """x moved by j ulps away from zero (j < 0: towards zero)"""
    return (np.asarray(x, F32).view(np.int32) + np.int32(j)).view(F32)


def boundary_pairs(cell, ks, d2_limit):
    """(q, p) float32 pairs next to the cell faces k cell, k in ks, within 3 ulps of them: the query's filing of q and the FLOAT filing of p differ by two
    cells while the float d2 of the pair is not above d2_limit (a double).  Sorted by |k|."""
    ks = np.asarray(ks, np.int64)
    ks = ks[np.abs(ks) >= 3]
    c = float(F64(cell))
    j = np.arange(-3, 4)
    out = []
    for dk in (-1, 1):
        p = _step(F32(ks[:, None] * c), j[None, :])            # (nk, 7) around face k
        q = _step(F32((ks[:, None] + dk) * c), j[None, :])     # (nk, 7) around face k + dk
        fp, fq = file_float(p, cell), file_query(q, cell)
        d = q[:, None, :] - p[:, :, None]                      # (nk, jp, jq) float32
        d2 = (d * d).astype(F64)
        hit = (np.abs(fq[:, None, :] - fp[:, :, None]) == 2) & (d2 <= d2_limit)
        for a, b, e in zip(*np.nonzero(hit)):
            out.append((abs(int(ks[a])), float(q[a, e]), float(p[a, b])))
    out.sort()
    return [(F32(qq), F32(pp)) for _, qq, pp in out]


def _fillers(d2_pair, hi, base):
    """five float32 y coordinates base + dy whose d2 = dy dy lies strictly between d2_pair and hi, in increasing order; None if the gap is too narrow"""
    ys = []
    for t in np.linspace(float(d2_pair), float(hi), 9)[2:7]:
        y = F32(float(base) + np.sqrt(t))
        dy = y - F32(base)
        d2 = F64(dy * dy)
        if not (float(d2_pair) < d2 < hi) or (ys and y <= ys[-1]):
            return None
        ys.append(y)
    return ys


def _boundary_scene(cell, pairs, fillers_of, take):
    """pairs along x, each in its own slab of z (16 m apart) with y at the middle of cell 0; the pair's fillers at the query's x"""
    y0 = F32(0.5) if float(cell) > 0.75 else F32(0.25)  # the middle of cell 0 for either cell size
    m, q, rows = [], [], []
    for qx, px in pairs:
        dx = F32(qx) - F32(px)
        ys = fillers_of(dx * dx, y0)
        if ys is None:
            continue
        z = F32(16.0 * len(q) + float(y0))
        rows.append((len(q), len(m), float(qx), float(px)))  # query index, index of the pair's point
        m.append([px, y0, z])
        m += [[qx, y, z] for y in ys]
        q.append([qx, y0, z])
        if len(q) == take:
            break
    return m, q, rows


def _spread(pairs, n):
    """up to n pairs spread over the sorted list (small and large |x|, both signs as they come)"""
    if len(pairs) <= n:
        return pairs
    return [pairs[i] for i in np.linspace(0, len(pairs) - 1, n).astype(int)]


@functools.lru_cache(maxsize=None)
def boundary_filing(setting):
    """u1 / g2: pairs within +-700 cells whose float d2 is under the certification limit cell^2 (1 - 1e-5) -- with five fillers between the pair's d2
    and that limit the 27 cells (u1) or stage 1 (g2) certify a list without the pair's point if the point was filed one cell too far.
    g1: pairs near +-3998 cells; every one found is exactly the gate radius apart (the floats there are 2.4e-4 apart), so the pair's point is the 5th
    neighbour behind four fillers strictly inside the gate: a search that misses it reports four neighbours where five are within the gate."""
    cell = SETTINGS[setting][0]
    if setting == "g1":
        ks = np.concatenate([np.arange(-4100, -3899), np.arange(3900, 4101)])
        limit = float(GATE)
        fillers_of = lambda d2, y0: [F32(float(y0) + np.sqrt(t)) for t in (0.6, 0.7, 0.8, 0.9)] if float(d2) > 0.95 else None
    else:
        ks = np.arange(-700, 701)
        limit = certify_limit(cell)
        fillers_of = lambda d2, y0: _fillers(d2, limit, y0)
    pairs = boundary_pairs(cell, ks, limit)
    m, q, rows = _boundary_scene(cell, _spread(pairs, 8), fillers_of, 8)
    return _case(m, q, IDENTITY, (setting,), rows=rows, n_pairs=len(pairs), cell=cell, limit=limit)


CASES = {
    "uniform": uniform, "lattice_ties": lattice_ties, "small_map": small_map, "prune_edges": prune_edges, "shell": shell, "out_of_range": out_of_range,
    "quad_tails_g1": functools.partial(quad_tails, "g1"), "quad_tails_g2": functools.partial(quad_tails, "g2"), "quad_tails_u1": functools.partial(quad_tails, "u1"),
    "rings_out": functools.partial(rings_out, False), "rings_out_hashed": functools.partial(rings_out, True),
    "boundary_filing_u1": functools.partial(boundary_filing, "u1"), "boundary_filing_g2": functools.partial(boundary_filing, "g2"),
    "boundary_filing_g1": functools.partial(boundary_filing, "g1"),
}
K1_CASES = ("uniform", "lattice_ties", "quad_tails_g1", "small_map", "out_of_range")


def runs():
    """every (case, setting) pair of the K = 5 matrix"""
    return [(name, s) for name, fn in CASES.items() for s in fn().settings]
