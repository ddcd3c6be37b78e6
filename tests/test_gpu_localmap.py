"""The device local-map source (include/fls_localmap.h, csrc/localmap.hpp, csrc/kernels_localmap.hpp) on the GPU.  The expected values never
come from the store: the crop box, the tile keys, the evolution of the resident tile set and the stitch order are restated here in numpy
(float32 comparisons, float64 floor), the filtered clouds are the oracle's VoxelGrid, and a hand-over is held against
fls_add_cloud_to_local_map of the rows the store itself reports -- the exported maps byte for byte, the next Match and the fitness score bit
for bit."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg
from funny_lidar_slam_amd.localmap import LocalMapSource
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
T0 = np.array([123.456789, -87.654321, 3.21])  # a translation no float holds


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"


def pose(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def same_rows(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the models ------------------------------------------------------------------------------------------------------------------------------
def corners(t):
    e = np.concatenate([np.asarray(t, np.float64) - 100.0, np.asarray(t, np.float64) + 100.0])
    return e, e[:3].astype(F32), e[3:].astype(F32)


def model_crop(rows, t):
    _, mn, mx = corners(t)
    xyz = rows[:, :3]
    return rows[~((xyz < mn).any(1) | (xyz > mx).any(1))]


def model_need(edge, t, force=False):
    if edge is None or force:
        return True
    for i in range(3):
        if abs(t[i] - edge[i]) > 50.0 and abs(t[i] - edge[i + 3]) > 50.0:
            continue
        return True
    return False


def tile_keys(rows, g):
    x, y = rows[:, 0].astype(np.float64), rows[:, 1].astype(np.float64)
    return np.floor((x - g / 2) / g).astype(np.int64), np.floor((y - g / 2) / g).astype(np.int64)


def model_split(rows, g):
    """[(gx, gy, rows of the tile in cloud order)] in LessGridIndex order"""
    gx, gy = tile_keys(rows, g)
    order = np.lexsort((np.arange(len(rows)), gy, gx))  # stable by construction
    out = []
    for k in order:
        if not out or (out[-1][0], out[-1][1]) != (gx[k], gy[k]):
            out.append([int(gx[k]), int(gy[k]), []])
        out[-1][2].append(k)
    return [(a, b, rows[np.asarray(ix)]) for a, b, ix in out]


class TileModel:
    """LoadLocalMap's tile branch (src/slam/localization.cpp:309-365) with the store's two cached forms per tile"""

    def __init__(self, tiles, g):
        self.tiles, self.g = tiles, g  # {(gx, gy): rows}
        self.resident, self.cache, self.local, self.leaf = set(), {k: [] for k in tiles}, np.zeros((0, 4), F32), None
        self.filters = self.hits = 0

    def form(self, k, leaf, count=True):
        if not leaf > 0:
            return self.tiles[k]
        for lf, rows in self.cache[k]:
            if lf == leaf:
                self.hits += count
                return rows
        rows = O.voxel_grid(self.tiles[k], leaf)
        self.filters += 1
        self.cache[k] = (self.cache[k] + [(leaf, rows)])[-2:]
        return rows

    def step(self, t, leaf):
        g = self.g
        cx, cy = int(np.floor((t[0] - g / 2) / g)), int(np.floor((t[1] - g / 2) / g))
        updated, entered = False, []
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                k = (cx + dx, cy + dy)
                if k in self.tiles and k not in self.resident:
                    self.resident.add(k)
                    entered.append(k)
                    updated = True
        for k in sorted(self.resident):
            if float(np.hypot(F32(k[0] - cx), F32(k[1] - cy))) > 2:
                self.resident.discard(k)
                updated = True
        other_leaf = bool(self.resident) and leaf != self.leaf
        for k in entered:
            self.form(k, leaf)
        if other_leaf:
            for k in sorted(self.resident):
                if k not in entered:
                    self.form(k, leaf)
        if updated or other_leaf:
            parts = [self.form(k, leaf, count=False) for k in sorted(self.resident)]
            self.local = np.concatenate(parts) if parts else np.zeros((0, 4), F32)
            self.leaf = leaf
        return updated or other_leaf


# ---- crop --------------------------------------------------------------------------------------------------------------------------------
def crop_cloud(n, seed, ends_kept):
    """uniform in a 400 x 400 x 60 m box around T0, with points planted on and next to the six faces and chosen first / last points"""
    rng = np.random.default_rng(seed)
    rows = np.empty((n, 4), F32)
    rows[:, :3] = (T0 + rng.uniform(-1, 1, (n, 3)) * np.array([200.0, 200.0, 30.0])).astype(F32)
    rows[:, 3] = rng.uniform(0, 255, n).astype(F32)
    _, mn, mx = corners(T0)
    centre = T0.astype(F32)
    planted = []
    for a in range(3):
        for face, out_dir in ((mn[a], -np.inf), (mx[a], np.inf)):
            for v in (face, np.nextafter(face, F32(out_dir)), np.nextafter(face, F32(-out_dir))):
                p = centre.copy()
                p[a] = v
                planted.append(p)
    planted = np.asarray(planted, F32)[rng.permutation(18)]
    slots = rng.permutation(np.arange(1, n - 1))[: len(planted)] if n > 2 else np.array([], np.int64)
    rows[slots, :3] = planted[: len(slots)]
    if n == 1:
        rows[0, :3] = planted[0] if ends_kept else centre + F32(500)
        if ends_kept:
            rows[0, 0], rows[0, 1], rows[0, 2] = centre[0], mx[1], centre[2]  # the single point lies on a face
    else:
        rows[[0, n - 1], :3] = centre if ends_kept else centre + F32(500)
    return rows


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097, 20000, 300000])
def test_crop_equals_the_model(n):
    src = LocalMapSource()
    for ends_kept in (True, False):
        rows = crop_cloud(n, 100 + n, ends_kept)
        assert src.SetGlobal(rows) == n
        want = model_crop(rows, T0)
        assert (len(want) > 0) == (ends_kept or n > 2)
        upd, n_local = src.Crop(pose(T0))
        got = src.Local()
        assert upd and n_local == len(want) and same_rows(got, want), (n, ends_kept, n_local, len(want))
        if n > 2:
            _, mn, mx = corners(T0)
            on_face = ((got[:, :3] == mn) | (got[:, :3] == mx)).any(1).sum()
            assert on_face == min(6, n - 2) or n < 20, on_face  # the planted face points are kept
    assert src.Stat(3) == 2 and src.Stat(4) == 0 and src.Stat(0) == n
    src.close()


def test_crop_all_inside_all_outside_and_a_filtered_global_map():
    rng = np.random.default_rng(5)
    rows = np.empty((5000, 4), F32)
    rows[:, :3] = (T0 + rng.uniform(-1, 1, (5000, 3)) * np.array([99.0, 99.0, 20.0])).astype(F32)
    rows[:, 3] = np.arange(5000, dtype=F32)
    src = LocalMapSource()
    src.SetGlobal(rows)
    assert src.Crop(pose(T0)) == (True, 5000) and same_rows(src.Local(), rows)
    far = T0 + np.array([1000.0, 0.0, 0.0])
    assert src.Crop(pose(far)) == (False, 5000)  # far outside the old box both distances exceed the margin again: the reference's rule, kept
    assert src.Crop(pose(far), force=True) == (True, 0) and src.Local().shape == (0, 4)  # an empty cut is a valid local map
    m = reg.make_matcher("PointToPlane_IVOX", reg.YAML_NCLT_IVOX, is_localization_mode=True)
    with pytest.raises(_lib.FlsError) as e:
        src.AddTo(m)
    assert e.value.status == _lib.FLS_ERR_STATE and src.Stat(9) == src.Stat(10) == 0
    m.close()
    # LoadGlobalMap + VoxelGridCloud(global, 0.3): the stored cloud is the oracle's filter output, the cut is taken from it
    dense = crop_cloud(40000, 9, True)
    dense[:, :3] = (T0 + (dense[:, :3] - T0.astype(F32)) * np.array([0.55, 0.55, 0.01], F32)).astype(F32)  # 220 x 220 x 0.6 m: leaves share points, the box still cuts
    want_global = O.voxel_grid(dense, 0.3)
    assert src.SetGlobal(dense, 0.3) == len(want_global) < len(dense)
    want = model_crop(want_global, T0)
    upd, n_local = src.Crop(pose(T0))
    assert upd and 0 < n_local == len(want) < len(want_global) and same_rows(src.Local(), want)
    assert src.Stat(7) == 0  # the device filter took it
    # a cloud the device filter declines (a NaN point): the exact host filter, counted
    dense[7, 1] = np.nan
    assert src.SetGlobal(dense, 0.3) == len(O.voxel_grid(dense, 0.3)) and src.Stat(7) == 1
    with pytest.raises(_lib.FlsError) as e:
        src.SetGlobal(dense, 0.0)  # unfiltered clouds hold finite points only
    assert e.value.status == _lib.FLS_ERR_RANGE and src.Stat(0) == len(O.voxel_grid(dense, 0.3))  # the store is what it was
    src.close()


def test_hysteresis_walk_force_and_reset():
    rng = np.random.default_rng(11)
    rows = np.empty((20000, 4), F32)
    rows[:, :3] = rng.uniform(-1, 1, (20000, 3)) * np.array([400.0, 400.0, 150.0])
    rows[:, 3] = rng.uniform(0, 1, 20000)
    src = LocalMapSource()
    src.SetGlobal(rows)
    walk = [(0, 0, 0), (30, 0, 0), (49.5, 0, 0), (50.0, 0, 0), (60, 40, 0), (60, 49.9, 0), (60, 50.5, 0), (60, 60, 30), (60, 60, 49), (60, 60, 51),
            (-45, 60, 51), (100, 100, 60)]
    edge, local, runs, skips = None, None, 0, 0
    for k, t in enumerate(walk):
        t = np.asarray(t, np.float64) + np.array([0.123, -0.456, 0.789])
        need = model_need(edge, t)
        if need:
            edge, _, _ = corners(t)
            local = model_crop(rows, t)
        runs, skips = runs + need, skips + (not need)
        upd, n_local = src.Crop(pose(t))
        assert upd == need and n_local == len(local) and same_rows(src.Local(), local), (k, t)  # a skipped call leaves the local map as it was
        assert (src.Stat(3), src.Stat(4)) == (runs, skips), k
    assert runs >= 5 and skips >= 5
    t = np.asarray(walk[-1], np.float64) + 1.0
    assert not model_need(edge, t) and src.Crop(pose(t))[0] is False
    upd, n_local = src.Crop(pose(t), force=True)
    assert upd and same_rows(src.Local(), model_crop(rows, t))
    assert src.Crop(pose(t))[0] is False
    before = src.Local()
    src.Reset()
    assert same_rows(src.Local(), before)  # reset forgets the edges, not the local map
    assert src.Crop(pose(t))[0] is True and src.Stat(3) == runs + 2 and src.Stat(4) == skips + 2
    src.close()


# ---- split -------------------------------------------------------------------------------------------------------------------------------
def split_cloud(n, g, seed):
    rng = np.random.default_rng(seed)
    rows = np.empty((n, 4), F32)
    rows[:, :3] = rng.uniform(-1, 1, (n, 3)) * np.array([260.0, 190.0, 10.0]) + np.array([-40.0, 25.0, 0.0])
    rows[:, 3] = rng.uniform(0, 255, n)
    planted = []
    for k in (-2, 0, 1):
        b = F32(g / 2 + k * g)
        for v in (b, np.nextafter(b, F32(-np.inf)), np.nextafter(b, F32(np.inf))):
            planted += [(v, F32(1.5)), (F32(-2.5), v), (v, v)]
    m = min(len(planted), n)
    rows[rng.permutation(n)[:m], :2] = np.asarray(planted, F32)[:m]
    return rows


def check_tiles(src, want):
    idx, cnt = src.Tiles()
    assert [tuple(r) for r in idx] == [(a, b) for a, b, _ in want] and list(cnt) == [len(r) for _, _, r in want]
    for a, b, r in want:
        assert same_rows(src.GetTile(a, b), r), (a, b)


@pytest.mark.parametrize("n,g", [(20000, 100.0), (20000, 37.5), (257, 100.0), (257, 37.5), (1, 100.0), (1, 37.5)])
def test_split_equals_the_model(n, g):
    rows = split_cloud(n, g, 3 * n + int(g))
    want = model_split(rows, g)
    assert n == 1 or len(want) > 4
    allrows = np.concatenate([r for _, _, r in want])
    assert same_rows(allrows[np.lexsort(allrows.T)], rows[np.lexsort(rows.T)])  # a permutation of the input
    src = LocalMapSource()
    src.SetGlobal(rows)
    assert src.Split(g) == len(want) and src.Stat(1) == len(want) and src.Stat(2) == n
    check_tiles(src, want)
    # the same tiles added one by one answer identically
    other = LocalMapSource()
    for a, b, r in reversed(want):
        other.AddTile(g, a, b, r)
    check_tiles(other, want)
    with pytest.raises(_lib.FlsError) as e:
        other.AddTile(g + 1.0, 0, 0, rows[:1])  # another grid size than the one in force
    assert e.value.status == _lib.FLS_ERR_INVALID
    with pytest.raises(_lib.FlsError) as e:
        other.GetTile(10 ** 6, 0)
    assert e.value.status == _lib.FLS_ERR_INVALID
    src.close(); other.close()


def test_split_of_a_single_tile_cloud():
    rng = np.random.default_rng(2)
    rows = np.empty((3000, 4), F32)
    rows[:, :3] = rng.uniform(-40, 40, (3000, 3)) + np.array([100.0, -200.0, 0.0])  # inside tile (0, -3) of a 100 m grid
    rows[:, 3] = np.arange(3000)
    src = LocalMapSource()
    src.SetGlobal(rows)
    assert src.Split(100.0) == 1
    check_tiles(src, [(0, -3, rows)])
    src.close()


def test_split_refuses_more_points_than_the_sort_takes():
    """4,194,304 points is the radix sort's limit: one more is FLS_ERR_INVALID and the tiles stay what they were (the crop has no such limit)"""
    n = 4194304 + 1
    rows = np.zeros((n, 4), F32)
    rows[:, 0] = np.arange(n, dtype=np.float64) * (180.0 / n)
    src = LocalMapSource()
    src.AddTile(100.0, 0, 0, rows[:10])
    assert src.SetGlobal(rows) == n and src.Stat(1) == 0  # (a new global map clears the tiles)
    src.AddTile(100.0, 0, 0, rows[:10])
    with pytest.raises(_lib.FlsError) as e:
        src.Split(100.0)
    assert e.value.status == _lib.FLS_ERR_INVALID and src.Stat(1) == 1 and src.Stat(2) == 10
    t = np.array([90.0, 0.0, 0.0])
    upd, n_local = src.Crop(pose(t))
    assert upd and n_local == n  # every point lies inside the box
    src.close()


# ---- the tile branch -------------------------------------------------------------------------------------------------------------------------
def test_tile_walk_equals_the_model():
    g, rng = 50.0, np.random.default_rng(21)
    tiles = {}
    for gx in range(5):
        for gy in range(5):
            if (gx, gy) in ((1, 3), (3, 0)):  # two holes
                continue
            n = int(rng.integers(300, 900))
            r = np.empty((n, 4), F32)
            r[:, :3] = rng.uniform(0, 1, (n, 3)) * np.array([g, g, 4.0]) + np.array([g / 2 + gx * g, g / 2 + gy * g, -2.0])
            r[:, 3] = rng.uniform(0, 255, n)
            tiles[(gx, gy)] = r
    src = LocalMapSource()
    for (gx, gy), r in tiles.items():
        src.AddTile(g, gx, gy, r)
    model = TileModel(tiles, g)
    centre = lambda gx, gy: np.array([(gx + 1) * g - 3.25, (gy + 1) * g + 7.5, 0.4])
    #       start    one tile on  still there   a jump of three  back to the first tiles  the other leaf   the first leaf again
    walk = [((1, 1), 0.5), ((2, 1), 0.5), ((2, 1), 0.5), ((2, 4), 0.5), ((1, 1), 0.5), ((1, 1), 0.8), ((1, 1), 0.5), ((4, 4), 0.0)]
    seen_updates = []
    for k, (c, leaf) in enumerate(walk):
        hits_before = src.Stat(6)
        want_upd = model.step(centre(*c), leaf)
        upd, n_local = src.LoadTiles(pose(centre(*c)), leaf)
        assert upd == want_upd and n_local == len(model.local), (k, upd, want_upd, n_local, len(model.local))
        assert same_rows(src.Local(), model.local), k
        assert (src.Stat(5), src.Stat(6)) == (model.filters, model.hits), k
        seen_updates.append((upd, src.Stat(6) - hits_before))
    assert [u for u, _ in seen_updates] == [True, True, False, True, True, True, True, True]
    assert seen_updates[4][1] > 0  # the tiles left behind by the jump come back from the cache
    assert src.Stat(8) == 7
    # the filtered form of a tile, on request
    assert same_rows(src.GetTile(0, 0, 0.5), O.voxel_grid(tiles[(0, 0)], 0.5))
    src.Reset()
    assert src.LoadTiles(pose(centre(4, 4)), 0.0)[0] is True  # the resident set was forgotten
    src.close()


# ---- the hand-over ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def world():
    """a street scene 240 m long and 60 m wide: ground and walls, dense enough for plane fits"""
    rng = np.random.default_rng(77)
    n = 200000
    k = n // 3
    ground = np.stack([rng.uniform(-120, 120, k), rng.uniform(-30, 30, k), np.full(k, -1.8)], 1)
    wall_x = np.stack([np.round(rng.uniform(-120, 120, k) / 20.0) * 20.0 + 3.0, rng.uniform(-30, 30, k), rng.uniform(-1.8, 4.0, k)], 1)
    m = n - 2 * k
    wall_y = np.stack([rng.uniform(-120, 120, m), np.where(rng.uniform(0, 1, m) < 0.5, -22.0, 17.0), rng.uniform(-1.8, 4.0, m)], 1)
    xyz = np.concatenate([ground, wall_x, wall_y]) + rng.normal(0, 0.01, (n, 3))
    rows = np.empty((n, 4), F32)
    rows[:, :3] = xyz[rng.permutation(n)]
    rows[:, 3] = rng.uniform(0, 255, n)
    return rows


def scan_at(t, seed):
    rows = world()
    near = np.flatnonzero(np.linalg.norm(rows[:, :3].astype(np.float64) - t, axis=1) < 25.0)
    pick = np.random.default_rng(seed).permutation(near)[:3000]
    return (rows[pick, :3].astype(np.float64) - t).astype(F32)


MODES = {"ivox": ("PointToPlane_IVOX", reg.YAML_NCLT_IVOX, 140), "ndt": ("IncrementalNDT", reg.YAML_NCLT_NDT, 150), "icp": ("IcpOptimized", reg.YAML_NCLT_ICP, None)}


def fitness_of(m):
    try:
        return F32(m.GetFitnessScore(2.0)).view(np.uint32)
    except _lib.FlsError as e:
        return e.status


def handover_check(kind, loc, device_path):
    """A gets fls_add_cloud_to_local_map of the rows, B the hand-over: twice in a row for a localization handle (the reload after the walk
    has moved 60 m, then a second reload), once for a mapping handle's first insert"""
    mode, y, build_slot = MODES[kind]
    src = LocalMapSource()
    src.SetGlobal(world())
    a = reg.make_matcher(mode, y, is_localization_mode=loc)
    b = reg.make_matcher(mode, y, is_localization_mode=loc)
    walk = [np.array([-25.3, 1.7, 0.2]), np.array([34.7, 1.7, 0.2]), np.array([34.7, 1.7, 0.2])] if loc else [np.array([-25.3, 1.7, 0.2])]
    for k, t in enumerate(walk):
        upd, n_local = src.Crop(pose(t), force=(k == 2))
        assert upd and 50000 < n_local < len(world()), (k, n_local)
        rows = src.Local()
        assert same_rows(rows, model_crop(world(), t))
        builds = b.map_size(build_slot) if build_slot else 0
        a.AddCloudToLocalMap([rows])
        src.AddTo(b)
        assert (src.Stat(9), src.Stat(10)) == ((k + 1, 0) if device_path else (0, k + 1)), (kind, k)
        if build_slot:
            assert b.map_size(build_slot) == builds + (1 if device_path else 0), (kind, k)
        ea, eb = a.ExportMap(), b.ExportMap()
        assert ea.shape == eb.shape and np.array_equal(ea, eb), (kind, k)
        if kind == "ndt":
            n = a.MapImageBytes()
            ia, ib = np.zeros(n, np.uint8), np.ones(n, np.uint8)
            assert n == b.MapImageBytes() and n > 64
            a.ExportMapImage(ia.ctypes.data, n, False); b.ExportMapImage(ib.ctypes.data, n, False)
            assert np.array_equal(ia, ib), k
        assert a.map_size() == b.map_size() > 0
        scan = scan_at(t, 50 + k)
        Ta, Tb = pose(t + np.array([0.08, -0.05, 0.03])), pose(t + np.array([0.08, -0.05, 0.03]))
        oka = a.Match(reg.PointcloudCluster(planar_cloud_=scan, ordered_cloud_=scan), Ta, update_map=False)
        okb = b.Match(reg.PointcloudCluster(planar_cloud_=scan, ordered_cloud_=scan), Tb, update_map=False)
        assert oka == okb and np.array_equal(Ta.view(np.uint64), Tb.view(np.uint64)), (kind, k)
        assert (a.stats.iterations, a.stats.n_valid) == (b.stats.iterations, b.stats.n_valid) and a.stats.n_valid > 100, (kind, k, a.stats.n_valid)
        assert np.linalg.norm(Ta[:3, 3] - t) < 0.05, (kind, k, Ta[:3, 3] - t)  # and the registration found the scan's true place
        fa, fb = fitness_of(a), fitness_of(b)
        assert fa == fb and (not loc or fa > 0), (kind, k, fa, fb)
    a.close(); b.close(); src.close()
    return True


@pytest.mark.parametrize("kind,loc", [("ivox", True), ("ndt", True), ("ivox", False), ("ndt", False)])
def test_handover_equals_the_host_entry_point(kind, loc):
    assert handover_check(kind, loc, device_path=True)


@pytest.mark.parametrize("kind", ["ivox", "ndt"])
def test_declined_builds_go_through_the_host_entry_point(kind):
    """FLS_IVOX_DEVICE_BUILD=0 / FLS_NDT_DEVICE_BUILD=0 are read when the library creates a handle: a child process"""
    env = dict(os.environ, FLS_IVOX_DEVICE_BUILD="0", FLS_NDT_DEVICE_BUILD="0")
    code = f"from tests.test_gpu_localmap import handover_check; print('declined path equal:', handover_check({kind!r}, True, False))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "declined path equal: True" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_other_kinds_take_the_fallback():
    assert handover_check("icp", True, device_path=False)


def test_the_matcher_keeps_its_map_when_the_store_moves_on():
    src = LocalMapSource()
    src.SetGlobal(world())
    for kind in ("ivox", "ndt"):
        mode, y, _ = MODES[kind]
        m = reg.make_matcher(mode, y, is_localization_mode=True)
        t = np.array([-25.3, 1.7, 0.2])
        src.Crop(pose(t), force=True)
        first = src.Local()
        src.AddTo(m)
        before = m.ExportMap()
        upd, _ = src.Crop(pose(t + np.array([80.0, 0.0, 0.0])))
        assert upd and not same_rows(src.Local(), first)
        assert np.array_equal(m.ExportMap(), before), kind  # until its next add the matcher's map does not change
        src.AddTo(m)
        assert not np.array_equal(m.ExportMap(), before), kind
        m.close()
    src.close()
