"""Constructed update histories of the iVox map, and what they are compared with: a plain sequential model of IVoxMap::AddPoints as
LoamPointToPlaneIVOX::AddCloudToLocalMap calls it (src/ivox_map/ivox_map.cpp:122-143; every "points_to_add" point in source order, then every
"point_no_need_downsample" point), codecs of the FLSIVOX1 blob (include/fls_map_ivox.h) and of the flat kNN-side image FLSIMG01
(csrc/ivox_image.hpp: IvoxImage::FlatHeader, flat_bytes, export_flat), and check_image, the checker of the invariant csrc/device_common.hpp states
for the brick image: a halo cell equals the interior cell it mirrors, and a brick exists whenever one of its interior or face / edge halo cells
is occupied.  No GPU is needed for anything here: tests/test_ivox_update_cases.py ties the model to the CPU oracle on every history and makes the
checker fail on purpose, tests/test_gpu_ivox_update.py drives the histories through fls_debug_ivox_add_points (include/fls_debug_ivox_update.h)."""
import collections
import functools

import numpy as np

from tests import evict_pin

KEY_LIMIT = (1 << 20) - 2          # device_common.hpp kKeyLimit
DEFAULT_CAPACITY = 1000000         # InitIVox
CHAIN_MAX_POINTS = 262144          # kernels_ivox_update.hpp kUpdMaxBlocks * kUpdBlock
UPD_BLOCK = 256                    # kUpdBlock
FINISH_MAX_K = 1024                # kUpdFinishMaxK
EV_BLOCK = 1024                    # kEvBlock
EV_MAX_RECREATE = 1024             # kEvMaxRecreate
FIRST_POOL_BRICKS = 256            # the smallest brick pool (IvoxMap::build_brick_pool / IvoxImage::build_from_ivox: max(n_bricks_cap, 256))
BRICK_SIDE, BRICK_STORED, BRICK_STRIDE = 8, 10, 1024
BRICK_PENDING, BRICK_INVALID = 0xFFFFFFFF, 0xFFFFFFFE
EMPTY_KEY = 0xFFFFFFFFFFFFFFFF
KIND_P2PLANE_IVOX = 1
FLS_OK, FLS_ERR_RANGE = 0, -3
NO_CHAIN = 0xFFFFFFFF

HDR = np.dtype([("magic", "S8"), ("version", "<u4"), ("kind", "<u4"), ("resolution", "<f4"), ("is_first", "<u4"), ("capacity", "<u8"), ("n_voxels", "<u8"),
                ("n_points", "<u8"), ("next_id", "<i8")])
VOX = np.dtype([("key", "<u8"), ("count", "<u4"), ("pad", "<u4")])
PT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("id", "<i4")])
IMG = np.dtype([("magic", "S8"), ("kind", "<u4"), ("want_hash", "<u4"), ("have_bricks", "<u4"), ("is_first", "<u4"), ("use_dense", "<u4"), ("mask", "<u4"),
                ("dir_mask", "<u4"), ("pad", "<u4"), ("resolution", "<f4"), ("pad_f", "<f4"), ("used", "<u8"), ("n_pts_live", "<u8"), ("n_bricks_live", "<u8"),
                ("n_bricks_cap", "<u8"), ("total_bytes", "<u8")])
DIR = np.dtype([("key", "<u8"), ("begin", "<u4"), ("count", "<u4")])
CELL = np.dtype([("begin", "<u4"), ("count", "<u4")])


# ------------------------------------------------------------------ keys ------------------------------------------------------------------
def keys_of(points):
    """IVoxMap::Pos2Grid: the float32 product p * 2, rounded half away from zero (np.round rounds half to even: wrong at +-0.25, +-0.75, ...).
    Returns (int64 keys (n, 3), inside the key range (n,))."""
    x = np.asarray(points, np.float32).reshape(-1, 3) * np.float32(2.0)
    assert x.dtype == np.float32
    xd = x.astype(np.float64)
    k = np.sign(xd) * np.floor(np.abs(xd) + 0.5)  # (|x| + 0.5 is exact in float64)
    return k.astype(np.int64), (np.abs(k) < KEY_LIMIT).all(axis=1)


def pack_key(x, y, z):
    return ((int(x) & 0x1FFFFF) << 42) | ((int(y) & 0x1FFFFF) << 21) | (int(z) & 0x1FFFFF)


def unpack_key(k):
    def sx(v):
        return v - (1 << 21) if v & (1 << 20) else v
    k = int(k)
    return sx((k >> 42) & 0x1FFFFF), sx((k >> 21) & 0x1FFFFF), sx(k & 0x1FFFFF)


def mirrors_of(key):
    """brick_for_each_mirror: the (dx, dy, dz) of the bricks whose halo mirrors voxel `key` -- every face / edge combination, no corner"""
    e = [-1 if (c & 7) == 0 else 1 if (c & 7) == 7 else 0 for c in key]
    out = []
    for m in range(1, 7):
        if any((m >> a) & 1 and not e[a] for a in range(3)):
            continue
        out.append(tuple(e[a] if (m >> a) & 1 else 0 for a in range(3)))
    return out


def bricks_of(keys):
    """the bricks the voxels `keys` need: their own and the ones that mirror them"""
    out = set()
    for k in keys:
        b = (k[0] >> 3, k[1] >> 3, k[2] >> 3)
        out.add(b)
        for d in mirrors_of(k):
            out.add((b[0] + d[0], b[1] + d[1], b[2] + d[2]))
    return out


# ------------------------------------------------------------------ model -----------------------------------------------------------------
class BatchInfo:
    """what one batch did to the model"""

    def __init__(self):
        self.n_source = self.inserted = self.n_alive_before = 0
        self.evictions = []        # keys, in eviction order
        self.n_recreated = 0       # creations of a voxel this batch evicted before
        self.evicted_own = False   # an eviction took a voxel this batch had created or touched before
        self.outside = False       # an inserted point's key is beyond the limit
        self.rc = FLS_OK           # what the sequential host path returns (HostIvox::add_points: each of the two lists all-or-nothing)
        self.k = collections.Counter()  # points inserted per voxel
        self.short_chain = False   # the batch cannot reach the capacity: n_alive + n_source < capacity
        self.bricks = 0            # bricks the alive voxels before and every voxel of the batch need (own + mirrors)

    @property
    def n_evicted(self):
        return len(self.evictions)

    @property
    def device_can_apply(self):
        """ivox_evict_select applies a batch when every voxel it evicts was neither created nor touched by the batch before its eviction, and at most
        kEvMaxRecreate voxels are evicted and created again (tests/host/evict_conflict_model_test.cpp: the same rule); ivox_upd_seq refuses a key
        beyond the limit before that"""
        return not self.outside and not self.evicted_own and self.n_recreated <= EV_MAX_RECREATE

    @property
    def refusal(self):
        """None, or why the device refuses: "outside" (slot 121), "need_host" (no reason slot), "conflict" (slot 119)"""
        if self.outside:
            return "outside"
        if self.evicted_own:
            return "need_host"
        return "conflict" if self.n_recreated > EV_MAX_RECREATE else None


class Model:
    """evict_pin.sequential_model carrying points and ids: vox maps key -> list of ids, least recently touched first; pts[id] is the point"""

    def __init__(self, capacity=None):
        self.capacity = DEFAULT_CAPACITY if capacity is None else int(capacity)
        self.vox = collections.OrderedDict()
        self.pts = np.zeros((0, 3), np.float32)
        self.next_id = 0

    def insert(self, points, codes=None):
        points = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
        codes = np.ones(len(points), np.uint8) if codes is None else np.asarray(codes, np.uint8)
        assert len(codes) == len(points) and (codes <= 2).all()
        keys, ok = keys_of(points)
        info = BatchInfo()
        info.n_source, info.n_alive_before = len(codes), len(self.vox)
        info.short_chain = info.n_alive_before + info.n_source < self.capacity
        lists = [np.flatnonzero(codes == 1), np.flatnonzero(codes == 2)]
        info.outside = not (ok[lists[0]].all() and ok[lists[1]].all())
        taken = []
        for idx in lists:
            if not ok[idx].all():
                info.rc = FLS_ERR_RANGE
                break
            taken.append(idx)
        order = np.concatenate(taken) if taken else np.zeros(0, np.int64)
        kt = list(map(tuple, keys[order].tolist()))
        info.bricks = len(bricks_of(set(self.vox) | set(kt)))
        vox, cap, base = self.vox, self.capacity, self.next_id
        touched, evicted_now = set(), set()
        for r, k in enumerate(kt):
            ids = vox.get(k)
            if ids is None:
                vox[k] = [base + r]
                info.n_recreated += k in evicted_now
                if len(vox) >= cap:
                    b, _ = vox.popitem(last=False)
                    info.evictions.append(b)
                    evicted_now.add(b)
                    info.evicted_own |= b in touched
            else:
                ids.append(base + r)
                vox.move_to_end(k)
            touched.add(k)
        info.k = collections.Counter(kt)
        info.inserted = len(kt)
        self.pts = np.concatenate([self.pts, points[order]])
        self.next_id += len(kt)
        return info

    @property
    def n_alive(self):
        return len(self.vox)

    @property
    def n_points(self):
        return sum(len(v) for v in self.vox.values())

    def voxels(self):
        """key -> the voxel's points as PT records in insertion order; least recently touched voxel first"""
        out = collections.OrderedDict()
        for k, ids in self.vox.items():
            out[k] = points_as_records(self.pts[ids], ids)
        return out

    def surviving_ids(self):
        return np.sort(np.fromiter((i for ids in self.vox.values() for i in ids), np.int64, self.n_points))


def points_as_records(xyz, ids):
    r = np.zeros(len(ids), PT)
    r["x"], r["y"], r["z"], r["id"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], np.asarray(ids, np.int32)
    return r


# ------------------------------------------------------------------ blob ------------------------------------------------------------------
def encode_blob(voxels, capacity, next_id, is_first=0, kind=KIND_P2PLANE_IVOX, resolution=0.5):
    """FLSIVOX1: header, the voxels least recently touched first {key, count}, then their points {x, y, z, id} in insertion order.  capacity and
    is_first are the handle's configuration; everything else is the model's."""
    h = np.zeros(1, HDR)
    h["magic"], h["version"], h["kind"], h["resolution"], h["is_first"] = b"FLSIVOX1", 1, kind, resolution, is_first
    h["capacity"], h["n_voxels"], h["n_points"], h["next_id"] = capacity, len(voxels), sum(len(p) for p in voxels.values()), next_id
    v = np.zeros(len(voxels), VOX)
    v["key"] = [pack_key(*k) for k in voxels]
    v["count"] = [len(p) for p in voxels.values()]
    p = np.concatenate(list(voxels.values())) if voxels else np.zeros(0, PT)
    return np.concatenate([h.view(np.uint8), v.view(np.uint8), p.view(np.uint8)])


def decode_blob(blob):
    """(header record, key -> PT records, least recently touched first)"""
    blob = np.ascontiguousarray(blob, np.uint8)
    h = blob[:HDR.itemsize].view(HDR)[0]
    assert h["magic"] == b"FLSIVOX1" and h["version"] == 1
    nv, npt = int(h["n_voxels"]), int(h["n_points"])
    assert blob.size == HDR.itemsize + 16 * (nv + npt)
    v = blob[HDR.itemsize:HDR.itemsize + 16 * nv].view(VOX)
    p = blob[HDR.itemsize + 16 * nv:].view(PT)
    assert int(v["count"].sum()) == npt
    out, q = collections.OrderedDict(), 0
    for key, cnt in zip(v["key"].tolist(), v["count"].tolist()):
        out[unpack_key(key)] = p[q:q + cnt].copy()
        q += cnt
    assert len(out) == nv, "a voxel is listed twice"
    return h, out


def model_blob(model, is_first=0):
    return encode_blob(model.voxels(), model.capacity, model.next_id, is_first)


# --------------------------------------------------------------- flat image ---------------------------------------------------------------
def decode_image(image):
    """FLSIMG01 in brick form: (header record, pts as PT records [used], directory [dir_mask + 1], cells [n_bricks_live][1024])"""
    image = np.ascontiguousarray(image, np.uint8)
    h = image[:IMG.itemsize].view(IMG)[0]
    assert h["magic"] == b"FLSIMG01" and int(h["total_bytes"]) == image.size
    assert h["have_bricks"] == 1 and h["want_hash"] == 0, "not the brick form"
    used, nd, nb = int(h["used"]), int(h["dir_mask"]) + 1, int(h["n_bricks_live"])
    o = IMG.itemsize
    pts = image[o:o + 16 * used].view(PT); o += 16 * used
    d = image[o:o + 16 * nd].view(DIR); o += 16 * nd
    cells = image[o:o + 8 * BRICK_STRIDE * nb].view(CELL).reshape(nb, BRICK_STRIDE); o += 8 * BRICK_STRIDE * nb
    assert o == image.size
    return h, pts, d, cells


def encode_image(pts, directory, cells, kind=KIND_P2PLANE_IVOX, n_pts_live=None, n_bricks_cap=None):
    """the inverse (for the checker's self-test): pts PT [used], directory DIR [power of two], cells CELL [n_bricks][1024]"""
    h = np.zeros(1, IMG)
    h["magic"], h["kind"], h["have_bricks"], h["use_dense"], h["dir_mask"], h["resolution"] = b"FLSIMG01", kind, 1, 1, len(directory) - 1, 0.5
    h["used"], h["n_pts_live"], h["n_bricks_live"] = len(pts), len(pts) if n_pts_live is None else n_pts_live, len(cells)
    h["n_bricks_cap"] = len(cells) if n_bricks_cap is None else n_bricks_cap
    body = [np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in (pts, directory, cells)]
    h["total_bytes"] = IMG.itemsize + sum(b.size for b in body)
    return np.concatenate([h.view(np.uint8)] + body)


def slab_index(sx, sy, sz):
    return (sz * BRICK_STORED + sy) * BRICK_STORED + sx


@functools.lru_cache(maxsize=None)
def _slab_tables():
    """(stored coordinates of the 512 primary cells, of the face / edge halo cells) as (slab index, (sx, sy, sz)) lists"""
    prim, halo = [], []
    for sz in range(BRICK_STORED):
        for sy in range(BRICK_STORED):
            for sx in range(BRICK_STORED):
                n_out = sum(c in (0, BRICK_STORED - 1) for c in (sx, sy, sz))
                if n_out == 0:
                    prim.append((slab_index(sx, sy, sz), (sx, sy, sz)))
                elif n_out < 3:  # (corner halo cells are never read nor maintained)
                    halo.append((slab_index(sx, sy, sz), (sx, sy, sz)))
    return prim, halo


def check_image(image, voxels):
    """asserts the brick image holds exactly `voxels` (key -> PT records in insertion order) and keeps the halo invariant"""
    h, pts, d, cells = decode_image(image)
    used, nb = int(h["used"]), int(h["n_bricks_live"])
    # the directory: every brick key once, every index a live brick, once
    ent = d[d["key"] != EMPTY_KEY]
    assert not np.isin(ent["begin"], (BRICK_PENDING, BRICK_INVALID)).any(), "a directory entry is pending or invalid"
    assert len(np.unique(ent["key"])) == len(ent), "a brick key appears twice in the directory"
    assert (ent["begin"] < nb).all() and len(np.unique(ent["begin"])) == len(ent), "directory indices are not distinct live bricks"
    brick = {unpack_key(k): int(i) for k, i in zip(ent["key"].tolist(), ent["begin"].tolist())}
    prim, halo = _slab_tables()
    # alive voxels: their primary cells address exactly their points
    want_count = np.zeros((nb, BRICK_STRIDE), np.int64)
    cell_of = {}
    regions = []
    for key, rec in voxels.items():
        b = (key[0] >> 3, key[1] >> 3, key[2] >> 3)
        assert b in brick, f"voxel {key}: its brick {b} is not in the directory"
        bi, si = brick[b], slab_index((key[0] & 7) + 1, (key[1] & 7) + 1, (key[2] & 7) + 1)
        begin, count = int(cells[bi, si]["begin"]), int(cells[bi, si]["count"])
        assert count == len(rec), f"voxel {key}: {count} points in its cell, {len(rec)} expected"
        assert begin + count <= used, f"voxel {key}: its region ends behind the slots in use"
        assert pts[begin:begin + count].tobytes() == rec.tobytes(), f"voxel {key}: points or ids differ, or are out of insertion order"
        want_count[bi, si] = count
        cell_of[key] = (begin, count)
        regions.append((begin, count, key))
        for dx, dy, dz in mirrors_of(key):
            assert (b[0] + dx, b[1] + dy, b[2] + dz) in brick, f"voxel {key}: the brick that mirrors it at {(dx, dy, dz)} is missing"
    # every other primary cell is empty
    pi = np.array([i for i, _ in prim])
    got = cells["count"][:, pi].astype(np.int64)
    bad = np.argwhere(got != want_count[:, pi])
    assert len(bad) == 0, f"{len(bad)} primary cells hold points of no alive voxel, first: brick {bad[0][0]} cell {prim[bad[0][1]][1]}"
    # regions pairwise disjoint
    regions.sort()
    for (b0, c0, k0), (b1, _, k1) in zip(regions, regions[1:]):
        assert b0 + c0 <= b1, f"the regions of voxels {k0} and {k1} overlap"
    # halo cells: equal to the primary cell of the voxel they mirror, {*, 0} when that voxel is not alive
    for (bx, by, bz), bi in brick.items():
        row = cells[bi]
        for si, (sx, sy, sz) in halo:
            key = (bx * 8 + sx - 1, by * 8 + sy - 1, bz * 8 + sz - 1)
            want = cell_of.get(key)
            c = row[si]
            if want is None:
                assert c["count"] == 0, f"brick {(bx, by, bz)}: halo cell {(sx, sy, sz)} is stale: voxel {key} is not alive"
            else:
                assert (int(c["begin"]), int(c["count"])) == want, f"brick {(bx, by, bz)}: halo cell {(sx, sy, sz)} differs from the cell of voxel {key}"
    return len(brick)


# ---------------------------------------------------------------- histories ----------------------------------------------------------------
class History:
    def __init__(self, name, first, capacity, batches, room=()):
        self.name, self.first, self.capacity, self.batches = name, first, capacity, batches
        self.room = set(room)  # indices of the batches the device refuses for room (point array or brick pool full: slot 120)


def at(keys, rng=None, jitter=0.19):
    """points in the voxels `keys`: centre 0.5 * key plus a jitter below 0.2 per axis"""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    p = keys * 0.5
    if rng is not None and jitter:
        p = p + rng.uniform(-jitter, jitter, p.shape)
    p = p.astype(np.float32)
    got, ok = keys_of(p)
    assert ok.all() and np.array_equal(got, keys)
    return p


def mixed(rng, n, drop=0.0):
    """codes 1 and 2 mixed, a share `drop` of zeros"""
    c = rng.integers(1, 3, n).astype(np.uint8)
    if drop:
        c[rng.random(n) < drop] = 0
    return c


def _ranks():
    rng = np.random.default_rng(101)
    vk = np.array([[x, y, 0] for y in range(5) for x in range(6)], np.int64) + [2, -3, 1]  # 30 voxels; the first 10 are old
    first_counts = [4, 4, 8, 8, 3, 3, 2, 2, 5, 1]                                           # 40 points
    first = at(np.repeat(vk[:10], first_counts, 0), rng)
    # batch 1: 700 source points, 480 inserted.  Old voxels: 4 -> 5 and 8 -> 9 (cap_for steps, old points relocated), 8 -> 71, 3 -> 4, 3 -> 67, 2 -> 4 and
    # 5 -> 8 (inside the region), 2 -> 67; the new voxels share the rest
    k = [1, 2, 1, 63, 1, 64, 2, 65, 3, 2]
    rest = 480 - sum(k)
    new = np.ones(20, np.int64)
    for _ in range(rest - 20):
        new[rng.integers(0, 20)] += 1
    k = np.array(k + new.tolist())
    seq = rng.permutation(np.repeat(np.arange(30), k))
    codes = np.zeros(700, np.uint8)
    ins = np.sort(rng.choice(700, 480, replace=False))
    codes[ins] = rng.integers(1, 3, 480)
    keys = np.tile(np.array([[40, 40, 40]], np.int64), (700, 1))  # dropped points: a voxel of their own, which must not appear
    keys[ins] = vk[seq]
    b1 = (at(keys, rng), codes)
    b2 = (at(vk[rng.integers(0, 30, 100)], rng), mixed(rng, 100, drop=0.2))
    return History("ranks", first, None, [b1, b2])


RANKS_GHOST = (40, 40, 40)


def _finish_limits():
    rng = np.random.default_rng(102)
    A, B, C = (5, 5, 5), (-6, 2, 9), (0, 0, 0)
    first = at([C] * 3 + [A] * 2, rng)
    which = rng.permutation(np.repeat([0, 1, 2], [FINISH_MAX_K, FINISH_MAX_K + 1, 51]))  # 2 = dropped
    keys = np.array([A, B, C], np.int64)[which]
    codes = mixed(rng, len(which))
    codes[which == 2] = 0
    return History("finish_limits", first, None, [(at(keys, rng), codes)])


LRU_KEYS = dict(A=(1, 1, 1), B=(9, 1, 1), C=(-4, 3, 0), D=(2, -7, 5), E=(0, 0, 12))


def _lru():
    rng = np.random.default_rng(103)
    K = LRU_KEYS
    first = at([K["A"], K["B"], K["C"]], rng)
    b1 = (at([K[c] for c in "DABAABCED"], rng), np.array([1, 1, 1, 1, 1, 1, 1, 2, 2], np.uint8))  # D: first point code 1, last point code 2
    b2 = (at([K[c] for c in "ABA"], rng), np.array([2, 1, 2], np.uint8))                            # sequence B A A
    b3 = (at([K[c] for c in "AB"], rng), np.array([1, 1], np.uint8))
    return History("lru", first, None, [b1, b2, b3])


def _chain_limit():
    rng = np.random.default_rng(104)
    # the point array is reserved with used + used / 2 + 2^16 slots: 100 full regions of 4,096 points leave room for the 262,144 slots of batch 1
    old = np.array([[x, y, 40] for y in range(10) for x in range(10)], np.int64)
    first = at(np.repeat(old, 4096, 0), rng)
    block = np.array([[x, y, z] for z in range(16) for y in range(16) for x in range(16)], np.int64)
    b1 = (at(rng.permutation(np.repeat(block, 64, 0)), rng), mixed(rng, CHAIN_MAX_POINTS))
    k2 = np.concatenate([np.repeat(block, 64, 0), block[:1]])
    b2 = (at(rng.permutation(k2), rng), mixed(rng, CHAIN_MAX_POINTS + 1))
    return History("chain_limit", first, None, [b1, b2])


FACE_COORDS = (-9, -8, -1, 0, 7, 8, 15, 16)


def _brick_faces():
    rng = np.random.default_rng(105)
    vk = np.array([[x, y, z] for z in FACE_COORDS for y in FACE_COORDS for x in FACE_COORDS], np.int64)
    b1 = (at(rng.permutation(np.repeat(vk, 2, 0)), rng), mixed(rng, 2 * len(vk)))
    b2 = (at(rng.permutation(vk[::2]), rng), mixed(rng, len(vk[::2])))
    return History("brick_faces", at([(3, 3, 3)], rng), None, [b1, b2])


def _half_way():
    rng = np.random.default_rng(106)
    c = np.array([-1.25, -0.75, -0.25, 0.25, 0.75, 1.25], np.float32)
    grid = np.array([[x, y, z] for z in c for y in c for x in c], np.float32)  # exactly half way between two keys on every axis
    pick = rng.permutation(len(grid))[:100]
    return History("half_way", grid, None, [(grid[pick], mixed(rng, 100))])


def _outside():
    rng = np.random.default_rng(107)
    first = at([(x, 0, 0) for x in range(6)], rng)

    def batch(code_of_far):
        keys = np.array([[rng.integers(-5, 12), rng.integers(-3, 4), rng.integers(0, 3)] for _ in range(50)], np.int64)
        p = at(keys, rng)
        far = np.array([[0.5 * KEY_LIMIT, 0.1, 0.1]], np.float32)  # key (1 << 20) - 2 on x: the first one beyond the range
        assert not keys_of(far)[1][0]
        codes = np.concatenate([mixed(rng, 25), [code_of_far], mixed(rng, 25)]).astype(np.uint8)
        return np.concatenate([p[:25], far, p[25:]]), codes
    ordinary = (at([(rng.integers(-5, 12), 1, 1) for _ in range(40)], rng), mixed(rng, 40))
    return History("outside", first, None, [batch(1), batch(2), ordinary])


def _pool_full():
    rng = np.random.default_rng(108)
    first = at([(3, 3, 3), (4, 3, 3), (3, 4, 3)], rng)
    far = np.array([[24 * (i % 20) + 3, 24 * (i // 20) + 3, 99] for i in range(400)], np.int64)  # interior voxels, one brick each, no mirrors
    ordinary = (at([(rng.integers(0, 8), rng.integers(0, 8), 3) for _ in range(60)], rng), mixed(rng, 60))
    return History("pool_full", first, None, [(at(rng.permutation(far), rng), mixed(rng, 400)), ordinary], room=[0])


# The point array is reserved with used + used / 2 + 2^16 slots (IvoxMap::build_brick_pool), and DevBuf::reserve rounds that up along its growth
# sequence c -> c + c / 2 + 64, so to less than 1.5 times the request + 64: about 98,400 slots behind a small first cloud.  4 N slots exceed that.
ARRAY_FULL_N = 25000


def _array_full():
    rng = np.random.default_rng(109)
    first = at([(0, 0, 20), (1, 0, 20), (0, 1, 20)], rng)
    block = np.array([[x, y, z] for z in range(25) for y in range(32) for x in range(32)], np.int64)[:ARRAY_FULL_N]
    ordinary = (at(block[rng.integers(0, len(block), 80)], rng), mixed(rng, 80))
    return History("array_full", first, None, [(at(rng.permutation(block), rng), mixed(rng, ARRAY_FULL_N)), ordinary], room=[0])


def _line(n, y=0, z=0, x0=0):
    return np.array([[x0 + i, y, z] for i in range(n)], np.int64)


def _evict_untouched():
    rng = np.random.default_rng(110)
    b1 = (at(_line(50, y=30, z=7), rng), mixed(rng, 50))
    b2 = (at(_line(30, y=-30, z=7), rng), mixed(rng, 30))
    return History("evict_untouched", at(_line(290), rng), 300, [b1, b2])


def _evict_skip():
    rng = np.random.default_rng(111)
    v = _line(39)
    new = _line(3, y=20)
    return History("evict_skip", at(v, rng), 40, [(at(np.concatenate([v[:1], new]), rng), np.ones(4, np.uint8))])


def _evict_recreate():
    rng = np.random.default_rng(112)
    v = _line(39)
    new = _line(4, y=20)
    b1 = (at([new[0], v[0], new[1]], rng), np.ones(3, np.uint8))
    b2 = (at([new[2], v[3], v[4], new[3]], rng), np.array([1, 1, 2, 2], np.uint8))  # v3 and v4: neighbours in the LRU order, both evicted and created again
    return History("evict_recreate", at(v, rng), 40, [b1, b2])


def _evict_chunks():
    rng = np.random.default_rng(113)
    old = np.array([[i % 40, i // 40, 0] for i in range(1199)], np.int64)  # o0 the least recently touched
    new = np.array([[i % 40, i // 40, 50] for i in range(1100)], np.int64)
    keys = np.concatenate([old[1050:1051], new[:20], old[10:11], new[20:1080], old[1060:1061], new[1080:]])
    return History("evict_chunks", at(old, rng), 1200, [(at(keys, rng), np.ones(len(keys), np.uint8))])


def _evict_own():
    rng = np.random.default_rng(114)
    return History("evict_own", at(_line(5), rng), 40, [(at(_line(40, y=9), rng), mixed(rng, 40)), (at(_line(3, y=-9), rng), mixed(rng, 3))])


def _evict_overflow():
    rng = np.random.default_rng(115)
    old = np.array([[i % 40, i // 40, 0] for i in range(1199)], np.int64)
    keys = np.concatenate([[[0, 0, 50]], old[:1030]])
    return History("evict_overflow", at(old, rng), 1200, [(at(keys, rng), np.ones(len(keys), np.uint8))])


def _evict_stream():
    rng = np.random.default_rng(116)
    pts, _ = evict_pin.make_cloud()
    batches = [(pts[i:i + 250], mixed(rng, len(pts[i:i + 250]))) for i in range(40, len(pts), 250)]
    return History("evict_stream", pts[:40], evict_pin.CAPACITY, batches)


_BUILDERS = dict(ranks=_ranks, finish_limits=_finish_limits, lru=_lru, chain_limit=_chain_limit, brick_faces=_brick_faces, half_way=_half_way, outside=_outside,
                 pool_full=_pool_full, array_full=_array_full, evict_untouched=_evict_untouched, evict_skip=_evict_skip, evict_recreate=_evict_recreate,
                 evict_chunks=_evict_chunks, evict_own=_evict_own, evict_overflow=_evict_overflow, evict_stream=_evict_stream)
NAMES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def history(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def replay(name):
    """the model run over the history once: [(BatchInfo, blob bytes, voxels)] after the first cloud and after every batch.  Shared by the tests;
    nothing in it is changed by them."""
    h = history(name)
    m = Model(h.capacity)
    out = []
    for pts, codes in [(h.first, None)] + list(h.batches):
        info = m.insert(pts, codes)
        vox = m.voxels()
        out.append((info, encode_blob(vox, m.capacity, m.next_id), vox, m.next_id))
    return out, m
