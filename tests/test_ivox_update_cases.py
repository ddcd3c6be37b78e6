"""tests/ivox_update_cases.py without a GPU: every history reaches the numbers it is named for (on the sequential model alone), the model's final
state is the CPU oracle's after a fresh oracle took the first cloud and every batch's inserted points as ONE first cloud at the same capacity (the
reference inserts in a plain loop, so batch after batch equals their concatenation: first cloud, then per batch its code-1 points, then its code-2
points), the blob codec round-trips, and check_image passes a hand-made image and fails on each way it is made wrong -- a checker that cannot fail proves
nothing."""
import collections

import numpy as np
import pytest

from funny_lidar_slam_amd import registration as reg
from tests import evict_pin, util
from tests import ivox_update_cases as U


def _infos(name):
    out, model = U.replay(name)
    return [o[0] for o in out], model


# ---------------------------------------------------- the model against the CPU oracle ----------------------------------------------------
@pytest.mark.parametrize("name", U.NAMES)
def test_model_final_state_is_the_oracles(built, name):
    h = U.history(name)
    _, model = U.replay(name)
    assert model.next_id == len(model.pts), "ids are positions in the concatenation of everything inserted"
    o = util.oracle_for("PointToPlane_IVOX", reg.YAML_NCLT_IVOX)
    if h.capacity is not None:
        o.set_ivox_capacity(h.capacity)
    o.AddCloudToLocalMap(model.pts)
    try:
        assert o.map_voxels() == model.n_alive and o.map_size() == model.n_points
        assert np.array_equal(o.map_dump(0), model.pts[model.surviving_ids()])  # (the oracle dumps in insertion-id order)
    finally:
        o.close()


def test_model_is_evict_pins_sequential_model():
    """the ten-line model tests/evict_pin.py ties to the compiled reference, on its own cloud: same LRU order, same points per voxel, same counts"""
    pts, keys = evict_pin.make_cloud()
    lru, vox, n_evict, n_recreate = evict_pin.sequential_model(keys, evict_pin.CAPACITY)
    m = U.Model(evict_pin.CAPACITY)
    info = m.insert(pts)
    assert list(reversed(m.vox)) == lru and {k: v for k, v in m.vox.items()} == vox
    assert (info.n_evicted, info.n_recreated) == (n_evict, n_recreate) and info.evicted_own


def test_key_rule_is_round_half_away_in_float32():
    p = np.array([[0.25, -0.25, 0.75], [-0.75, 1.25, -1.25], [0.24999999, 0.7499999, 2.5]], np.float32)
    k, ok = U.keys_of(p)
    assert ok.all() and k.tolist() == [[1, -1, 2], [-2, 3, -3], [0, 1, 5]]
    assert not np.array_equal(np.round(p * np.float32(2.0)), k), "np.round (half to even) is another rule"
    far = np.array([[0.5 * (U.KEY_LIMIT - 1), 0, 0], [0.5 * U.KEY_LIMIT, 0, 0], [0, -0.5 * U.KEY_LIMIT, 0]], np.float32)
    assert U.keys_of(far)[1].tolist() == [True, False, False]
    for key in [(0, 0, 0), (-1, 5, -1048573), (1048573, -1048573, 7)]:
        assert U.unpack_key(U.pack_key(*key)) == key


# ------------------------------------------------------ the numbers a history is named for ------------------------------------------------
def test_ranks_numbers():
    h = U.history("ranks")
    info, model = _infos("ranks")
    b1 = info[1]
    assert (b1.n_source, b1.inserted) == (700, 480) and len(b1.k) == 30 and len(info[0].k) == 10
    assert {1, 2, 63, 64, 65} <= set(b1.k.values())
    codes = h.batches[0][1]
    for blk in range(3):  # both code sequences cross the two 256-thread block boundaries of the 700 source points
        c = codes[blk * U.UPD_BLOCK:(blk + 1) * U.UPD_BLOCK]
        assert (c == 0).any() and (c == 1).any() and (c == 2).any()
    first_keys = list(collections.OrderedDict.fromkeys(map(tuple, U.keys_of(h.first)[0].tolist())))
    grew = {(info[0].k[k], info[0].k[k] + b1.k[k]) for k in first_keys}
    assert {(4, 5), (8, 9)} <= grew, "cap_for steps: old points are relocated"
    assert {(3, 4), (2, 4), (5, 8)} <= grew, "appended inside the region"
    assert U.RANKS_GHOST not in model.vox and (codes == 0).sum() == 220, "dropped points create nothing"
    assert all(i.device_can_apply and i.short_chain and not i.evictions for i in info)
    assert info[2].inserted < info[2].n_source == 100


def test_finish_limits_numbers():
    info, _ = _infos("finish_limits")
    assert sorted(info[1].k.values()) == [U.FINISH_MAX_K, U.FINISH_MAX_K + 1], "the wave sort at its limit, the serial fallback one past it"
    codes = U.history("finish_limits").batches[0][1]
    assert set(codes.tolist()) == {0, 1, 2} and info[1].device_can_apply and info[1].short_chain


def test_lru_numbers():
    K = U.LRU_KEYS
    out, _ = U.replay("lru")
    order = [[k for k in reversed(o[2])] for o in out]  # most recently touched first
    assert order[0] == [K["C"], K["B"], K["A"]]
    assert order[1] == [K["D"], K["E"], K["C"], K["B"], K["A"]], "D: first point code 1, last point code 2 -- its place is its last rank; C is only appended to"
    assert order[2] == [K["A"], K["B"], K["D"], K["E"], K["C"]] and order[3] == [K["B"], K["A"], K["D"], K["E"], K["C"]]
    assert [len(p) for p in out[1][2].values()] == [4, 3, 2, 1, 2]


def test_chain_limit_numbers():
    info, model = _infos("chain_limit")
    assert info[1].n_source == info[1].inserted == U.CHAIN_MAX_POINTS and set(info[1].k.values()) == {64} and len(info[1].k) == 4096
    assert info[2].n_source == U.CHAIN_MAX_POINTS + 1 and info[1].short_chain and info[1].device_can_apply
    # room for batch 1 in the point array as the first build reserves it (used + used / 2 + 2^16), and in the smallest brick pool
    used0 = sum(max(4, 1 << (n - 1).bit_length()) for n in info[0].k.values())
    assert used0 // 2 + (1 << 16) >= 4096 * 64 and info[1].bricks <= U.FIRST_POOL_BRICKS


def test_brick_numbers():
    info, _ = _infos("brick_faces")
    assert len(info[1].k) == 512 and set(info[1].k.values()) == {2} and len(info[2].k) == 256
    assert info[1].bricks == 125 and all(U.mirrors_of(k) for k in info[1].k), "every voxel sits on a face of its brick: 5^3 bricks, all made by the batch"
    assert sorted(len(U.mirrors_of((x, 3, 3))) for x in (3, 8, 15)) == [0, 1, 1] and len(U.mirrors_of((0, 7, 3))) == 3 and len(U.mirrors_of((0, 7, 8))) == 6
    info, model = _infos("half_way")
    assert {abs(c) for k in model.vox for c in k} == {1, 2, 3} and model.n_alive == 216 and info[1].inserted == 100
    info, _ = _infos("pool_full")
    assert info[1].bricks > U.FIRST_POOL_BRICKS and len(info[1].k) == 400 and U.history("pool_full").room == {0}
    info, _ = _infos("array_full")
    used0 = sum(max(4, 1 << (n - 1).bit_length()) for n in info[0].k.values())
    reserved = used0 + used0 // 2 + (1 << 16)  # IvoxMap::build_brick_pool; DevBuf::reserve allocates less than 1.5 times that + 64
    assert used0 + 4 * U.ARRAY_FULL_N > reserved + reserved // 2 + 64 and set(info[1].k.values()) == {1}, "more new regions than the point array has slots"
    assert info[1].bricks <= U.FIRST_POOL_BRICKS, "the brick pool is not what refuses the batch"


def test_outside_numbers():
    h = U.history("outside")
    info, model = _infos("outside")
    n1 = int((h.batches[1][1] == 1).sum())
    assert [(i.rc, i.inserted, i.outside) for i in info[1:]] == [(U.FLS_ERR_RANGE, 0, True), (U.FLS_ERR_RANGE, n1, True), (U.FLS_OK, 40, False)]
    assert 0 < n1 < 50 and [i.refusal for i in info[1:]] == ["outside", "outside", None]


def test_eviction_numbers():
    line = [(i, 0, 0) for i in range(39)]
    info, model = _infos("evict_untouched")
    assert [i.n_evicted for i in info] == [0, 41, 30] and info[1].evictions == [(i, 0, 0) for i in range(41)] and model.n_alive == 299
    assert all(i.device_can_apply and not i.n_recreated for i in info) and not info[1].short_chain
    info, model = _infos("evict_skip")
    assert info[1].evictions == line[1:4] and line[0] in model.vox and info[1].n_recreated == 0 and info[1].device_can_apply
    info, model = _infos("evict_recreate")
    assert info[1].evictions == line[0:3] and info[1].n_recreated == 1 and info[1].device_can_apply and len(model.vox[line[0]]) == 1
    assert info[2].evictions == line[3:7] and info[2].n_recreated == 2 and info[2].device_can_apply
    info, model = _infos("evict_chunks")
    old = [(i % 40, i // 40, 0) for i in range(1199)]
    ev = info[1].evictions
    assert len(ev) == 1102 > U.EV_BLOCK and info[1].n_recreated == 2 and info[1].device_can_apply
    assert old[1050] in model.vox and old[1050] not in ev and ev.index(old[1051]) > U.EV_BLOCK, "a touched-before candidate beyond the first chunk is skipped"
    assert ev.index(old[10]) < U.EV_BLOCK < ev.index(old[1060]) and old[10] in model.vox and old[1060] in model.vox, "one re-creation per chunk"
    info, _ = _infos("evict_own")
    assert info[1].evicted_own and info[1].refusal == "need_host" and len(info[1].k) == 40 == U.history("evict_own").capacity and info[2].device_can_apply
    info, _ = _infos("evict_overflow")
    assert info[1].n_recreated == 1030 > U.EV_MAX_RECREATE and not info[1].evicted_own and info[1].refusal == "conflict" and info[1].n_evicted == 1031
    info, model = _infos("evict_stream")
    assert len(info) == 13 and all(i.n_evicted > 0 and i.n_recreated > 0 for i in info[1:]) and model.n_alive == evict_pin.CAPACITY - 1
    assert [i.refusal for i in info[1:]] == ["need_host"] * 12, "250 points at capacity 60: every batch evicts voxels it touched itself"


# ------------------------------------------------------------------ codecs ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["ranks", "evict_recreate", "half_way"])
def test_blob_round_trip(name):
    out, model = U.replay(name)
    for info, blob, vox, next_id in out:
        h, got = U.decode_blob(blob)
        assert (int(h["capacity"]), int(h["next_id"]), int(h["is_first"]), int(h["kind"])) == (model.capacity, next_id, 0, U.KIND_P2PLANE_IVOX)
        assert list(got) == list(vox) and all(got[k].tobytes() == vox[k].tobytes() for k in vox)
        assert U.encode_blob(got, int(h["capacity"]), int(h["next_id"])).tobytes() == blob.tobytes()


def _two_brick_image():
    """bricks (0,0,0) and (1,0,0); voxel (7,3,3) on the shared face (mirrored in brick 1), voxel (2,2,2) inside brick 0, voxel (9,3,3) inside brick 1"""
    vox = collections.OrderedDict()
    pts = np.zeros(12, U.PT)
    pts["id"] = -1
    layout = {(7, 3, 3): (0, [0, 3]), (2, 2, 2): (4, [1]), (9, 3, 3): (8, [2, 4, 5])}
    cells = np.zeros((2, U.BRICK_STRIDE), U.CELL)
    for key, (begin, ids) in layout.items():
        rec = U.points_as_records(np.array([[0.5 * c for c in key]] * len(ids), np.float32), ids)
        pts[begin:begin + len(ids)] = rec
        vox[key] = rec
        cells[key[0] >> 3, U.slab_index((key[0] & 7) + 1, (key[1] & 7) + 1, (key[2] & 7) + 1)] = (begin, len(ids))
    cells[1, U.slab_index(0, 4, 4)] = (0, 2)  # the halo copy of (7,3,3) in brick 1
    d = np.zeros(8, U.DIR)
    d["key"] = U.EMPTY_KEY
    d["begin"] = U.BRICK_PENDING
    d[3] = (U.pack_key(0, 0, 0), 0, 0)
    d[6] = (U.pack_key(1, 0, 0), 1, 0)
    return pts, d, cells, vox


def test_check_image_passes_and_fails():
    pts, d, cells, vox = _two_brick_image()
    assert U.check_image(U.encode_image(pts, d, cells), vox) == 2
    stale = cells.copy()
    stale[1, U.slab_index(0, 4, 4)] = (0, 1)
    with pytest.raises(AssertionError, match="halo cell"):
        U.check_image(U.encode_image(pts, d, stale), vox)
    ghost = cells.copy()
    ghost[0, U.slab_index(9, 5, 5)] = (8, 1)  # a halo cell that mirrors a voxel nobody holds
    with pytest.raises(AssertionError, match="stale"):
        U.check_image(U.encode_image(pts, d, ghost), vox)
    lone = d.copy()
    lone[6] = (U.EMPTY_KEY, U.BRICK_PENDING, 0)
    only0 = collections.OrderedDict((k, v) for k, v in vox.items() if k != (9, 3, 3))
    c0 = cells[:1].copy()
    with pytest.raises(AssertionError, match="mirrors it"):
        U.check_image(U.encode_image(pts, lone, c0), only0)
    over = cells.copy()
    over[0, U.slab_index(3, 3, 3)] = (1, 1)  # voxel (2,2,2) inside the region of (7,3,3); the point there made to match
    p2 = pts.copy()
    p2[1] = vox[(2, 2, 2)][0]
    v2 = collections.OrderedDict(vox)
    v2[(7, 3, 3)] = p2[0:2].copy()
    with pytest.raises(AssertionError, match="overlap"):
        U.check_image(U.encode_image(p2, d, over), v2)
    gone = collections.OrderedDict((k, v) for k, v in vox.items() if k != (2, 2, 2))
    with pytest.raises(AssertionError, match="no alive voxel"):
        U.check_image(U.encode_image(pts, d, cells), gone)
    twice = d.copy()
    twice[7] = (U.pack_key(1, 0, 0), 1, 0)
    with pytest.raises(AssertionError, match="twice"):
        U.check_image(U.encode_image(pts, twice, cells), vox)
    pend = d.copy()
    pend[6]["begin"] = U.BRICK_INVALID
    with pytest.raises(AssertionError, match="pending or invalid"):
        U.check_image(U.encode_image(pts, pend, cells), vox)
    with pytest.raises(AssertionError, match="points or ids"):
        swapped = pts.copy()
        swapped[[8, 9]] = swapped[[9, 8]]
        U.check_image(U.encode_image(swapped, d, cells), vox)
