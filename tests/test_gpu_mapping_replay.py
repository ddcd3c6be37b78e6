"""Mapping-mode replay parity on the GPU (SURVEY.md 8a rows a15, a17, a19 + a7): HIP path through the C ABI vs the CPU
oracle over a multi-scan trajectory with update_map = true -- the call the reference's FrontEnd actually issues.

Compared after EVERY scan: return value, iteration count, n_valid and pose after every Gauss-Newton iteration,
valid flags / neighbour counts / correspondence ids of every source point (ids are map cloud indices for the kd-tree
kinds, so they also pin the ORDER of the rebuilt local map), the map_updated decision, the map sizes of every slot.
The scenarios (tests/replay.py) are asserted to actually reach the rules they are there for.
"""
import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg, synth
from tests import replay, util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"


def run_replay(name, monkeypatch=None, r=None, start=None):
    r = r if r is not None else replay.make_replay(name)
    mode, y = r["mode"], r["y"]
    m = reg.make_matcher(mode, y)
    o = util.oracle_for(mode, y)
    m.AddCloudToLocalMap(r["init_clouds"])
    o.AddCloudToLocalMap(*r["init_clouds"])
    slots = (0, 1) if mode == "LoamFull_KdTree" else (0,)
    for s in slots:
        assert m.map_size(s) == o.map_size(s), ("init", s)
    Tprev = np.eye(4) if start is None else np.array(start, dtype=np.float64)
    hist = []
    for k, f in enumerate(r["frames"]):
        guess = Tprev @ f["guess_step"]
        T = guess.copy()
        ok = m.Match(util.cluster_for(mode, f["scan"], f["corner"]), T, update_map=True)
        ok_ref, T_ref = o.Match(f["scan"], guess, src1=f["corner"], update_map=True)
        ties = int(o.counters().tie_queries)
        util.assert_same_registration(m, o, ok, T, ok_ref, T_ref, slots=slots, sets_only_tail=(mode == "PointToPlane_IVOX"), max_tie_rows=ties)
        assert m.stats.map_updated == o.stats.map_updated, (name, k)
        assert m.stats.n_source == o.stats.n_source and m.stats.n_source_corner == o.stats.n_source_corner, (name, k)
        for s in slots:
            assert m.map_size(s) == o.map_size(s), (name, k, s, m.map_size(s), o.map_size(s))
        hist.append(dict(ok=ok_ref, upd=int(o.stats.map_updated), size=o.map_size(0), iters=int(o.stats.iterations)))
        Tprev = T_ref
    if mode == "IncrementalNDT":
        r["image_syncs"] = (m.map_size(107), m.map_size(108))  # full rebuilds, incremental updates of the device image
        r["device_updates"] = (m.map_size(109), m.map_size(110))  # map updates applied on the device / refused
        r["device_growths"] = (m.map_size(112), m.map_size(113))  # device-side table rebuilds / row-array growths
        r["device_evictions"] = (m.map_size(117), m.map_size(118))  # voxels evicted by device batches / row compactions
        r["device_recreated"] = m.map_size(126)  # voxels evicted and re-created inside one device batch
    m.close()
    return r, hist


def test_icp_mapping_replay():
    """IcpOptimized in mapping mode: deque + pop_front, Q13 VoxelGrid of the concatenated deque, IsNeedAddCloud, Q10."""
    r, h = run_replay("icp")
    assert sum(x["upd"] for x in h) > r["y"]["local_map_size"], "the deque must overflow (pop_front)"
    assert any(x["ok"] and not x["upd"] for x in h[1:]), "a converged frame must fail the keyframe gate"
    assert any(not x["ok"] for x in h), "a frame must run out of iterations (Q10)"
    assert all(x["upd"] == 0 for x in h if not x["ok"]), "Q10: no map update without convergence"


def test_p2plane_kd_mapping_replay():
    """LoamPointToPlaneKdtree in mapping mode (every other test of this kind runs in localization mode): deque growth, pop_front
    once it holds more than local_map_size clouds, VoxelGrid of the concatenated deque, keyframe gate."""
    r, h = run_replay("p2plane_kd")
    clouds = 1 + np.cumsum([x["upd"] for x in h])  # clouds pushed so far (the initial one included), after every frame
    full = clouds > r["y"]["local_map_size"]  # this frame's push found the deque full: pop_front
    assert any(x["upd"] == 1 and f for x, f in zip(h, full)), "a map update must land on a full deque (pop_front)"
    assert any(x["ok"] and not x["upd"] for x in h), "a converged frame must fail the keyframe gate"


def test_ndt_mapping_replay_host_evictions(monkeypatch):
    """IncrementalNDT in mapping mode: non-first-scan UpdateVoxel (min / max points, pooled mean + covariance, SVD clamp),
    LRU eviction at the (shrunk) capacity, Q11 (map update with the input pose -- every guess differs from the result).
    HOST path of the evictions (FLS_NDT_DEVICE_UPDATE=0; the device evictions of the same frames: ..._with_conflicts below)."""
    monkeypatch.setenv("FLS_NDT_DEVICE_UPDATE", "0")
    r, h = run_replay("ndt")
    cap = r["y"]["ndt_capacity"]
    assert all(x["upd"] == 1 for x in h)
    assert h[-1]["size"] == cap - 1 and sum(1 for x in h if x["size"] == cap - 1) >= 4, "the LRU list must sit at capacity for several scans"
    full, incr = r["image_syncs"]
    assert incr >= 4, (full, incr)  # the device image is edited in place (rows, table entries, tombstones of evicted voxels), not re-uploaded


def test_ndt_mapping_replay_device_update():
    """The same frames with the LRU capacity far away: after the first (host) update the handle enters device mode and every later
    AddCloud -- key lookup / voxel creation (ids in first-appearance order), pending-point carry, pooled mean + covariance, SVD
    clamp, LRU stamps -- runs in kernels_ndt_update.hpp; correspondence ids (voxel ids), n_valid, poses and map sizes of every
    frame equal the oracle's."""
    r, h = run_replay("ndt_dev")
    applied, refused = r["device_updates"]
    assert all(x["upd"] == 1 for x in h)
    assert applied >= len(h) - 1 and refused == 0, (applied, refused)


def test_ndt_mapping_replay_device_update_growing_arrays(monkeypatch):
    """No spare room allocated ahead: the device-mode table is re-hashed on the device and the row arrays are re-allocated (with
    their contents) while the map grows -- same results."""
    monkeypatch.setenv("FLS_NDT_DEVICE_SLACK", "0")
    r, h = run_replay("ndt_dev")
    applied, refused = r["device_updates"]
    assert applied >= len(h) - 1 and refused == 0
    assert r["device_growths"][0] >= 1 or r["device_growths"][1] >= 1, r["device_growths"]


def test_ndt_mapping_replay_device_refusal_when_the_batch_evicts_its_own_voxels():
    """Capacity 700: four 12 m scans (about 380 voxels each) run on the device; then the sensor range jumps to 40 m and the batch
    creates about 1,000 voxels, so the sequential loop would evict voxels this batch itself created (incremental_ndt.h:202-206).  The
    device refuses that batch without side effects, the device state comes back to the host mirror (LRU order from the stamps, pending
    points from the carry buffers) and the exact sequential path takes over -- including the evictions."""
    r = replay.make_replay("ndt_dev", max_range=12.0, y_over=dict(ndt_capacity=700))
    scene = synth.make_scene()
    rng = synth.rng_for(5, 99)
    for f in r["frames"][4:]:
        f["scan"] = synth.cast_scan(scene, f["T_gt"], rng=rng, max_range=40.0, **dict(synth.VELODYNE_64, n_az=100))
    r, h = run_replay("ndt_dev", r=r)
    applied, refused = r["device_updates"]
    cap = r["y"]["ndt_capacity"]
    assert refused == 1 and applied >= 1, (applied, refused)  # (eight host-path updates go by before device mode is entered again)
    assert h[-1]["size"] == cap - 1


def test_ndt_mapping_replay_device_evictions():
    """Round 3: LRU evictions INSIDE a device batch (incremental_ndt.h:202-206).  A straight 33 m run with a 20 m sensor range and a
    capacity of 1,700 voxels: from frame ~17 on every scan creates 30-70 voxels and the same number of least recently touched ones
    -- far behind the sensor, untouched by the batch -- are evicted on the device (rows sorted by their 64-bit LRU stamp, tombstoned
    table entries).  The handle never leaves device mode: no refused batch; every frame equals the oracle (voxel ids, n_valid, poses,
    map sizes)."""
    start = np.eye(4)
    start[1, 3] = 18.0  # the corridor between two rows of buildings
    r = replay.make_replay("ndt_dev", n_frames=40, yaw_long_deg=0.0, start=start, max_range=20.0, y_over=dict(ndt_capacity=1700))
    r, h = run_replay("ndt_dev", r=r, start=start)
    applied, refused = r["device_updates"]
    evicted, compactions = r["device_evictions"]
    assert h[-1]["size"] == 1699 and sum(1 for x in h if x["size"] == 1699) >= 15, "the LRU list must sit at capacity for many scans"
    assert refused == 0 and applied >= len(h) - 1, (applied, refused)
    assert evicted > 500, evicted
    print(f"ndt straight run at capacity 1700: {applied} device batches, {refused} refused, {evicted} voxels evicted on the device, {compactions} compactions")


def test_ndt_mapping_replay_device_evictions_with_conflicts():
    """The adversarial case: capacity 2,600 in a scene the sensor sees end to end, so the least recently touched voxels ARE touched by
    nearly every batch.  Round 3 refused such a batch and replayed it on the host; since round 4 the eviction walk (ndt_evict_select)
    skips the candidates the batch touched before their turn and re-creates the ones it touched after it, like the sequential loop
    does (incremental_ndt.h:196-211).  Only a batch whose evictions would reach voxels it created or touched itself still goes to the
    host.  Results equal the oracle throughout (run_replay asserts every frame)."""
    r, h = run_replay("ndt")
    applied, refused = r["device_updates"]
    evicted, _ = r["device_evictions"]
    cap = r["y"]["ndt_capacity"]
    print(f"ndt adversarial run at capacity {cap}: {applied} device batches, {refused} refused, {evicted} voxels evicted on the device, "
          f"{r['device_recreated']} of them re-created by the same batch")
    assert h[-1]["size"] == cap - 1 and sum(1 for x in h if x["size"] == cap - 1) >= 4
    assert applied >= len(h) - 2 and evicted >= 1, (applied, refused, evicted)


def test_ndt_mapping_replay_host_path_ab(monkeypatch):
    monkeypatch.setenv("FLS_NDT_DEVICE_UPDATE", "0")
    r, h = run_replay("ndt_dev")
    assert r["device_updates"] == (0, 0) and r["image_syncs"][1] >= 1  # small map: most updates touch too much of it for in-place edits


def test_loam_full_mapping_replay():
    """LoamFull: corner + planar deques, VoxelGrid once a deque holds more than five frames, keyframe gate."""
    r, h = run_replay("loam")
    n_upd = sum(x["upd"] for x in h)
    assert n_upd >= 6, "more than five keyframes so that the VoxelGrid branch (loam_full_kdtree.h:92-100) fires"
    assert any(not x["upd"] for x in h[1:]), "some frame must fail the keyframe gate"
    sizes = [x["size"] for x in h]
    assert any(b < a for a, b in zip(sizes, sizes[1:])), "the planar map must shrink when the VoxelGrid switches on"
    assert h[-1]["iters"] > 0


def test_ivox_mapping_replay_prior_map():
    """LoamPointToPlaneIVOX on the shared scenario (same one the compiled-reference pin uses)."""
    r, h = run_replay("ivox")
    assert all(x["upd"] == 1 for x in h) and h[-1]["size"] > h[0]["size"]


def test_update_map_after_match_only_upload():
    """fls_match(update_map=0) uploads the scan without its host copy; a later
    fls_match_resident(update_map=1) on that resident scan must either work or refuse BEFORE touching T."""
    cfg = synth.make_config(1, scale=0.03)
    m = reg.make_matcher("PointToPlane_IVOX", reg.YAML_NCLT_IVOX)
    m.AddCloudToLocalMap([cfg["map"]])
    cl = reg.PointcloudCluster(planar_cloud_=cfg["scan"])
    T = np.eye(4)
    m.Match(cl, T, update_map=False)
    n0 = m.map_size()
    T2 = np.eye(4)
    ok = m.MatchResident(T2, update_map=True)  # header contract: fls_match == fls_scan_upload + fls_match_resident
    assert ok and m.stats.map_updated == 1 and m.map_size() > n0
    # same end state as the two fls_match calls on another handle (the second Match differs from the first one:
    # nearest_points_ persists across Matches, Q15)
    f = reg.make_matcher("PointToPlane_IVOX", reg.YAML_NCLT_IVOX)
    f.AddCloudToLocalMap([cfg["map"]])
    T3 = np.eye(4)
    f.Match(cl, T3, update_map=False)
    assert np.array_equal(T3, T)
    T4 = np.eye(4)
    f.Match(cl, T4, update_map=True)
    assert np.array_equal(T4, T2) and f.map_size() == m.map_size() and f.map_size(102) == m.map_size(102)
    m.close(); f.close()


def test_update_map_zero_leaves_keyframe_gate_alone():
    """a Match with update_map = 0 must not consume the keyframe gate (IsNeedAddCloud's last_T)."""
    r = replay.make_replay("icp")
    mode, y = r["mode"], r["y"]
    a = reg.make_matcher(mode, y)
    b = reg.make_matcher(mode, y)
    for m in (a, b):
        m.AddCloudToLocalMap(r["init_clouds"])
    Tprev = np.eye(4)
    for k, f in enumerate(r["frames"][:5]):
        guess = Tprev @ f["guess_step"]
        cl = util.cluster_for(mode, f["scan"], None)
        Tb0 = guess.copy()
        b.Match(cl, Tb0, update_map=False)  # an extra look without map update (e.g. a relocalisation probe) ...
        Ta, Tb = guess.copy(), guess.copy()
        oka = a.Match(cl, Ta, update_map=True)
        okb = b.Match(cl, Tb, update_map=True)  # ... must not change what the real call does
        assert oka == okb and np.array_equal(Ta, Tb), k
        assert a.stats.map_updated == b.stats.map_updated and a.map_size() == b.map_size(), k
        Tprev = Ta
    a.close(); b.close()
