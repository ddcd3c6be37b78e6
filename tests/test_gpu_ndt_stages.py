"""The IncrementalNDT kernels on constructed inputs (tests/ndt_cases.py; tests/test_ndt_cases.py shows on the oracle alone that every case reaches its decision).

Scoring: ndt_lanes_kernel<true> (the product's launch) and ndt_kernel<true> + gn_solve_lu_kernel (set_profiling(False, counters=True)), one iteration on an
imported image, against the oracle on the same image: ids [n][7], counts, flags, n_valid, return value and iteration count equal; traffic counters equal; H
and g within 2 gamma_N A per entry (A, N as in test_gpu_fit_stages.py), H symmetric to the bit; sum_res within gamma_N sum |r|; the pose through
util.assert_same_registration where H is conditioned.

Histories: every batch of ndt_upd_voxel (default handle) and of the host mirror + ndt_apply_edits_kernel (FLS_NDT_DEVICE_UPDATE=0): after every batch
ExportMap() equals the oracle's full dump encoded as an image BYTE FOR BYTE, ndt_voxels() agrees with it, and a one-iteration Match of a probe cloud with a
point in every voxel is compared like a scoring case -- which is what shows that the rows and table entries the Match kernel reads were published."""
import functools

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg
from tests import fit_cases as FC, linalg_cases as LC, ndt_cases as N, util
from tests.test_gpu_linalg import _p

pytestmark = pytest.mark.gpu
HOST = {"FLS_NDT_DEVICE_UPDATE": "0"}
SLACK0 = {"FLS_NDT_DEVICE_SLACK": "0"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"


def make(monkeypatch, y, env=None, loc=False, image=None):
    """the switches are read when the handle is created"""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    m = reg.make_matcher(N.MODE, y, is_localization_mode=loc)
    for k in (env or {}):
        monkeypatch.delenv(k)
    if image is not None:
        m.ImportMap(image)
    return m


def oracle(y, image=None, loc=False):
    o = util.oracle_for(N.MODE, y, loc)
    if image is not None:
        assert o.ndt_import_image(image)
    return o


class Ref:
    """one oracle Match, kept: the reference is computed once and shared"""

    def __init__(self, o, cloud, T0):
        self.ok, self.T = o.Match(cloud, T0, update_map=False)
        self.o = o
        self.stats = (o.stats.iterations, o.stats.n_valid, o.stats.n_source, o.stats.converged)
        self.ids, self.cnt, self.valid = o.correspondences()
        self.log = o.iteration_log()
        self.H, self.g = o.last_system()
        self.Ha, self.ga, self.terms = o.last_abs_system()
        c = o.counters()
        self.traffic = (int(c.probes), int(c.hit_voxels), int(c.cand_points))
        self.cond = np.linalg.cond(self.H) if np.isfinite(self.H).all() and self.H.any() else np.inf


def compare(m, ref, cloud, T0, name, conditioned, counting=False, out_of_range=0):
    """one Match of `m` against the kept reference; returns the largest observed / bound ratios (H, g, sum_res)"""
    T = np.array(T0, np.float64)
    ok = m.Match(util.cluster_for(N.MODE, cloud), T, update_map=False)
    assert ok == ref.ok, name
    assert (m.stats.iterations, m.stats.n_valid, m.stats.n_source, m.stats.converged) == ref.stats, (name, m.stats.n_valid, ref.stats)
    ids, cnt, valid = m.correspondences()
    bad = np.flatnonzero((ids != ref.ids).any(1))
    assert bad.size == 0, (name, bad[:8], ids[bad[:4]], ref.ids[bad[:4]])
    assert np.array_equal(cnt, ref.cnt) and np.array_equal(valid, ref.valid), name
    Tg, nvg, srg = m.iteration_log()
    assert len(nvg) == len(ref.log[1]) == 1 and np.array_equal(nvg, ref.log[1]), name
    if counting:
        want = (ref.traffic[0] - 7 * out_of_range, ref.traffic[1], ref.traffic[2])  # (a point out of the key range is not probed)
        assert m.traffic_counters() == want, (name, m.traffic_counters(), want)
    H = np.full(36, 7.0); g = np.full(6, 7.0)
    assert _lib.lib().fls_debug_last_system(m._h, _p(H), _p(g)) == 0
    H = H.reshape(6, 6, order="F")
    assert LC.same_bits(H, H.T).all(), (name, H - H.T)
    n = len(cloud)
    Nn = ref.terms + (n + 31) // 32 + 8
    bH, bg = 2 * FC.gamma(Nn) * ref.Ha, 2 * FC.gamma(Nn) * ref.ga
    with np.errstate(divide="ignore", invalid="ignore"):
        rH = np.where(bH > 0, np.abs(H - ref.H) / bH, np.where(H == ref.H, 0.0, np.inf))
        rg = np.where(bg > 0, np.abs(g - ref.g) / bg, np.where(g == ref.g, 0.0, np.inf))
    sr, sr_ref = float(srg[0]), float(ref.log[2][0])
    b_sr = FC.gamma(Nn) * abs(sr_ref)  # every kept r is >= 0: sum |r| is the sum
    r_sr = abs(sr - sr_ref) / b_sr if b_sr > 0 else (0.0 if sr == sr_ref else np.inf)
    print("%s%s: n %d, n_valid %d, cond(H) %.2e; |H - H_o| / (2 gamma_N A) = %.3e, g: %.3e, sum_res / (gamma_N sum|r|): %.3e" %
          (name, " [counting]" if counting else "", n, ref.stats[1], ref.cond, rH.max(), rg.max(), r_sr))
    assert rH.max() <= 1.0 and rg.max() <= 1.0 and r_sr <= 1.0, (name, rH, rg, r_sr)
    if not ref.ok:
        assert np.array_equal(T, np.asarray(T0, np.float64)), name  # below the effective-point floor: T comes back as it went in
        assert np.array_equal(Tg[0], ref.log[0][0]), name
    elif conditioned:
        assert ref.cond < 1e8, (name, ref.cond)
        util.assert_same_registration(m, ref.o, ok, T, ref.ok, ref.T, sets_only_tail=False, max_tie_rows=0)
    return float(rH.max()), float(rg.max()), r_sr


# ---- scoring ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scoring_ref(name):
    c = N.scoring_cases()[name]
    return c, Ref(oracle(c["y"], c["image"]), c["cloud"], c["T"])


@pytest.mark.parametrize("counting", [False, True], ids=["ndt_lanes_kernel", "ndt_kernel+tail"])
@pytest.mark.parametrize("name", N.SCORING_NAMES)
def test_scoring_case(name, counting, monkeypatch):
    c, ref = scoring_ref(name)
    m = make(monkeypatch, c["y"], image=c["image"])
    assert (m.map_size(158), m.map_size(159)) == (1, 0)
    m.set_profiling(False, counters=counting)
    for _ in range(2):
        compare(m, ref, c["cloud"], c["T"], name, c["conditioned"], counting, c["out_of_range"])
    m.close()


@functools.lru_cache(maxsize=None)
def sizes_ref(n):
    c = N.sizes_case(n)
    return c, Ref(oracle(c["y"], c["image"]), c["cloud"], c["T"])


@pytest.mark.parametrize("counting", [False, True], ids=["ndt_lanes_kernel", "ndt_kernel+tail"])
def test_sizes_on_one_handle(counting, monkeypatch):
    """1 .. 4097 points (4097: 65 workgroups of 64 points, above the 8 ticket shards), each size twice and once more after the next size: what a launch
    leaves behind (tickets, partial rows, flags of a longer scan) must not reach the next one"""
    m = make(monkeypatch, N.Y, image=N.sizes_map()[0])
    m.set_profiling(False, counters=counting)
    seq = []
    for i, n in enumerate(N.SIZES):
        seq += [n, n] + ([N.SIZES[i - 1]] if i else [])
    seq.append(N.SIZES[0])
    for n in seq:
        c, ref = sizes_ref(n)
        compare(m, ref, c["cloud"], c["T"], c["name"], c["conditioned"], counting)
    m.close()


@pytest.mark.parametrize("counting", [False, True], ids=["ndt_lanes_kernel", "ndt_kernel+tail"])
def test_effective_floor(counting, monkeypatch):
    """exactly ndt_min_effective_pts pairs registers, one fewer returns false with T unchanged and the iteration logged"""
    c50, c49 = N.effective_floor(50), N.effective_floor(49)
    m = make(monkeypatch, c50["y"], image=c50["image"])
    m.set_profiling(False, counters=counting)
    for c in (c50, c49, c50, c49):
        ref = Ref(oracle(c["y"], c["image"]), c["cloud"], c["T"])
        assert ref.ok == (c is c50) and ref.stats[1] == (50 if c is c50 else 49)
        compare(m, ref, c["cloud"], c["T"], c["name"], False, counting)
        ref.o.close()
    m.close()


def test_effective_floor_then_fitness_on_a_localization_handle(monkeypatch):
    """a Match stopped at the floor leaves final_transformation_ alone: the following GetFitnessScore uses the new source cloud with the previous pose"""
    c50, c49 = N.effective_floor(50), N.effective_floor(49)
    rng = np.random.default_rng(41)
    parts = [N.history_points(v["key"], 4, rng) for v in c50["voxels"]]  # a map built from a cloud: an imported image has no fitness grid
    cloud = np.concatenate(parts)
    m = make(monkeypatch, c50["y"], loc=True)
    o = oracle(c50["y"], loc=True)
    m.AddCloudToLocalMap([cloud]); o.AddCloudToLocalMap(cloud)
    probe = np.array([q.astype(np.float64).mean(0) for q in parts], np.float32)  # on the voxels' means: every point scores in its own voxel alone
    seen = []
    for n in (49, 50, 49):  # (before any Match got through; after one; after one more that did not)
        T = np.eye(4)
        ok = m.Match(util.cluster_for(N.MODE, probe[:n]), T, update_map=False)
        ok_ref, T_ref = o.Match(probe[:n], np.eye(4), update_map=False)
        assert ok == ok_ref and m.stats.n_valid == o.stats.n_valid, (n, ok, ok_ref, m.stats.n_valid, o.stats.n_valid)
        fm, fo = m.GetFitnessScore(2.0), o.GetFitnessScore(2.0)
        print("n %d: ok %s, n_valid %d, fitness %r oracle %r" % (n, ok, m.stats.n_valid, fm, fo))
        assert fm == fo, n
        seen.append((ok, m.stats.n_valid, fm < 1e30))
    assert seen == [(False, 49, False), (True, 50, True), (False, 49, True)], seen
    m.close(); o.close()


@pytest.mark.parametrize("env", [None, SLACK0, HOST], ids=["default", "slack0", "host"])
def test_after_eviction(env, monkeypatch):
    """host: the mirror evicts, the image gets its tombstones through ndt_apply_edits_kernel's table edits"""
    c = N.after_eviction()
    m = make(monkeypatch, c["y"], env, image=c["image"])
    o = oracle(c["y"], c["image"])
    for cl in c["pre_clouds"]:
        m.AddCloudToLocalMap([cl]); o.AddCloudToLocalMap(cl)
    if env is HOST:
        assert m.map_size(109) == 0
    else:
        assert (m.map_size(109), m.map_size(110)) == (2, 0) and m.map_size(117) == 11, "the two batches and their evictions did not run in device rows"
    if env is SLACK0:
        print("table rebuilds %d, row growths %d" % (m.map_size(112), m.map_size(113)))
        assert m.map_size(112) > 0 and m.map_size(113) > 0, "no slack: the table and the rows must have grown on the device"
    assert np.array_equal(m.ExportMap(), o.ndt_image())
    ref = Ref(o, c["cloud"], c["T"])
    for counting in (False, True):
        m.set_profiling(False, counters=counting)
        compare(m, ref, c["cloud"], c["T"], c["name"], True, counting)
    m.close(); o.close()


# ---- histories -----------------------------------------------------------------------------------------------------------------------------------
def same_map(m, o, where):
    img = o.ndt_image()
    blob = m.ExportMap()
    if not np.array_equal(blob, img):
        n = o.map_size()
        assert blob.size == img.size, (where, blob.size, img.size)
        L = _lib.ndt_image_layout(n)
        names = ["header"] + [k for k in ("key", "num_points", "vid", "estimated", "pending", "points", "mu", "sigma", "info")]
        starts = [0] + [L[k] for k in names[1:]] + [img.size]
        diff = {names[i]: int((blob[starts[i]:starts[i + 1]] != img[starts[i]:starts[i + 1]]).sum()) for i in range(len(names))}
        raise AssertionError("%s: the exported image differs from the oracle's, bytes per array: %r" % (where, {k: v for k, v in diff.items() if v}))
    d, v = o.ndt_dump_full(), m.ndt_voxels()  # (ndt_voxels lists the most recently touched first)
    assert np.array_equal(v["keys"][::-1], d["keys"]) and np.array_equal(v["pending"][::-1], d["pending"]), where
    for k in ("vid", "num_points", "estimated"):
        assert np.array_equal(v[k][::-1], d[k]), (where, k)
    for k in ("mu", "sigma", "info"):
        assert LC.same_bits(v[k][::-1], d[k]).all(), (where, k)


@pytest.mark.parametrize("name", N.HISTORY_NAMES)
def test_history(name, monkeypatch):
    h = N.histories()[name]
    dev, host = make(monkeypatch, h["y"], image=h["start"]), make(monkeypatch, h["y"], HOST, image=h["start"])
    o = oracle(h["y"], h["start"])
    assert (dev.map_size(158), dev.map_size(159), host.map_size(158), host.map_size(159)) == (1, 0, 0, 1)
    worst = np.zeros(3)
    for b, cloud in enumerate(h["clouds"]):
        o.AddCloudToLocalMap(cloud)
        ref = Ref(o, h["probe"], np.eye(4))
        for label, m in (("device", dev), ("host", host)):
            where = "%s, batch %d, %s handle" % (name, b, label)
            m.AddCloudToLocalMap([cloud])
            same_map(m, o, where)
            worst = np.maximum(worst, compare(m, ref, h["probe"], np.eye(4), where, False))
        assert (dev.map_size(109), dev.map_size(110)) == (b + 1, 0), (name, b, "the batch did not run as a device batch")
        assert host.map_size(109) == 0
    if name == "eviction_cap40":
        assert dev.map_size(117) > 0 and dev.map_size(126) == 1, "no eviction / re-creation in device rows"
    print("%s: %d batches, %d voxels; worst ratios H %.3e g %.3e sum_res %.3e" % (name, len(h["clouds"]), o.map_size(), *worst))
    dev.close(); host.close(); o.close()


@pytest.mark.parametrize("name", N.HISTORY_NAMES)
def test_history_through_match(name, monkeypatch):
    """the same batches arriving the way a mapping run delivers them: Match(update_map = True) from a general pose.  The map update takes the INPUT pose
    (incremental_ndt.h:327-329), transforms the filtered scan in float and filters it again in the world frame, so the map stays comparable byte for byte
    whatever the iteration's last bits are.  Batch 0 goes in through AddCloudToLocalMap: the main histories start from one voxel far away, nothing to match."""
    h = N.histories()[name]
    dev, host = make(monkeypatch, h["y"], image=h["start"]), make(monkeypatch, h["y"], HOST, image=h["start"])
    o = oracle(h["y"], h["start"])
    updates = 0
    for b, cloud in enumerate(h["clouds"]):
        scan = N.source_for(cloud, N.POSE_GEN)
        if b == 0:
            o.AddCloudToLocalMap(cloud)
        else:
            ok_ref, _ = o.Match(scan, N.POSE_GEN, update_map=True)
            updates += o.stats.map_updated
        for label, m in (("device", dev), ("host", host)):
            where = "%s, batch %d, %s handle" % (name, b, label)
            if b == 0:
                m.AddCloudToLocalMap([cloud])
            else:
                T = N.POSE_GEN.copy()
                ok = m.Match(util.cluster_for(N.MODE, scan), T, update_map=True)
                assert (ok, m.stats.n_valid, m.stats.n_source, m.stats.map_updated) == (ok_ref, o.stats.n_valid, o.stats.n_source, o.stats.map_updated), where
                ids, cnt, valid = m.correspondences()
                ids_ref, cnt_ref, _ = o.correspondences()
                assert np.array_equal(ids, ids_ref) and np.array_equal(cnt, cnt_ref), where
            same_map(m, o, where)
    assert updates >= len(h["clouds"]) - 2, "the history did not reach the map through Match"
    assert (dev.map_size(109), dev.map_size(110)) == (1 + updates, 0) and host.map_size(109) == 0, (dev.map_size(109), dev.map_size(110))
    print("%s: %d map updates through Match (%d fed by the device-resident filtered scan), %d voxels" % (name, updates, dev.map_size(111), o.map_size()))
    dev.close(); host.close(); o.close()
