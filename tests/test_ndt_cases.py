"""tests/ndt_cases.py on the CPU oracle alone: the oracle's image import / full dump round trip, and every constructed case shown to be what it says
-- a case that does not reach its decision fails here, before any device sees it."""
import numpy as np
import pytest

from funny_lidar_slam_amd import registration as reg, synth
from oracle import oracle as O
from tests import ndt_cases as N, util

ARRAYS = ("keys", "vid", "num_points", "estimated", "pending", "points", "mu", "sigma", "info")


def oracle(y, image=None, loc=False):
    o = util.oracle_for(N.MODE, y, loc)
    if image is not None:
        assert o.ndt_import_image(image), "the oracle refused a case's image"
    return o


def same_dump(a, b):
    return [k for k in list(ARRAYS) + ["next_vid", "flag_first_scan"] if not np.array_equal(np.asarray(a[k]).view(np.uint8) if k in ARRAYS else a[k],
                                                                                           np.asarray(b[k]).view(np.uint8) if k in ARRAYS else b[k])]


def index_of(cloud, p):
    i = np.flatnonzero((cloud == np.asarray(p, np.float32)).all(1))
    assert len(i) == 1, (p, i)
    return int(i[0])


# ---- the oracle's import and dump ----------------------------------------------------------------------------------------------------------
def cloud_built():
    y = dict(reg.YAML_NCLT_NDT, ndt_capacity=1300, ndt_max_points_in_voxel=20)
    cfg = synth.make_config(2, scale=0.02)
    o = oracle(y)
    o.AddCloudToLocalMap(cfg["map"])
    T = cfg["T_init"]
    for k in range(2):
        ok, T = o.Match(cfg["scan"] + np.float32(0.3 * k), T, update_map=True)
    return y, cfg, o, T


def test_round_trip_continues_bit_for_bit(built):
    y, cfg, a, T = cloud_built()
    d = a.ndt_dump_full()
    est, sat = d["estimated"] != 0, (d["estimated"] != 0) & (d["num_points"] > 20)
    assert (~est & (d["pending"] > 0)).any() and (est & (d["pending"] > 0)).any() and sat.any() and not d["pending"][sat].any(), "not every entry state is present"
    assert d["flag_first_scan"] == 0 and d["next_vid"] > d["vid"].max()
    img = a.ndt_image()
    b = oracle(y, img)
    assert same_dump(a.ndt_dump_full(), b.ndt_dump_full()) == [] and np.array_equal(b.ndt_image(), img)
    Ta, Tb = T, T
    for k in range(3):
        more = (cfg["map"][k::3] + np.float32(0.11 * (k + 1))).astype(np.float32)
        a.AddCloudToLocalMap(more); b.AddCloudToLocalMap(more)
        assert same_dump(a.ndt_dump_full(), b.ndt_dump_full()) == [], k
        scan = cfg["scan"] + np.float32(0.2 * k)
        oka, Ta = a.Match(scan, Ta, update_map=True)
        okb, Tb = b.Match(scan, Tb, update_map=True)
        assert oka == okb and np.array_equal(Ta, Tb)
        for u, v in zip(a.correspondences(), b.correspondences()):
            assert np.array_equal(u, v)
        for u, v in zip(a.iteration_log(), b.iteration_log()):
            assert np.array_equal(u, v)
        assert same_dump(a.ndt_dump_full(), b.ndt_dump_full()) == [], k
    a.close(); b.close()


def test_localization_image_keeps_first_scan(built):
    y = dict(reg.YAML_NCLT_NDT)
    cfg = synth.make_config(2, scale=0.02)
    a = oracle(y, loc=True)
    a.AddCloudToLocalMap(cfg["map"])
    assert a.ndt_dump_full()["flag_first_scan"] == 1
    b = oracle(y, a.ndt_image(), loc=True)
    crop = cfg["map"][::2].copy()
    a.AddCloudToLocalMap(crop); b.AddCloudToLocalMap(crop)
    assert same_dump(a.ndt_dump_full(), b.ndt_dump_full()) == []
    a.close(); b.close()


def test_refused_image_leaves_the_oracle_unchanged(built):
    y, cfg, a, T = cloud_built()
    good = a.ndt_image()
    d = a.ndt_dump_full()
    n = len(d["vid"])
    L = O.ndt_image_layout(n)
    est = int(np.flatnonzero(d["estimated"] == 1)[3])
    sat = int(np.flatnonzero((d["estimated"] == 1) & (d["num_points"] > 20))[0])

    def poke(offset, value):
        b = good.copy()
        raw = np.atleast_1d(value).view(np.uint8)
        b[offset:offset + raw.size] = raw
        return b
    bad = {
        "magic": poke(2, np.uint8(good[2] ^ 0x40)), "revision": poke(8, np.uint32(2)), "carry": poke(12, np.uint32(5)), "truncated": good[:-16].copy(),
        "n_voxels": poke(24, np.uint64(n + 1)), "n_voxels and total": poke(16, np.array([O.ndt_image_layout(n + 1)["total"], n + 1], np.uint64)),
        "next_vid below n": poke(32, np.int32(n - 1)), "flag_first_scan 2": poke(36, np.uint32(2)), "voxel size": poke(40, np.float64(0.5)),
        "min_points": poke(48, np.int32(4)), "max_points": poke(52, np.int32(21)), "capacity": poke(56, np.int32(1301)), "reserved": poke(60, np.uint32(1)),
        "duplicated key": poke(L["key"] + 8 * (n - 1), O.ndt_pack_keys(d["keys"][3:4])),
        "reserved key": poke(L["key"] + 8 * 5, np.uint64(0xFFFFFFFFFFFFFFFE)), "key out of range": poke(L["key"] + 8 * 5, O.ndt_pack_keys([[N.KEY_LIMIT, 0, 0]])),
        "estimated 2": poke(L["estimated"] + est, np.uint8(2)), "pending 9": poke(L["pending"] + 7, np.uint8(9)),
        "pending beyond max": poke(L["pending"] + sat, np.uint8(1)), "num_points < 0": poke(L["num_points"] + 4 * 9, np.int32(-1)),
        "vid = next_vid": poke(L["vid"] + 4 * 2, np.int32(d["next_vid"])), "vid < 0": poke(L["vid"] + 4 * 2, np.int32(-1)),
        "NaN info": poke(L["info"] + 72 * est + 32, np.float64(np.nan)), "inf mu": poke(L["mu"] + 24 * est + 8, np.float64(np.inf)),
    }
    for name, b in bad.items():
        assert not np.array_equal(b, good), name
        assert not a.ndt_import_image(b), name
        assert same_dump(a.ndt_dump_full(), d) == [], name
    small = oracle(dict(y, ndt_capacity=n))  # an insert evicts as soon as the count reaches the capacity: n voxels do not fit a capacity of n
    assert not small.ndt_import_image(poke(56, np.int32(n)))
    assert a.ndt_import_image(good) and same_dump(a.ndt_dump_full(), d) == []
    a.close(); small.close()


# ---- probe clouds ------------------------------------------------------------------------------------------------------------------------------
def all_probe_clouds():
    out = {c["name"]: c["cloud"] for c in N.scoring_cases().values()}
    out.update({"sizes_%d" % n: N.sizes_case(n)["cloud"] for n in N.SIZES})
    out.update({"effective_%d" % n: N.effective_floor(n)["cloud"] for n in (49, 50)})
    out["after_eviction"] = N.after_eviction()["cloud"]
    for h in N.histories().values():
        out[h["name"] + " probe"] = h["probe"]
    return out


def test_every_probe_point_survives_the_source_filter_as_itself(built):
    for name, cloud in all_probe_clouds().items():
        f = N.filtered(cloud)
        lib_f = reg.VoxelGridCloud(cloud, N.LEAF, on_device=False)[:, :3]
        assert np.array_equal(f, lib_f), name  # the library's host filter and the oracle's agree, order included
        assert len(f) == len(cloud), name
        srt = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]
        assert np.array_equal(srt(f), srt(cloud)), name  # (-0.0 comes back as 0.0: equal, not the same bits)
    for n in N.SIZES:
        assert len(N.filtered(N.sizes_case(n)["cloud"])) == n
    assert np.array_equal(N.scoring_cases()["gate_eq"]["T"], np.eye(4)) and not np.array_equal(N.POSE_GEN, np.eye(4))


def run(case):
    o = oracle(case["y"], case["image"])
    for c in case.get("pre_clouds", []):
        o.AddCloudToLocalMap(c)
    ok, T = o.Match(case["cloud"], case["T"], update_map=False)
    return o, ok, T


def residual(q, v):
    """e^T info e in the kernel's (and the reference's) order of operations"""
    e = np.asarray(q, np.float64) - v["mu"]
    I = v["info"]
    with np.errstate(over="ignore", invalid="ignore"):
        ei = [(e[0] * I[3 * c] + e[1] * I[3 * c + 1]) + e[2] * I[3 * c + 2] for c in range(3)]
        return (ei[0] * e[0] + ei[1] * e[1]) + ei[2] * e[2]


def test_gate_cases_sit_on_the_threshold_in_the_bits(built):
    cases = N.scoring_cases()
    for name, kept in (("gate_eq", True), ("gate_next", False)):
        c = cases[name]
        o, ok, T = run(c)
        f = N.filtered(c["cloud"])
        ids, cnt, valid = o.correspondences()
        for s in range(7):
            v = c["voxels"][84 + s]
            p = c["gate_points"][s]
            r = residual(p, v)
            assert (r == N.THR) if kept else (r > N.THR and r < N.THR * (1 + 1e-4)), (name, s, r)
            assert tuple(N.key_of(p) + N.NB[s]) == v["key"]
            row = ids[index_of(f, p)]
            want = np.full(7, -1); want[s] = 84 + s if kept else -1
            assert np.array_equal(row, want), (name, s, row)
        assert ok and o.stats.n_valid == 84 + (7 if kept else 0)
        o.close()


def test_nan_case_is_nan_and_rejected(built):
    c = N.scoring_cases()["nan_residual"]
    rA, rB = residual(c["nan_points"][0], c["voxels"][84]), residual(c["nan_points"][1], c["voxels"][85])
    assert np.isnan(rA) and np.isposinf(rB)
    assert np.isfinite(c["voxels"][84]["info"]).all() and np.isfinite(c["voxels"][85]["info"]).all()
    o, ok, T = run(c)
    ids, cnt, valid = o.correspondences()
    f = N.filtered(c["cloud"])
    for p in c["nan_points"]:
        assert (ids[index_of(f, p)] == -1).all()
    assert ok and o.stats.n_valid == 84 and int(o.counters().hit_voxels) == 86 and np.isfinite(T).all() and np.isfinite(o.last_system()[0]).all()
    o.close()


def test_truncation_unestimated_and_key_edge_reach_what_they_say(built):
    cases = N.scoring_cases()
    for which in "ab":
        c = cases["truncation_" + which]
        o, ok, T = run(c)
        ids, cnt, valid = o.correspondences()
        f = N.filtered(c["cloud"])
        keyvid = {v["key"]: i for i, v in enumerate(c["voxels"])}
        tr = np.flatnonzero(np.abs(f).max(1) < 2.0)
        assert len(tr) == 343
        for i in tr:
            k = N.key_of(f[i])  # truncation toward zero: +-0.3, +-0.9 and 0.0 share key 0; -1.0 and -1.3 share key -1
            assert (np.abs(k) <= 1).all()
            for s in range(7):
                assert ids[i, s] in (-1, keyvid[tuple(k + N.NB[s])]), (f[i], s)
        assert (cnt[tr] >= 1).all() and (cnt[tr] == 7).any() and (ids[tr] == -1).any()  # every point scores; some in all seven voxels, some gated
        o.close()
    c = cases["unestimated"]
    o, ok, T = run(c)
    ids, _, _ = o.correspondences()
    assert not np.isin(ids, c["waiting_vids"]).any() and np.isin(ids, [84, 86, 88, 90, 92]).any()
    near = [i for i, p in enumerate(N.filtered(c["cloud"])) if tuple(N.key_of(c["T"][:3, :3] @ p.astype(np.float64) + c["T"][:3, 3])) in
            [c["voxels"][v]["key"] for v in c["waiting_vids"]]]
    assert len(near) == 4 and (ids[near, 0] == -1).all() and (ids[near, 1] >= 0).all() and (ids[near, 2] >= 0).all()
    o.close()
    c = cases["key_edge"]
    o, ok, T = run(c)
    ids, cnt, _ = o.correspondences()
    f = N.filtered(c["cloud"])
    big = np.abs(f).max(1)
    inside, outside = np.flatnonzero((big > 1e6) & (big < N.KEY_LIMIT)), np.flatnonzero(big > N.KEY_LIMIT)
    assert len(inside) == 6 and len(outside) == 6 == c["out_of_range"]
    assert (ids[inside, 0] >= 84).all() and (cnt[inside] == 1).all() and (ids[outside] == -1).all() and (cnt[outside] == 0).all()
    assert not o.ndt_import_image(N.image_of([N.voxel((N.KEY_LIMIT, 0, 0))], c["y"])), "KEY_LIMIT - 1 is not the largest key an image may hold"
    o.close()


def test_effective_floor_is_exact(built):
    for n, want in ((50, True), (49, False)):
        c = N.effective_floor(n)
        o, ok, T = run(c)
        assert o.stats.n_valid == n and ok == want and c["y"]["ndt_min_effective_pts"] == 50
        if not want:
            assert np.array_equal(T, c["T"])
        o.close()


def test_after_eviction_evicts_and_recreates(built):
    c = N.after_eviction()
    o = oracle(c["y"], c["image"])
    assert o.map_size() == c["y"]["ndt_capacity"] - 1
    before = o.ndt_dump_full()
    for cl in c["pre_clouds"]:
        o.AddCloudToLocalMap(cl)
    d = o.ndt_dump_full()
    keys = {tuple(k): i for i, k in enumerate(d["keys"])}
    assert not any(k in keys for k in c["evicted_keys"])
    r = keys[c["recreated_key"]]
    assert d["vid"][r] >= before["next_vid"] and d["estimated"][r] == 1
    ok, T = o.Match(c["cloud"], c["T"], update_map=False)
    ids, cnt, _ = o.correspondences()
    assert ok and (ids == d["vid"][r]).any() and not np.isin(ids, np.arange(0, 11)).any() and np.isin(ids, [11, 12, 13]).any()
    assert (ids >= before["next_vid"]).sum() >= 11
    A, B, D = c["chain"]  # one probe chain: A's entry becomes a tombstone in front of (or between) B's and D's
    hs = N.hash_key(O.ndt_pack_keys([A, B, D])) & np.uint32((1 << 20) - 1)
    assert hs[0] == hs[1] == hs[2] and A in c["evicted_keys"] and A not in keys
    assert d["vid"][keys[B]] == 20 and d["vid"][keys[D]] >= before["next_vid"] and (ids == 20).any() and (ids == d["vid"][keys[D]]).any()
    o.close()


@pytest.mark.parametrize("name", [n for n in N.SCORING_NAMES] + ["after_eviction", "sizes_63", "sizes_4097"])
def test_named_cases_are_conditioned(built, name):
    c = N.scoring_cases()[name] if name in N.SCORING_NAMES else (N.after_eviction() if name == "after_eviction" else N.sizes_case(int(name[6:])))
    assert c["conditioned"]
    o, ok, T = run(c)
    H, g = o.last_system()
    cond = np.linalg.cond(H)
    print(name, "cond(H) = %.3e, n_valid %d" % (cond, o.stats.n_valid))
    assert ok and o.stats.n_valid >= 50
    if name not in N.COND_EXEMPT:
        assert cond < 1e8
    o.close()


# ---- histories -----------------------------------------------------------------------------------------------------------------------------------
def by_key(d):
    return {tuple(k): {a: d[a][i] for a in ARRAYS} | {"rank": i} for i, k in enumerate(d["keys"])}


def walk(h):
    """the branches of UpdateVoxel every batch of a history takes, read off the oracle's dumps before and after"""
    y = h["y"]
    minp, maxp = y["ndt_min_points_in_voxel"], y["ndt_max_points_in_voxel"]
    o = oracle(y, h["start"])
    seen = set()
    for cloud in h["clouds"]:
        prev = by_key(o.ndt_dump_full())
        f = N.filtered(cloud)
        assert len(f) == len(cloud)
        fk = [tuple(k) for k in N.key_of(f)]
        o.AddCloudToLocalMap(cloud)
        d = o.ndt_dump_full()
        now = by_key(d)
        assert d["flag_first_scan"] == 0
        if fk[0] == fk[-1] and len(set(fk)) > 1:
            assert now[fk[-1]]["rank"] == len(now) - 1  # most recently touched
            seen.add("first and last point")
        for k in dict.fromkeys(fk):
            added, a, b = fk.count(k), prev.get(k), now[k]
            if a is None or b["vid"] != a["vid"]:
                seen.add("created" if a is None else "re-created")
                a = dict(estimated=0, pending=0, num_points=0, mu=np.zeros(3), sigma=np.zeros(9), info=np.zeros(9))
            npts = int(a["pending"]) + added
            if not a["estimated"] and not b["estimated"]:
                assert npts <= minp and b["pending"] == npts and b["num_points"] == a["num_points"] + added
                seen.add("wait"); seen.add("wait at min") if npts == minp else None
            elif not a["estimated"]:
                assert npts > minp and b["pending"] == 0
                seen.add("estimate"); seen.add("estimate at min + 1") if npts == minp + 1 else None
                if not b["sigma"].any():
                    seen.add("sigma 0")
            elif a["num_points"] > maxp:
                assert all(np.array_equal(a[x], b[x]) for x in ("mu", "sigma", "info", "num_points")) and b["pending"] == 0
                seen.add("frozen")
            elif npts <= minp:
                assert b["pending"] == npts and np.array_equal(a["info"], b["info"])
                seen.add("pending beside an estimate"); seen.add("carry full") if npts == 8 else None
            else:
                assert b["num_points"] == a["num_points"] + npts and b["pending"] == 0
                seen.add("merge")
                seen.add("merge of min + 1") if npts == minp + 1 else None
                seen.add("merge of 150") if npts >= 150 else None
                seen.add("merge from max") if a["num_points"] == maxp else None
                seen.add("lands on max") if b["num_points"] == maxp else None
                seen.add("lands on max + 1") if b["num_points"] == maxp + 1 else None
                seen.add("merge onto sigma 0") if not a["sigma"].any() else None
                seen.add("merge near 2.5 km") if abs(k[0]) > 2000 else None
                S = O.svd3(b["sigma"].reshape(3, 3, order="F"))[1]
                if S[2] < S[0] * 1e-3:
                    seen.add("clamp on S[2]")
                if S[1] < S[0] * 1e-3:
                    seen.add("clamp on S[1]")
                assert np.isfinite(b["info"]).all()
        gone = [k for k in prev if k not in now]
        if gone:
            seen.add("evicted")
    o.close()
    return seen, now


MAIN = {"wait", "wait at min", "estimate", "estimate at min + 1", "pending beside an estimate", "merge", "merge of min + 1", "merge of 150", "merge from max",
        "lands on max", "lands on max + 1", "frozen", "clamp on S[2]", "clamp on S[1]", "sigma 0", "merge onto sigma 0", "merge near 2.5 km",
        "first and last point", "created"}


@pytest.mark.parametrize("name", N.HISTORY_NAMES)
def test_history_reaches_every_branch(built, name):
    h = N.histories()[name]
    assert len(h["clouds"]) <= 12
    seen, last = walk(h)
    print(name, sorted(seen))
    if name.startswith("main"):
        assert MAIN <= seen, MAIN - seen
        assert len(last) >= 30  # "a few dozen"
    if name == "main_min8" or name == "started_min8":
        assert "carry full" in seen
    if name == "started_min8":
        assert {"merge from max", "frozen", "estimate", "pending beside an estimate", "wait"} <= seen
    if name == "eviction_cap40":
        assert {"evicted", "re-created", "created", "merge", "estimate"} <= seen
        assert h["skipped_key"] in last and last[h["skipped_key"]]["vid"] == 0 and last[h["recreated_key"]]["vid"] >= 39
        assert not any(k in last for k in h["evicted_keys"])
