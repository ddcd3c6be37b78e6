"""The frames of tests/feature_cases.py without a GPU: the numpy model equals the oracle (oracle/flo_features.h) bit for bit on every frame, and
every frame shows, in the model's event record, the property it is named for.  A frame that does not reach its property fails here, before
tests/test_gpu_feature_stages.py runs it on a device."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import feature_cases as FC
from tests import refpin

F32 = np.float32


def _all_events(names):
    return {(n, k): ev for n in names for k, ev in FC.modelled(n)[2].items()}


@pytest.mark.parametrize("name", list(FC.FRAMES) + list(FC.REUSE))
def test_model_equals_oracle(name):
    m, _, _ = FC.modelled(name)
    o = FC.oracle_arrays(name)
    for k in O.FEAT_ARRAYS:
        assert m[k].dtype == o[k].dtype and m[k].shape == o[k].shape and np.array_equal(m[k].view(np.uint8), o[k].view(np.uint8)), (name, k)
    assert o["extracted"] == (o["n_ordered"] >= 12)


def test_raw_from_image_hits_bits_and_columns_and_raises():
    """every column of 64, 900, 1800 and 4096 on a 2^-6 depth grid between 4 and 100 m: depth bits and column as designed"""
    rng = np.random.default_rng(1)
    for cols in (64, 900, 1800, 4096):
        d = (rng.integers(4 * 64, 100 * 64 + 1, cols) / 64.0).astype(F32)
        raw = FC.raw_from_image([(1, c, d[c]) for c in range(cols)], cols, FC.h_res_for(cols))
        assert np.array_equal(FC.depth_f32(raw["x"], raw["y"], raw["z"]).view(np.uint32), d.view(np.uint32))
        got = [O.lib().flo_col_index(float(x), float(y), FC.h_res_for(cols), cols) for x, y in zip(raw["x"][::7], raw["y"][::7])]
        assert got == list(range(0, cols, 7))
    with pytest.raises(ValueError):
        FC.raw_from_image([(0, 3, F32(0.0))], 64, FC.h_res_for(64))  # depth 0 cannot be hit from a column's centre


def test_cap_sectors():
    f = FC.frame("cap")
    m, _, ev = FC.modelled("cap")
    for (ring, s), want in f.info["candidates"].items():
        if want == 0:
            assert ev[(ring, s)]["corners"] == 0
            continue
        e = ev[(ring, s)]
        assert e["corners"] == min(want, 20) and e["cap_hit"] == (want > 20), (ring, s, want, e["corners"], e["cap_hit"])
        assert e["ties_corner"] == 0  # distinct heights: no tie decides which twenty
    # cap_hit: the walk met a 21st element above the threshold with its flag still set, which a wrong cap would have accepted and emitted
    assert len(m["corner_idx"]) == 2 * (19 + 20 + 20 + 20) and m["row_start"][2] == m["row_start"][1] == 5 + 11 + 6 * 256


def test_boundary_elements():
    f = FC.frame("boundary")
    m, _, ev = FC.modelled("boundary")
    for ring in (0, 1):
        e = [ev[(ring, s)] for s in range(6)]
        assert all(x["t"] == 16 for x in e)
        assert e[0]["b1_corner"] and e[0]["corners"] == 2 and not e[1]["b0_planar_again"]   # taken first, not emitted by either sector
        assert e[1]["b1_candidate_invalid"] and not e[1]["b1_corner"] and e[1]["b1_planar_emitted"] and e[2]["b0_planar_again"]
        assert e[2]["b1_planar_accept"] and e[2]["b1_planar_emitted"] and e[3]["b0_planar_again"]
        assert not e[3]["b1_planar_accept"] and not e[3]["b1_corner"] and e[3]["b1_planar_emitted"] and e[4]["b0_planar_again"]
        assert e[4]["b1_corner"] and e[4]["corners"] == 3 and e[4]["accept_lanes"]["corner"] == {0, 1, 2}   # b1 first, though not the largest
        assert e[5]["b1_corner"]                                                            # the last sector's b1
    rs, re_ = m["row_start"], m["row_end"]
    t = f.info["t"]
    assert re_[1] - (rs[1] + 6 * t) == 5 and re_[0] == rs[0] + 6 * t  # ring 1: a remainder behind the last b1, ring 0: none
    # duplicates in the planar list: exactly the boundary elements both neighbours emitted
    idx, cnt = np.unique(m["planar_idx"], return_counts=True)
    assert (cnt <= 2).all() and (cnt == 2).sum() == 2 * 3


def test_gap_offsets():
    f = FC.frame("gaps")
    m, _, ev = FC.modelled("gaps")
    cuts, passed = FC.merged(ev, "cuts"), FC.merged(ev, "passed10")
    for loop in ("corner", "planar"):
        for side in ("f", "b"):
            assert {k for (l, s, k, step) in cuts if l == loop and s == side and step == 11} == {1, 2, 3, 4, 5}, (loop, side, "cut at 11")
            assert {k for (l, s, k) in passed if l == loop and s == side} == {1, 2, 3, 4, 5}, (loop, side, "no cut at 10")
    assert {(kf, kb) for (l, kf, kb) in FC.merged(ev, "both_sides") if l == "corner"} >= {(k, k) for k in range(1, 6)}
    col, isc = m["col"].astype(int), m["is_corner"]
    for (kind, k, g), q in f.info["where"].items():
        q += int(m["row_start"][1]) - 5
        assert isc[q], (kind, k, g)
        if "f" in kind:  # a step of 11 cuts, B survives and is accepted; a step of 10 does not, B is cleared
            assert col[q + k] - col[q + k - 1] == g and isc[q + k] == (g == 11), (kind, k, g)
        if "b" in kind:
            assert col[q - k + 1] - col[q - k] == g and isc[q - k] == (g == 11), (kind, k, g)


def test_chunk_lengths_and_suppressions_ahead():
    names = list(FC.CHUNK_LENGTHS)
    seen_t = set()
    for n in names:
        m, _, ev = FC.modelled(n)
        ts = sorted({e["t"] for e in ev.values()})
        assert tuple(ts) == tuple(sorted(FC.CHUNK_LENGTHS[n])), (n, ts)
        seen_t |= set(ts)
    assert seen_t == {1, 2, 62, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 680}
    m, _, _ = FC.modelled("chunks_c")
    assert m["row_end"][1] + 6 - (m["row_start"][1] - 5) == 4096   # t = 680 on a fully occupied 4096-column ring
    ev = _all_events(names)
    ahead = set().union(*[e["ahead"] for e in ev.values()])
    for loop in ("corner", "planar"):
        for where in ("same", "later"):
            for side in ("lo", "hi"):
                assert (loop, where, True, side) in ahead, (loop, where, side)  # a candidate the walk would have taken, cleared while ahead
        lanes = set().union(*[e["accept_lanes"][loop] for e in ev.values()])
        assert {0, 63} <= lanes, (loop, sorted(lanes))
    # every length of more than one chunk: the planar walk accepts in its last chunk; the corner walk accepts behind its first chunk somewhere
    for t in (255, 256, 257, 512, 680):   # (planar candidates sit at the low end of the order: the chunks they fill grow with the flat share)
        assert any(e["t"] == t and max(e["accept_chunks"]["planar"], default=0) >= 1 for e in ev.values()), t
    for t in (64, 65):   # the second chunk holds one or two elements: cleared from the first chunk while still ahead
        assert any(e["t"] == t and ("planar", "later", True, "hi") in e["ahead"] for e in ev.values()), t
    assert any(max(e["accept_chunks"]["corner"], default=0) >= 1 for e in ev.values())
    assert any(e["cap_hit"] for e in ev.values()) and any(e["t"] == 2 and e["corners"] == 1 for e in ev.values())


def test_ties_decide():
    f = FC.frame("ties")
    m, _, ev = FC.modelled("ties")
    t = f.info["t"]
    for s in range(6):
        assert ev[(0, s)]["cap_hit"] and ev[(0, s)]["corners"] == 20                      # the spike pattern: 20 corners in every sector
        assert ev[(1, s)]["ties_corner"] >= t - 2 and ev[(1, s)]["cap_hit"]              # the plateau above the corner threshold
        assert s in (1, 4) or ev[(2, s)]["ties_planar"] >= t - 12                        # the plateau below the planar threshold
    assert ev[(2, 1)]["cap_hit"] and ev[(2, 1)]["ties_corner"] == 48 and ev[(2, 4)]["cap_hit"]
    assert sum(e["ties_corner"] for e in ev.values()) > 2000
    o = FC.oracle_arrays("ties")
    assert set(np.unique(o["depth"][:1800]).tolist()) == {20.0, 20.25} and o["tie_pairs"] > 2352
    # the order of the ties decides: libstdc++'s std::sort order (the reference's) selects other corners than the stable order
    o1 = FC.oracle_arrays("ties", 1)
    assert not np.array_equal(o["corner_idx"], o1["corner_idx"])


def test_threshold_equalities():
    for name, selected in (("thresholds_eq", False), ("thresholds_next", True)):
        f = FC.frame(name)
        m, _, ev = FC.modelled(name)
        rough = m["roughness"]
        for q, kind in f.info["centres"]:
            grp = np.arange(q - 5, q + 6)
            if kind == "corner":
                assert rough[q] == F32(FC.TH_CORNER) and bool(m["is_corner"][q]) == selected, (name, q)
            else:
                assert (rough[grp[grp != q]] == F32(FC.TH_PLANAR)).all() and rough[q] > F32(FC.TH_PLANAR), (name, q)
            assert (m["valid_pre"][grp] == 1).all() and (m["valid_post"][grp] == (0 if selected else 1)).all(), (name, q, kind)
        eqc, eqp = sum(e["eq_corner_thr"] for e in ev.values()), sum(e["eq_planar_thr"] for e in ev.values())
        assert (eqc >= 6 and eqp >= 60) if not selected else (eqc == 0 and eqp == 0)
    p = FC.frame("thresholds_next").params
    assert F32(p["corner_thres"]) == np.nextafter(F32(FC.TH_CORNER), F32(0)) and F32(p["planar_thres"]) == np.nextafter(F32(FC.TH_PLANAR), F32(1))


def test_short_rings():
    for name in ("short_rings_a", "short_rings_b", "short_rings_c"):
        f = FC.frame(name)
        m, _, ev = FC.modelled(name)
        cnt = (m["row_end"] + 6) - (m["row_start"] - 5)
        assert cnt.tolist() == f.info["counts"] and set(FC.SHORT_COUNTS) <= set(cnt.tolist())
        assert (m["row_end"] < m["row_start"]).sum() >= 5
        ts = {ring: e["t"] for (ring, s), e in ev.items()}
        assert sorted(ts[r] for r in ts if cnt[r] < 20) == [1, 1]   # 17 and 18 cells: t = 1; everything shorter has no sector
        assert any(e["t"] == 1 and e["corners"] for e in ev.values())
    for name, n in (("tiny11", 11), ("tiny12", 12)):
        o = FC.oracle_arrays(name)
        assert o["n_ordered"] == n and o["extracted"] == (n == 12) and (o["row_end"] < o["row_start"]).all()


def test_flag_probes():
    f = FC.frame("flags")
    m, fev, _ = FC.modelled("flags")
    f03 = F32(0.3)
    below = np.nextafter(f03, F32(0))
    assert 0.02 * 25.0 == 0.5
    for rule, j, step, marks in f.info["probes"]:
        diff = fev["diff_a" if rule == "a" else "diff_b"][j]
        fired = fev["rule_a" if rule == "a" else "rule_b"][j]
        assert fev["cd"][j] == step and fired == marks, (rule, j, step)
        assert diff == (f03 if (marks or step == 10) else below), (rule, j, float(diff))
        hit = m["valid_pre"][j - 5:j + 1] if rule == "a" else m["valid_pre"][j + 1:j + 7]
        assert (hit == 0).all() == marks, (rule, j, step)
    n0, n1 = f.info["n0"], f.info["n1"]
    for j, isolated, marks in f.info["cprobes"]:
        j += n0
        assert fev["rule_c"][j] == marks, (j, isolated)
        if isolated:
            assert not fev["rule_a"][j - 1:j + 1].any() and not fev["rule_b"][j - 1:j + 1].any() and fev["cd"][j] == 10
            assert bool(m["valid_pre"][j]) == (not marks), j
        else:
            assert fev["rule_a"][j - 1] or fev["rule_b"][j - 1]
    eq = (fev["f1"] == F32(0.5)) & (fev["f2"] == F32(0.5)) & (m["depth"] == F32(25.0))
    assert eq.any() and not fev["rule_c"][eq].any()                    # both differences AT 0.02 d: not marked
    assert (fev["hits"] >= 2).any() and (fev["rule_c"] & (fev["hits"] >= 2)).any()   # two rules zero the same flag
    last1 = n0 + n1 - 1
    assert fev["rule_a"][last1] and fev["cd"][last1] == 5 and (m["valid_pre"][last1 - 5:last1 + 1] == 0).all()   # across the ring boundary
    n = len(m["depth"])
    assert fev["rule_b"][n - 7]                                         # marks n - 6 .. n - 1
    assert fev["rule_a"][7] and fev["diff_a"][7] == f03                 # marks 2 .. 7: into the first five


def test_projection_frames():
    g = FC.frame("gates")
    o = FC.oracle_arrays("gates")
    d = FC.depth_f32(g.raw["x"], g.raw["y"], g.raw["z"])[:6]
    assert d[0] == F32(4.0) and d[3] == F32(100.0) and d[1] < F32(4.0) and d[4] > F32(100.0)
    assert [int(k) in o["raw_index"].tolist() for k in range(6)] == g.info["kept"]
    for cols, name in ((64, "columns64"), (257, "columns257"), (900, "columns900"), (1800, "columns1800"), (4096, "columns4096_one_row")):
        o = FC.oracle_arrays(name)
        assert np.array_equal(o["col"][:cols], np.arange(cols)) and o["n_ordered"] == cols * (1 if cols == 4096 else 2)
    o = FC.oracle_arrays("edges")
    f = FC.frame("edges")
    c = FC.col_index(f.raw["x"][:514], f.raw["y"][:514], f.params["horizontal_resolution"], 257).reshape(257, 2)
    assert o["n_ordered"] <= len(f.raw) - 3 and (np.abs(c[:, 1] - c[:, 0]) == 1).sum() >= 1     # the two sides of an edge
    assert not (set(range(len(f.raw) - 4, len(f.raw) - 1)) & set(o["raw_index"].tolist()))   # rings rows, 65535, rows + 1: dropped
    for name in ("h_res_fine", "h_res_coarse"):
        f = FC.frame(name)
        o = FC.oracle_arrays(name)
        if name == "h_res_fine":
            assert f.info["below"] > 100 and f.info["beyond"] > 100 and f.info["wrapped"] > 100
        else:
            assert f.info["below"] == f.info["beyond"] == 0 and o["col"].min() >= 96 and o["col"].max() <= 160
    for name in ("returns", "returns_layout_b"):
        f = FC.frame(name)
        o = FC.oracle_arrays(name)
        raw, p = f.raw, f.params
        cell = raw["ring"].astype(np.int64) * p["horizontal_scan"] + FC.col_index(raw["x"], raw["y"], p["horizontal_resolution"], p["horizontal_scan"])
        real = np.isin(raw["ring"], (0, 1, 127))
        per = np.unique(cell[real], return_counts=True)[1]
        assert set(per.tolist()) == set(range(2, 10))
        win = o["raw_index"][np.isin(raw["ring"][o["raw_index"]], (0, 1, 127))]
        assert len(win) == f.info["ncell"] and (win < 300).all() and (np.diff(win) < 0).any()   # first returns, not in cell order
        other_block = [np.all(np.nonzero(cell == cell[w])[0][1:] // 256 != w // 256) for w in win]
        assert sum(other_block) > 200
        z = raw["z"][cell == cell[win[0]]]
        assert len(set(z.tolist())) > 1
        assert {63, 64, 255, 256, 257, p["horizontal_scan"] - 1} == set(o["col"][raw["ring"][o["raw_index"]] == 2].tolist())
    assert FC.frame("returns_layout_b").raw.dtype.itemsize == 40 and FC.frame("returns").params["vertical_scan"] == 128


def test_fuzz_seeds_cover_the_parameter_space():
    """the eight ffuzz seeds the device runs: both lidar models, every threshold value, a frame with nine returns in ten dropped"""
    assert len(FC.FUZZ_SEEDS) == 8
    ps, sizes = [], []
    for s in FC.FUZZ_SEEDS:
        raw, p = refpin.make_feature_case(f"ffuzz{s}")
        ps.append(p)
        sizes.append(len(raw) / (p["vertical_scan"] * 1800.0))
    assert {p["vertical_scan"] for p in ps} == {16, 64}
    assert {p["corner_thres"] for p in ps} == {0.5, 1.0, 2.0} and {p["planar_thres"] for p in ps} == {0.05, 0.1, 0.3}
    assert {p["min_distance"] for p in ps} == {2.0, 4.0, 8.0} and {p["max_distance"] for p in ps} >= {30.0, 100.0}
    assert min(sizes) < 0.06   # a 16-ring scan has 900 azimuths: 0.43 of rings x 1800 at most; a tenth of that is the 0.9 drop rate
