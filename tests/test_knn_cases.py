"""tests/knn_cases.py without a GPU: the numpy model of the grid k-NN equals the oracle's brute force on every query of every case (and its
kd-tree where no tie sits at the 5th place), every case has the property it is named for, no NaN appears anywhere, and the contract of
tests/test_gpu_knn_stages.py leaves no query of a gated case out."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import knn_cases as KC

U32 = np.uint32
ALL = tuple(KC.CASES)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(U32)


def _cells(x, cell):
    return KC.file_query(x, cell).astype(np.int64)


@pytest.mark.parametrize("name", ALL)
def test_model_equals_the_oracle(built, name):
    c = KC.CASES[name]()
    Qt, ids, dd = KC.model5(name)
    assert not np.isnan(c.map).any() and not np.isnan(c.query).any() and not np.isnan(Qt).any() and not np.isnan(dd).any()
    assert np.isfinite(c.map).all() and np.isfinite(c.query).all()
    nm = len(c.map)
    assert len(Qt) >= 1 and nm >= 1, name
    for i in range(len(Qt)):
        oi, od = O.knn_bruteforce(c.map, Qt[i], 5)
        k = min(5, nm)
        assert len(oi) == k and np.array_equal(oi, ids[i, :k]) and np.array_equal(_bits(od), _bits(dd[i, :k])), (name, i)
    if nm >= 6:
        ids6, dd6 = KC.brute_knn(Qt, c.map, 6)
        clear = (dd6[:, 4] != dd6[:, 5]) & np.isfinite(dd6[:, 5])  # no tie at the 5th / 6th place: the set is the kd-tree's too
        ki, kd = O.kdtree_knn(c.map, Qt, 5)
        assert np.array_equal(np.sort(ki[clear], axis=1), np.sort(ids[clear], axis=1)), name
        assert np.array_equal(_bits(kd[clear]), _bits(dd[clear])), name
    Q1, id1, d1 = KC.model1(name)
    assert not np.isnan(Q1).any() and not np.isnan(d1).any()
    for i in range(0, len(Q1), 7):
        oi, od = O.knn_bruteforce(c.map, Q1[i], 1)
        assert oi[0] == id1[i] and _bits(od)[0] == _bits(d1[i:i + 1])[0], (name, i)


@pytest.mark.parametrize("name,setting", KC.runs())
def test_the_contract_is_total(name, setting):
    """every query of a gated run is in exactly one of the two classes the GPU test checks; an un-gated run compares every query"""
    _, ids, dd = KC.model5(name)
    gate = KC.SETTINGS[setting][2]
    if np.isfinite(gate):
        full, rest = KC.gated_classes(dd, gate)
        assert (full ^ rest).all() and len(full) == len(ids)
        assert (ids[full] >= 0).all()


def test_uniform():
    c = KC.uniform()
    Qt, ids, dd = KC.model5("uniform")
    assert len(c.map) == 3000 and len(c.query) == KC.UNIFORM_COUNTS[-1] == 2081 and 2081 > 2048  # more than 64 workgroups of 32 queries
    assert not np.array_equal(c.T, KC.IDENTITY)
    lo, hi = c.map.min(axis=0), c.map.max(axis=0)
    outside = ((Qt < lo) | (Qt > hi)).any(axis=1)
    assert 100 < outside.sum() < len(Qt) - 100
    for n in KC.UNIFORM_COUNTS[1:]:  # every prefix meets both gated classes
        full, rest = KC.gated_classes(dd[:n], KC.GATE)
        assert full.any() and rest.any(), n
    ring = KC.fifth_ring("uniform", "g2")
    assert (ring >= 2).any() and (ring <= 1).any()  # LoamFull's second stage is needed for some queries and not for others


def test_lattice_ties():
    c = KC.lattice_ties()
    Qt, _, _ = KC.model5("lattice_ties")
    ids6, dd6 = KC.brute_knn(Qt, c.map, 6)
    assert (c.map * 8 == np.round(c.map * 8)).all() and (Qt * 8 == np.round(Qt * 8)).all()  # exact coordinates
    assert ((dd6[:, :5] == dd6[:, 1:]).any(axis=1)).all(), "every list is decided by a tie"
    tie56 = dd6[:, 4] == dd6[:, 5]
    assert tie56.sum() > 200
    _, inverse, counts = np.unique(c.map, axis=0, return_inverse=True, return_counts=True)
    assert set(range(2, 10)) <= set(counts.tolist()), "points duplicated two to nine times"
    assert len(np.unique(c.map, axis=0)) == 13 ** 3
    for cell in (KC.CELL1, KC.CELL2):
        a, b = _cells(c.map[ids6[tie56, 4]], cell), _cells(c.map[ids6[tie56, 5]], cell)
        across = (a != b).any(axis=1)
        same_point = (c.map[ids6[tie56, 4]] == c.map[ids6[tie56, 5]]).all(axis=1)
        assert across.sum() > 20 and same_point.sum() > 5, "ties at the 5th place across neighbouring cells and inside one cell"
    # the shuffled indices: a tie is not decided by position in space
    assert not np.array_equal(np.argsort(c.map[:, 0], kind="stable"), np.arange(len(c.map)))


@pytest.mark.parametrize("setting", ("g1", "g2", "u1"))
def test_quad_tails(setting):
    c = KC.quad_tails(setting)
    cell = c.info["cell"]
    assert cell == KC.SETTINGS[setting][0]
    mc, qc = _cells(c.map, cell), _cells(c.query, cell)
    seen = {}
    for k, (label, n, base, off) in enumerate(c.info["layout"]):
        assert tuple(qc[k]) == base, "the query sits in the cluster's base cell"
        target = np.array(base) + np.array(off)
        assert ((mc == target).all(axis=1)).sum() == n, (label, n)
        near = (np.abs(mc - np.array(base)).max(axis=1) <= 5)
        assert near.sum() == sum(f(n) for _, f in dict(KC.QUAD_CLASSES)[label]), "isolated: nothing else within 5 cells"
        seen.setdefault(label, set()).add(n)
    assert all(v == set(range(1, 10)) for v in seen.values()) and set(seen) == {lab for lab, _ in KC.QUAD_CLASSES}
    # the float filing of the parent's builders agrees on these points (they keep 0.2 cells from every face)
    assert np.array_equal(KC.file_float(c.map, cell), KC.file_query(c.map, cell))


def test_small_map():
    assert len(KC.small_map().map) < 5


def test_prune_edges():
    c = KC.prune_edges()
    Qt, ids, dd = KC.model5("prune_edges")
    ids6, dd6 = KC.brute_knn(Qt, c.map, 6)
    assert np.array_equal(Qt, c.query)
    kinds = {1: 0, 2: 0, 3: 0}
    for cell in (KC.CELL1, KC.CELL2):
        f = Qt.astype(np.float64) / float(cell)
        gap = np.abs(f - np.round(f)) * float(cell)
        near = gap <= 1.0001e-4 * float(np.float64(KC.CELL1))
        assert near.any(axis=1).all(), "every query is within 1e-4 cells of a face"
    variants = set()
    for i, (s, v, across) in enumerate(c.info["layout"]):
        s = np.array(s)
        kinds[int(np.abs(s).sum())] += 1
        variants.add(v)
        for cell in (KC.CELL1, KC.CELL2):
            qc, ac = _cells(Qt[i], cell), _cells(c.map[across], cell)
            assert np.array_equal(ac - qc, s), "the point across lies in the neighbouring cell in the direction(s) of the near face(s)"
            own = [j for j in ids[i] if j != across]
            assert all(np.array_equal(_cells(c.map[j], cell), qc) for j in own)
            # squared distance from the query to the box of the cell across, as box_dmin2 forms it
            edge = np.where(s > 0, (qc + s) * float(np.float64(cell)) - Qt[i], np.where(s < 0, Qt[i] - (qc + s + 1) * float(np.float64(cell)), 0.0))
            box = float((np.maximum(edge, 0.0) ** 2).sum()) * (1.0 - 1e-5)
            if v == 3:
                assert float(dd[i, 4]) < box and across not in ids[i], "the 5th distance is below the box distance: the cell across may be skipped"
            elif v == 4:
                assert across == ids[i, 4] and 0.97 * float(dd6[i, 5]) < box < float(dd[i, 4]), "the bound after round 0 is 2 % above the box distance"
            else:
                assert float(dd[i, 4]) > box, "the cell across can hold something closer than the 5th"
        d_across = KC.d2_f32(Qt[i:i + 1], c.map[across:across + 1])[0, 0]
        if v == 0:
            assert dd6[i, 4] == dd6[i, 5] == d_across and across in ids6[i, 4:6], "an exact tie for the 5th place with the point across"
            assert (ids[i, 4] == across) == (across < ids6[i, 4:6].max()), "the lower index wins"
        elif v == 1:
            assert across == ids[i, 4] and d_across < dd6[i, 5]
        elif v == 2:
            assert across == ids6[i, 5] and d_across > dd[i, 4]
    assert kinds == {1: 6, 2: 12, 3: 8} and variants == {0, 1, 2, 3, 4}
    wins = [ids[i, 4] == across for i, (s, v, across) in enumerate(c.info["layout"]) if v == 0]
    assert any(wins) and not all(wins), "the tie goes either way"


def test_shell():
    c = KC.shell()
    Qt, ids, dd = KC.model5("shell")
    mc, qc = _cells(c.map, KC.CELL2), _cells(Qt, KC.CELL2)
    for i in range(len(Qt)):
        cheb = np.abs(mc - qc[i]).max(axis=1)
        assert (cheb <= 1).sum() == c.info["inner"][i] < 5, "fewer than 5 points in the inner 27 half cells"
        shell_pts = cheb == 2
        assert shell_pts.sum() >= 40
        assert {tuple(np.abs(o)) for o in (mc[shell_pts] - qc[i])} >= {(2, 2, 2), (2, 0, 0)}, "out to the corners"
    full, rest = KC.gated_classes(dd, KC.GATE)
    assert full.sum() >= 3 and rest.sum() >= 3
    ring = KC.fifth_ring("shell", "g2")
    assert (ring[full] == 2).all(), "every accepted list needs the second stage"
    one = np.float32(1.0)
    d = KC.d2_f32(Qt, c.map)
    assert (d == one).any(axis=1).all() and (dd[full, 4] == one).any(), "a point at exactly the gate, for some queries the 5th neighbour (accepted)"
    assert (dd[rest, 4] == np.float32(1.0 + 2.0 ** -19)).any(), "for others the 5th neighbour is a step outside the gate (rejected)"
    assert ((d == np.nextafter(one, np.float32(0))).sum() + (d == np.float32(1.0 - 2.0 ** -19)).sum()) >= len(Qt), "a point a step inside the gate"
    assert (d == np.float32(1.0 + 2.0 ** -19)).sum() >= len(Qt), "a point a step outside the gate"


@pytest.mark.parametrize("hashed", (False, True))
def test_rings_out(hashed):
    name = "rings_out_hashed" if hashed else "rings_out"
    c = KC.CASES[name]()
    assert c.settings == ("u1",)
    ring = KC.fifth_ring(name, "u1")
    assert ring.tolist() == list(KC.RINGS_OUT)
    assert {2, 3, 4} <= set(ring.tolist()) and (ring > KC.K_MAX_RING).sum() >= 3
    mc = _cells(c.map, KC.CELL1)
    box = int(np.prod((mc.max(axis=0) - mc.min(axis=0) + 1).astype(object)))
    assert (box > KC.K_MAX_WINDOW_CELLS) == hashed
    assert np.array_equal(KC.file_float(c.map, KC.CELL1), KC.file_query(c.map, KC.CELL1))
    own = (np.abs(mc - _cells(c.query[-1], KC.CELL1)).max(axis=1) == 0).sum()
    assert own == 2, "the last query has 2 points in its own cell"


def test_out_of_range():
    c = KC.out_of_range()
    Qt, _, dd = KC.model5("out_of_range")
    assert np.isfinite(Qt).all()
    for cell in (KC.CELL1, KC.CELL2):
        assert KC.out_of_key_range(Qt, cell).all()
        assert (np.abs(KC.file_query(Qt, cell)) >= KC.K_KEY_LIMIT).any(axis=1).all(), "beyond the range knn_grid accepts as well"
    assert (dd[:, 0] > KC.GATE).all()
    Q1, _, d1 = KC.model1("out_of_range")
    assert (d1 > KC.GATE).all()


@pytest.mark.parametrize("setting", ("u1", "g2", "g1"))
def test_boundary_filing(setting):
    c = KC.boundary_filing(setting)
    cell, limit = c.info["cell"], c.info["limit"]
    Qt, ids, dd = KC.model5(f"boundary_filing_{setting}")
    assert np.array_equal(Qt, c.query)
    rows = c.info["rows"]
    assert len(rows) == 8 and c.info["n_pairs"] == (53 if setting == "g1" else 127)
    if setting == "u1":
        assert rows[0][2:] == (-137.01370239257812, -136.01361083984375)
    if setting == "g2":
        assert rows[0][2:] == (-68.50685119628906, -68.00680541992188)
    qc, mc_f, mc_q = _cells(c.query, cell), KC.file_float(c.map, cell).astype(np.int64), _cells(c.map, cell)
    for qi, pi, qx, px in rows:
        assert c.query[qi, 0] == np.float32(qx) and c.map[pi, 0] == np.float32(px)
        assert abs(int(qc[qi, 0]) - int(mc_f[pi, 0])) == 2, "the query's filing and the float filing of the point disagree by two cells"
        assert abs(int(qc[qi, 0]) - int(mc_q[pi, 0])) == 1, "filed with the query's expression the point is a neighbour"
        assert np.array_equal(qc[qi, 1:], mc_q[pi, 1:]) and np.array_equal(qc[qi, 1:], mc_f[pi, 1:])
        d2_pair = KC.d2_f32(c.query[qi:qi + 1], c.map[pi:pi + 1])[0, 0]
        assert float(d2_pair) <= limit
        nfill = 4 if setting == "g1" else 5
        fill = np.arange(pi + 1, pi + 1 + nfill)
        d2_fill = KC.d2_f32(c.query[qi:qi + 1], c.map[fill])[0]
        for filing in (mc_f, mc_q):
            assert (np.abs(filing[fill] - qc[qi]).max(axis=1) <= 1).all(), "the fillers are filed within one cell of the query"
        if setting == "g1":
            assert d2_pair == np.float32(KC.GATE) and (d2_fill < d2_pair).all() and (np.diff(d2_fill) > 0).all()
            assert ids[qi].tolist() == fill.tolist() + [pi], "the point at the gate is the 5th neighbour: the list is accepted only if it is found"
        else:
            assert (d2_fill > d2_pair).all() and (d2_fill.astype(np.float64) < limit).all() and (np.diff(d2_fill) > 0).all()
            assert ids[qi].tolist() == [pi] + fill[:4].tolist(), "the pair's point is the nearest; without it the five fillers certify themselves"
            assert float(d2_fill[4]) <= KC.certify_limit(cell)
        assert dd[qi, 4] <= np.float32(KC.GATE) or setting == "u1"
