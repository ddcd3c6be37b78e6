"""tests/ivox_decide_cases.py without a GPU: every case reaches the edge of LoamPointToPlaneIVOX::AddCloudToLocalMap's rule it is named after,
asserted from the oracle's own decision (oracle.ivox_add_decide, the function the oracle's AddCloud calls) and from doubles: the equalities are
exact, the brackets straddle dist + 1e-6 on adjacent floats, every code and every branch occurs, each named wrong edge (rule_model's mutants)
would change an answer, the flipper rows the list forms hide would change the decision if read.  And the host form of the rule,
fls_debug_ivox_decide_host (ivox_decide_host, what fls_add_cloud_to_local_map runs for a later cloud that is not the resident scan), equals the
oracle on every launch's inputs: codes exactly, world points bit for bit (NaN for NaN: x86 and the device give NaNs of different sign)."""
import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg
from oracle import oracle as O
from tests import ivox_decide_cases as D


def same_points(got, want):
    """bit for bit, NaN where the oracle has NaN"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


@pytest.fixture(scope="module")
def decided(built):
    """the oracle's (code, pw) per case, computed once"""
    return {name: O.ivox_add_decide(c.src, c.T, c.fs, c.nn, c.cnt) for name, c in D.cases().items()}


def test_the_model_is_the_oracle_and_the_claims_hold(decided):
    for name, c in D.cases().items():
        code, pw = decided[name]
        mcode, mpw = D.rule_model(c.src, c.T, c.fs, c.nn, c.cnt)
        assert np.array_equal(code, mcode) and same_points(mpw, pw), name
        assert set(np.unique(code)) <= {0, 1, 2}
        for i, e in enumerate(c.expect):
            assert e is None or (code[i] != 2 if e == "not2" else code[i] == e), (name, i, c.kind[i], e, int(code[i]))


def test_every_code_and_branch_occurs(decided):
    C = D.cases()
    for name in ("general_pose", "fs_0p3", "origin", "negative_coordinates") + tuple("n%d" % n for n in D.SIZES if n >= 63):
        assert set(np.unique(decided[name][0])) == {0, 1, 2}, name
    for name in ("general_pose", "fs_0p3", "origin", "n1000"):
        code, cnt = decided[name][0], C[name].cnt
        assert set(np.unique(cnt)) == set(range(8)), name
        assert {(int(a), int(b)) for a, b in zip(np.minimum(cnt, 5), code)} == {(0, 1)} | {(k, v) for k in (1, 2, 3, 4) for v in (1, 2)} | {(5, v) for v in (0, 1, 2)}, name
    low = C["low_counts_all_nearer"]
    again, _ = O.ivox_add_decide(low.src, low.T, low.fs, low.nn, np.full(len(low.cnt), 5, np.uint8))
    assert (again == 0).all()  # the same lists decide 0 once the count says 5: only the count kept the loop out
    c0 = C["count0_garbage_rows"]
    assert (O.ivox_add_decide(c0.src[1:3], c0.T, c0.fs, c0.nn[1:3], [5, 5])[0] == [0, 2]).all()
    kinds = C["distance_loop"].kind
    assert {"only_%d_nearer" % k for k in range(5)} | {"none_nearer", "same_dist"} <= set(kinds)


def test_equalities_are_exact_and_brackets_straddle(decided):
    n_face = n_same = n_lo = 0
    for name, c in D.cases().items():
        pw = decided[name][1].astype(np.float64)
        ctr = D.centre(decided[name][1], c.fs)
        nn = c.nn.astype(np.float64)
        with np.errstate(invalid="ignore"):
            dist = D.sq(pw - ctr)
            f2 = D.sq(nn - ctr[:, None, :])
        for i, kind in enumerate(c.kind):
            d0 = np.abs(nn[i, 0] - ctr[i])
            if kind == "face_eq":
                a = c.axis[i]
                assert d0[a] == 0.5 * c.fs and all(d0[b] > 0.5 * c.fs for b in range(3) if b != a) or (c.cnt[i] == 3 and (d0 == 0.5 * c.fs).all()), (name, i)
                n_face += 1
            elif kind == "beyond_all":
                step = np.abs(np.float32(c.nn[i, 0]) - np.nextafter(c.nn[i, 0], np.float32(ctr[i]).astype(np.float32)))  # one float back towards the centre ...
                assert (d0 > 0.5 * c.fs).all() and (d0 - step.astype(np.float64) <= 0.5 * c.fs).all(), (name, i)   # ... is on the face or inside
            elif kind == "beyond_two":
                a = c.axis[i]
                assert d0[a] < 0.5 * c.fs and all(d0[b] > 0.5 * c.fs for b in range(3) if b != a), (name, i)
            elif kind == "same_dist":
                assert (f2[i] == dist[i]).any() and not (f2[i] < dist[i]).any(), (name, i)
                n_same += 1
            elif kind == "bracket_lo":
                a, k = c.axis[i], int(np.argmin(f2[i]))
                hi = c.nn[i + 1, k]
                assert c.kind[i + 1] == "bracket_hi" and np.array_equal(np.delete(hi, a), np.delete(c.nn[i, k], a))
                assert abs(int(hi[a:a + 1].view(np.int32)[0]) - int(c.nn[i, k, a:a + 1].view(np.int32)[0])) == 1  # adjacent floats
                assert dist[i] <= f2[i, k] < dist[i] + 1.0e-6 <= f2[i + 1, k] and np.delete(f2[i], k).min() > dist[i] + 1.0e-6, (name, i)
                assert decided[name][0][i] == 0 and decided[name][0][i + 1] == 1
                n_lo += 1
    assert n_face >= 50 and n_same >= 50 and n_lo == 18


def test_every_wrong_edge_changes_an_answer(decided):
    """each mutant of the rule differs from the oracle on the case named for it: in a code, or for the float pose product in a world point"""
    seen = set()
    for name, c in D.cases().items():
        code, pw = decided[name]
        for m in c.mutants:
            mcode, mpw = D.rule_model(c.src, c.T, c.fs, c.nn, c.cnt, mutant=m)
            diff = int((mpw.view(np.uint32) != pw.view(np.uint32)).any(axis=1).sum()) if m == "float_pw" else int((mcode != code).sum())
            assert diff >= 1, (name, m)
            seen.add(m)
    assert seen == set(D.MUTANTS)


def test_the_other_form_of_every_list_would_flip_the_decision(built):
    """rows form and ids form are mixed inside every wave, and what a list keeps in the form it is NOT in -- and what words 5 to 7 of its ids row
    name -- is a neighbour that changes the decision when it stands first"""
    C = D.cases()
    for name, l in D.launches().items():
        if l.ids is None:
            continue
        c, nn_n, n_slots = C[l.case], len(l.cnt), len(l.map_rows)
        m = min(len(l.src), nn_n)
        ids_form = (l.cnt & D.ROWS_BIT) == 0
        if "mixed" in name and nn_n >= 64:
            for w in range(0, nn_n - 63, 64):
                assert 0 < ids_form[w:w + 64].sum() < 64, name
        assert (l.ids[:, 5:] < n_slots).all(), name
        code, pw = O.ivox_add_decide(c.src[:m], c.T, c.fs, c.nn[:m], c.cnt[:m])
        hidden = np.where(ids_form[:m, None], np.ascontiguousarray(l.rows[:m, 0, :3]), l.map_rows[l.ids[:m, 0] % n_slots][:, :3])
        for words in (hidden, l.map_rows[l.ids[:m, 5]][:, :3], l.map_rows[l.ids[:m, 6]][:, :3], l.map_rows[l.ids[:m, 7]][:, :3]):
            nn = c.nn[:m].copy()
            nn[:, 0] = np.ascontiguousarray(words).view(np.float32)
            flipped, _ = O.ivox_add_decide(c.src[:m], c.T, c.fs, nn, c.cnt[:m])
            judge = (c.cnt[:m] > 0) & np.isfinite(pw).all(axis=1) & (ids_form[:m] | (l.ids[:m, 0] < n_slots))
            assert (flipped[judge] != code[judge]).all(), name


def test_stale_ids_are_where_they_are_claimed(built):
    """ids in [n_slots, n_slots + MAP_PAD) only in ids-form lists of materializing launches; they resolve to (0, 0, 0, id -1), never to the sentinel"""
    L = D.launches()
    for name, l in L.items():
        if l.ids is None:
            assert l.stale == 0
            continue
        n_slots = len(l.map_rows)
        stale = l.ids[:, :5] >= n_slots
        assert (l.ids[:, :5] < n_slots + D.MAP_PAD).all() and (l.stale > 0 or not stale.any()) and (l.materialize or not stale.any()), name
        assert stale.any() or l.stale == 0 or len(l.cnt) < 60, name
        assert not stale[(l.cnt & D.ROWS_BIT) != 0].any(), name
        if stale.any():
            gathered, rows, cnt = D.materialized(l)
            assert (gathered[stale] == D.STALE_ROW).all() and not (rows == D.SENTINEL.view(np.uint32)).all(axis=2).any(), name
    st = L["origin/all_stale/m1"]
    assert (st.ids[:, :5] >= len(st.map_rows)).any(axis=1).all()
    # a stale neighbour decides: the oracle's codes on the resolved rows differ from its codes on the rows the lists were built from
    c = D.cases()["origin"]
    nn, cnt = D.rule_inputs(st)
    assert (O.ivox_add_decide(c.src, c.T, c.fs, nn, cnt)[0] != O.ivox_add_decide(c.src, c.T, c.fs, c.nn, c.cnt)[0]).sum() >= 10


def test_gate_cases_cover_both_sides():
    runs = {name.split("/")[1]: D.gate_runs(l.gate) for name, l in D.launches().items() if l.gate is not None}
    assert runs == {"not_done": False, "done_49": False, "done_50": True, "max_iter_50": True, "max_iter_49": False, "past_max_iter": True}
    for l in D.launches().values():
        if l.gate is not None:
            assert not np.array_equal(l.T, l.gate["T"]) and l.count == 1


def test_host_rule_equals_the_oracle_on_every_launch(built):
    """fls_debug_ivox_decide_host on what the rule sees of every launch (resolved rows, plain counts; a point without a list has count 0)"""
    for name, l in D.launches().items():
        nn, cnt = D.rule_inputs(l)
        T = l.T if l.gate is None else l.gate["T"]
        want_code, want_pw = O.ivox_add_decide(l.src, T, l.fs, nn, cnt)
        rc, code, pw = reg.DebugIvoxDecideHost(l.src, T, l.fs, nn, cnt)
        assert rc == _lib.FLS_OK and np.array_equal(code, want_code) and same_points(pw, want_pw), name
    for name, c in D.cases().items():
        want_code, want_pw = O.ivox_add_decide(c.src, c.T, c.fs, c.nn, c.cnt)
        rc, code, pw = reg.DebugIvoxDecideHost(c.src, c.T, c.fs, c.nn, c.cnt)
        assert rc == _lib.FLS_OK and np.array_equal(code, want_code) and same_points(pw, want_pw), name


def test_nonfinite_points_are_what_they_claim(decided):
    for name in ("nonfinite_identity", "nonfinite_general_pose"):
        code, pw = decided[name]
        bad = ~np.isfinite(D.cases()[name].src).all(axis=1)
        assert bad.sum() == 54 and np.isnan(pw[bad]).any(axis=1).any() and not np.isfinite(pw[bad]).all(axis=1).any()
    assert np.isinf(decided["nonfinite_general_pose"][1]).any() and (decided["nonfinite_general_pose"][0] == 2).any()
