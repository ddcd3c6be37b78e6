"""What the cases of tests/tail_cases.py reach, shown by the model alone (no GPU): the rows sum exactly in any order, every family takes the branch
it is named after, and each family has at least the cases FAMILY_MIN states.  tests/test_gpu_tails.py runs the same cases on the device and
asserts that it ran these counts."""
from fractions import Fraction

import numpy as np

from oracle import oracle as O
from tests import tail_cases as TC


def _by_family(fam):
    return [c for c in TC.cases() if c.family == fam]


def _model(c, **kw):
    st_in, mb_in, rt, pt, st, mb, info = TC.run_model(c, **kw)
    return st_in, mb_in, rt, pt, st, mb, info


def test_layouts_and_words(built):
    assert TC.ST.itemsize == 9656 and TC.MB.itemsize == 216
    assert TC.ST.fields["log_T"][1] == 696 and TC.ST.fields["log_res"][1] == 696 + 64 * 128 and TC.ST.fields["log_nv"][1] == 696 + 64 * 136
    assert TC.MB.fields["seq"][1] == 212
    assert TC.launch_word(TC.ID_MASK, True, 300) == 0xFFFFFFFF and TC.launch_word(1, False, 0) == 1
    assert TC.seq_word(TC.ID_MASK, 1, 255) == 0xFFFFFFFF and TC.seq_word(1, 0, 6) == (1 << 9) | 6


def test_family_counts(built):
    n = TC.family_counts()
    assert set(n) == set(TC.FAMILY_MIN)
    for f, least in TC.FAMILY_MIN.items():
        assert n[f] >= least, (f, n[f], least)
    print("tail cases by family:", n)


def test_rows_sum_exactly_in_any_order(built):
    """every entry on the 2^-12 grid and at most 2^20, columns 29..31 NaN, and the exact rational sum of every column equals the float sum taken
    forwards, backwards and pairwise"""
    checked = 0
    for c in TC.cases():
        for rows in (c.rows_a, c.rows_b):
            if rows is None:
                continue
            assert 1 <= rows.shape[0] <= 2048 and rows.shape[1] == 32
            assert np.isnan(rows[:, 29:]).all() and np.isfinite(rows[:, :29]).all()
            assert np.array_equal(rows[:, :29], TC.dyadic(rows[:, :29])) and np.abs(rows[:, :29]).max() <= 2.0 ** 20
            if rows.shape[0] in (1, 2, 33, 457, 2048) or c.family != "plain_continue":
                exact = TC.exact_totals(rows)
                fwd, rev = np.zeros(29), np.zeros(29)
                for r in range(rows.shape[0]):
                    fwd += rows[r, :29]
                    rev += rows[rows.shape[0] - 1 - r, :29]
                pair = TC.totals(rows)
                for k in range(29):
                    assert Fraction(float(fwd[k])) == exact[k] and Fraction(float(rev[k])) == exact[k] and Fraction(float(pair[k])) == exact[k], (c.label, k)
                checked += 1
    assert checked >= 100
    # negative pieces are in every set of more than a handful of rows
    assert all((c.rows_b[:, :29] < 0).any() for c in TC.cases() if c.rows_b.shape[0] >= 15)


def test_row_counts_and_distinct_targets(built):
    plain = _by_family("plain_continue")
    for tail, mode in (("loam", 0), ("lu", 0), ("lu", 1)):
        mine = [c for c in plain if c.tail == tail and c.mode == mode]
        assert sorted(set(c.rows_b.shape[0] for c in mine)) == sorted(TC.ROW_COUNTS), (tail, mode)
    loam = [c for c in plain if c.tail == "loam"]
    assert sorted(c.rows_b.shape[0] for c in loam if c.rows_a is None) == sorted(TC.ROW_COUNTS)
    assert sorted(c.rows_b.shape[0] for c in loam if c.rows_a is not None) == sorted(TC.ROW_COUNTS)
    assert sorted(set(c.rows_a.shape[0] for c in loam if c.rows_a is not None)) == sorted(TC.ROW_COUNTS)
    assert any(c.mailbox for c in plain) and any(not c.mailbox for c in plain)
    for c in TC.cases():
        if c.family in ("icp_singular", "zero_step", "loam_rank_deficient"):
            continue
        H, g, ta, tb = TC.system_of(c)
        tri = [H[a, b] for a in range(6) for b in range(a, 6)]
        assert len(set(tri)) == 21, c.label
        assert len(set(tri + g.tolist())) == 27 or c.family == "icp_indefinite", c.label
        if c.rows_a is not None:   # corner and planar statistics differ, and so does every column total of the two sets
            assert ta[27] != tb[27] and ta[28] != tb[28] and not (ta == tb).any(), c.label
            assert int(ta[28]) == ta[28] and int(tb[28]) == tb[28]


def test_expectations_of_every_case(built):
    for c in TC.cases():
        info = _model(c)[6]
        for k, v in c.expect.items():
            if k != "zero":
                assert info.get(k) == v, (c.label, k, v, info.get(k))


def test_plain_and_rule1(built):
    for c in _by_family("plain_continue"):
        _, _, rt, pt, st, mb, info = _model(c)
        rn, pn = TC.step_norms(c, info["dx"])
        assert info["kind"] == "step" and rn > 1e-2 and pn > 1e-2 and st[0]["done"] == 0 and st[0]["iter"] == 1
        assert np.linalg.cond(info["H"]) < 200 and np.linalg.eigvalsh(info["H"]).min() > 0
    for c in _by_family("stop_rule1"):
        st = _model(c)[4]
        assert st[0]["done"] == 1
        if c.tail == "lu":
            assert st[0]["converged"] == 1
        else:
            assert st[0]["converged"] == TC.canary_state()[0]["converged"]   # loam_tail has no such word to write
    for c in _by_family("rule1_one_side"):
        assert _model(c)[4][0]["done"] == 0


def test_loam_rule2_edges(built):
    gap, inside = 1.0e-4, float(np.nextafter(1.0e-4, 0.0))
    seen = set()
    for c in _by_family("loam_rule2"):
        st_in, _, rt, pt, st, _, info = _model(c)
        rn, pn = TC.step_norms(c, info["dx"])
        assert not (rn < rt and pn < pt) and rn > rt and pn > pt, c.label          # rule 1 is off: the norms are above the thresholds
        drot, dpos = abs(rn - float(st_in[0]["last_rot"])), abs(pn - float(st_in[0]["last_pos"]))
        assert int(st[0]["done"]) == int(drot < gap and dpos < gap) == c.expect["stop"], c.label
        seen.add((drot == gap, drot == inside, dpos == gap, dpos == inside))
        assert st[0]["last_rot"] == rn and st[0]["last_pos"] == pn and st[0]["iter"] == 4
    assert {(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True), (True, False, True, False),
            (False, True, False, True)} <= seen


def test_first_ignores_the_incoming_state(built):
    for c in _by_family("first_poisoned"):
        st_in, _, rt, pt, st, mb, info = _model(c)
        assert st_in[0]["done"] == 1 and st_in[0]["iter"] in (37, 61) and not np.array_equal(st_in[0]["T"], c.T0)
        clean = TC.canary_state()
        clean[0]["done"], clean[0]["iter"], clean[0]["T"], clean[0]["last_rot"], clean[0]["last_pos"] = 0, 0, c.T0, 0.0, 0.0
        st2, mb2, _ = TC.model_launch(c, clean, TC.canary_mailbox(), 0, c.word(True), rt, pt)
        for name in ("T", "iter", "done", "last_dx", "H", "g", "log_T", "log_res", "log_nv", "n_valid", "sum_res"):
            assert np.asarray(st[0][name]).tobytes() == np.asarray(st2[0][name]).tobytes(), (c.label, name)
        assert mb.tobytes() == mb2.tobytes() and st[0]["iter"] == 1 and st[0]["done"] == 0
        if c.tail == "loam":   # with the poisoned carried norms rule 2 would have fired
            rn, pn = TC.step_norms(c, info["dx"])
            assert abs(rn - float(st_in[0]["last_rot"])) < 1e-4 and abs(pn - float(st_in[0]["last_pos"])) < 1e-4 and rn >= 1e-4


def test_thresholds_at_the_norm(built):
    nxt = lambda v: float(np.nextafter(v, np.inf))
    for c in _by_family("thr_at_norm"):
        _, _, rt, pt, st, _, info = _model(c)
        rn, pn = TC.step_norms(c, info["dx"])
        at = (rt == rn and pt == TC.SLACK) or (pt == pn and rt == TC.SLACK)
        above = (rt == nxt(rn) and pt == TC.SLACK) or (pt == nxt(pn) and rt == TC.SLACK)
        assert at != above and int(st[0]["done"]) == int(above), c.label
        if c.tail == "lu":
            assert int(st[0]["converged"]) == int(above)
        else:
            assert rn >= 1e-4 and pn >= 1e-4   # first = 1: the carried norms are 0, rule 2 stays off
    assert sum(1 for c in _by_family("thr_at_norm") if c.expect["stop"]) == 6


def test_icp_singular_and_indefinite(built):
    for c in _by_family("icp_singular"):
        H = TC.system_of(c)[0]
        assert O.lu_inverse_6(H)[1] == 0.0, c.label
        st_in, _, _, _, st, mb, info = _model(c)
        s = st[0]
        assert info["kind"] == "skip" and s["done"] == 0 and s["converged"] == 0 and s["iter"] == 5
        assert np.array_equal(s["T"], st_in[0]["T"]) and s["last_dx"].tobytes() == st_in[0]["last_dx"].tobytes()
        assert np.array_equal(s["log_T"][64:80], st_in[0]["T"]) and s["log_nv"][4] == s["n_valid"]
        assert mb[0]["seq"] == TC.seq_word(c.match_id, 0, 5)
        if info["payload"]:
            assert not mb[0]["last_dx"].any() and np.array_equal(mb[0]["T"], s["T"])
    assert sorted(_model(c)[6]["payload"] for c in _by_family("icp_singular")) == [False, False, True, True]
    dets = []
    for c in _by_family("icp_indefinite"):
        H = TC.system_of(c)[0]
        w = np.linalg.eigvalsh(H)
        det = O.lu_inverse_6(H)[1]
        dets.append(det)
        assert (w < 0).any() and (w > 0).any() and det != 0.0 and np.linalg.cond(H) < 1e3, c.label
        st_in, _, _, _, st, _, info = _model(c)
        assert info["kind"] == "step" and np.isfinite(info["dx"]).all() and not np.array_equal(st[0]["T"], c.T0)
    assert sum(d < 0 for d in dets) >= 2 and sum(d > 0 for d in dets) >= 1


def test_min_effective(built):
    got = {}
    for c in _by_family("min_effective"):
        st_in, _, _, _, st, mb, info = _model(c)
        eff = int(TC.totals(c.rows_b)[28])
        got[(c.mode, eff - c.min_eff)] = info["kind"]
        if info["kind"] == "early":
            s = st[0]
            assert s["done"] == 1 and s["converged"] == 0 and np.array_equal(s["T"], st_in[0]["T"]) and s["iter"] == 3 and s["n_valid"] == eff
            assert s["last_dx"].tobytes() == st_in[0]["last_dx"].tobytes() and mb[0]["done"] == 1 and not mb[0]["last_dx"].any()
    assert got == {(1, -1): "early", (1, 0): "step", (1, 1): "step", (0, -1): "step", (0, 0): "step", (0, 1): "step"}


def test_done_on_entry_writes_nothing(built):
    for c in _by_family("done_on_entry"):
        st_in, mb_in, _, _, st, mb, info = _model(c)
        assert info["kind"] == "done" and st.tobytes() == st_in.tobytes() and mb.tobytes() == mb_in.tobytes() == TC.canary_mailbox().tobytes()


def test_log_guard(built):
    can = TC.canary_state()[0]
    for c in _by_family("iter_on_entry"):
        st_in, _, _, _, st, _, info = _model(c)
        it = c.expect["it"]
        s = st[0]
        assert s["iter"] == it + 1 and s["done"] == 0
        if it < 64:
            assert np.array_equal(s["log_T"][16 * it:16 * it + 16], s["T"]) and s["log_nv"][it] == s["n_valid"] and s["log_res"][it] == s["sum_res"]
            keep = np.ones(64, bool); keep[it] = False
            assert s["log_res"][keep].tobytes() == can["log_res"][keep].tobytes()
        else:
            for name in ("log_T", "log_res", "log_nv"):
                assert s[name].tobytes() == can[name].tobytes(), (c.label, name)
    assert sorted(set(c.expect["it"] for c in _by_family("iter_on_entry"))) == [62, 63, 64, 200]


def test_mailbox_rule(built):
    can = TC.canary_mailbox()[0]
    combos = set()
    for c in _by_family("mailbox"):
        for exact in (False, True):
            st_in, _, _, _, st, mb, info = _model(c, exact=exact)
            m, s = mb[0], st[0]
            it1 = int(s["iter"])
            max_it = c.max_it
            want = bool(s["done"]) or max_it == 0 or it1 >= max_it
            assert info["payload"] == want == c.expect["payload"], c.label
            assert m["seq"] == TC.seq_word(c.match_id, int(s["done"]), it1)
            for name in TC.MB.names:
                if name == "seq":
                    continue
                if want:
                    assert np.asarray(m[name]).tobytes() != np.asarray(can[name]).tobytes(), (c.label, name)
                else:
                    assert np.asarray(m[name]).tobytes() == np.asarray(can[name]).tobytes(), (c.label, name)
            if want:
                assert np.array_equal(m["T"], s["T"]) and np.array_equal(m["last_dx"], s["last_dx"]) and m["iter"] == it1 and m["n_valid"] == s["n_valid"]
                assert m["sum_res"] == s["sum_res"] and m["done"] == s["done"]
                if c.tail == "loam":
                    assert m["n_valid2"] == s["n_valid2"] != s["n_valid"] and m["sum_res2"] == s["sum_res2"] != s["sum_res"] and m["converged"] == 0
                else:
                    assert m["n_valid2"] == 0 and m["sum_res2"] == 0.0 and m["converged"] == s["converged"]
            combos.add((c.tail, max_it, c.match_id))
    for tail in ("loam", "lu"):
        for max_it in (0, 9, 6):
            for mid in (0, 1, TC.ID_MASK):
                assert (tail, max_it, mid) in combos
    assert any(not c.mailbox for c in TC.cases())


def test_rank_deficient_and_zero_step(built):
    for c in _by_family("loam_rank_deficient"):
        H, g, _, _ = TC.system_of(c)
        assert np.linalg.matrix_rank(H) == 3 and np.array_equal(H, np.round(H))
        info = _model(c)[6]
        assert np.isfinite(info["dx"]).all() and np.abs(H @ info["dx"] - g).max() <= 1e-9 * np.abs(g).max() and info["dx"].any()
    for c in _by_family("zero_step"):
        _, _, _, _, st, _, info = _model(c)
        assert not info["dx"].any() and np.array_equal(st[0]["T"], c.T0) and st[0]["done"] == 1 and st[0]["T"].tobytes() == np.asarray(c.T0).tobytes()


def test_chain_continues(built):
    for c in _by_family("chain"):
        assert c.launches == 2
        _, _, rt, pt, st1, mb1, i1 = _model(c)
        _, _, _, _, st2, mb2, i2 = _model(c, state=st1, first=0)
        a, b = st1[0], st2[0]
        assert a["iter"] == 1 and b["iter"] == 2 and a["done"] == 0 and not i1["payload"] and i2["payload"]
        assert np.array_equal(b["log_T"][:16], a["T"]) and np.array_equal(b["log_T"][16:32], b["T"]) and not np.array_equal(a["T"], b["T"])
        assert b["log_res"][0] == a["sum_res"] and b["log_nv"][1] == b["n_valid"]
        if c.tail == "loam":   # the same rows give the same step: the carried norms equal the new ones, rule 2 stops the second launch
            assert b["done"] == 1 and b["last_rot"] == a["last_rot"]
            zero = a.copy(); zero["last_rot"] = 0.0; zero["last_pos"] = 0.0
            st3 = TC.model_launch(c, np.array([zero]), None, 0, c.word(True), rt, pt)[0]
            assert st3[0]["done"] == 0
        else:
            assert b["done"] == 0
