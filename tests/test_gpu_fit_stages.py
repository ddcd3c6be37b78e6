"""The stages of the fit launch, each on its own, through the hooks of include/fls_debug_fit.h, which call the __forceinline__ routines themselves
on the LDS structs of the product kernels: plane_residual_dev, line_residual_dev (against the oracle's lambdas, bit for bit), icp_point_rows
(against the numpy model of the oracle's in-line code, bit for bit), the three wave reductions of the rank-1 terms (exact integers bit for bit;
the DPP tree bit for bit against its model; the matrix-core forms within gamma_66 of the exact sum), reduce_partials in its four instantiations
(bit for bit against the add-by-add model), the fan-in ticket (last arriver unique, sees every row, counters back at zero) and the assembled H, g
of one iteration of every kind (within 2 gamma_N sum |terms| of the oracle's).  The cases and what they reach: tests/fit_cases.py,
tests/test_fit_cases.py.  One launch per routine and family set.

Measured on an MI355X (printed by every run): see DESIGN.md, "The stages of the fit launch, routine by routine"."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg, synth
from tests import fit_cases as FC, linalg_cases as LC, util
from tests.test_gpu_linalg import _p, _report

pytestmark = pytest.mark.gpu

UP = C.POINTER(C.c_uint32)


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _residual(fn, cases):
    nn, ps, pt, T, gate, lab = cases
    n = lab.shape[0]
    valid = np.full(n, 7.0); J = np.full((n, 6), 7.0); d = np.full(n, 7.0)
    assert fn(0, _p(_c(nn.reshape(n, 15))), _p(_c(ps)), _p(_c(pt)), _p(_c(T)), _p(_c(gate)), n, _p(valid), _p(J), _p(d)) == 0
    assert np.isin(valid, (0.0, 1.0)).all()
    return valid == 1.0, J, d


def _compare_residual(name, cases, ref, got):
    lab = cases[5]
    (v_ref, J_ref, d_ref), (v, J, d) = ref, got
    _report(name + " valid flag", v == v_ref, lab, lambda s: (cases[4][s], bool(v_ref[s]), bool(v[s])))
    ok = LC.same_bits(J, J_ref, nan_free=True).all(1) & LC.same_bits(d, d_ref, nan_free=True)
    _report(name + " J, distance", ok | ~v_ref, lab, lambda s: (J_ref[s], J[s], d_ref[s], d[s]))
    # where the routine returned early it wrote nothing
    assert (J[~v] == FC.CANARY).all()


def test_plane_residual_bit_exact_against_oracle(built):
    """valid flag equal on every system -- the threshold at the oracle's own max |r| / nrm and one double below it, range within 1e-6 of 81 d^2 on
    both sides, d == 0, d < 0, NaN norm (valid, NaN J) -- and J, d_abs bit for bit where valid."""
    assert _lib.device_count() >= 1
    cases = FC.plane_residual_cases()
    got = _residual(_lib.lib().fls_debug_plane_residual, cases)
    _compare_residual("plane_residual_dev", cases, FC.oracle_plane_residual(), got)
    assert (got[2][~got[0]] == FC.CANARY).all()


def test_line_residual_bit_exact_against_oracle(built):
    """valid flag equal on every system -- the ratio at S0 / S1 of the oracle's singular values and its two neighbours either way, S = 0 -- and J,
    dist bit for bit where valid; dist == 0 gives NaN J on both sides."""
    assert _lib.device_count() >= 1
    cases = FC.line_residual_cases()
    got = _residual(_lib.lib().fls_debug_line_residual, cases)
    _compare_residual("line_residual_dev", cases, FC.oracle_line_residual(), got)


def test_icp_point_rows_bit_exact_against_model(built):
    assert _lib.device_count() >= 1
    T, p, m, lab = FC.icp_point_rows_cases()
    n = lab.shape[0]
    J = np.full((n, 18), 7.0); e = np.full((n, 3), 7.0); res = np.full(n, 7.0)
    assert _lib.lib().fls_debug_icp_point_rows(0, _p(_c(T)), _p(_c(p)), _p(_c(m)), n, _p(J), _p(e), _p(res)) == 0
    Jr, er, rr = FC.icp_point_rows_model(T, p, m)
    ok = LC.same_bits(J, Jr).all(1) & LC.same_bits(e, er).all(1) & LC.same_bits(res, rr)
    _report("icp_point_rows", ok, lab, lambda s: (Jr[s], J[s], er[s], e[s], rr[s], res[s]))


# ---- wave reductions ---------------------------------------------------------------------------------------------------------------------
def _run_rank1(fn, contrib, J, r):
    n = contrib.shape[0]
    rows = np.full((n, 32), -1.0)
    assert fn(0, _p(_c(contrib.astype(np.float64))), _p(_c(J.reshape(n, -1))), _p(_c(r.reshape(n, -1))), n, _p(rows)) == 0
    return rows


def _check_rank1(name, fn, cases, terms, own_cols, dpp_model=None):
    """own_cols: the columns the routine writes; every other column of the row keeps the canary"""
    contrib, J, r, lab, twin = cases
    n = lab.shape[0]
    rows = _run_rank1(fn, contrib, J, r)
    other = [c for c in range(32) if c not in own_cols]
    _report(name + " canary columns", (rows[:, other] == FC.CANARY).all(1), lab, lambda s: (rows[s],))
    # exact integers: any order gives these bits (the sign of an exact zero is the order's own: -h of the matrix-core forms, +0 of the tree)
    ints = np.nonzero(np.char.startswith(lab, "int_"))[0]
    want = np.zeros((n, 29))
    for s in ints:
        x, y = terms(contrib[s], J[s], r[s])
        want[s] = (x * y).sum(0)
    ok = np.ones(n, bool)
    ok[ints] = LC.same_bits(rows[ints][:, own_cols], want[ints][:, own_cols], zero_sign_free=True).all(1)
    _report(name + " exact-integer family", ok, lab, lambda s: (np.nonzero(contrib[s])[0], want[s], rows[s]))
    # poisoned lanes change nothing: the row of the same case with zeros there, bit for bit
    pz = np.nonzero(twin >= 0)[0]
    ok = np.ones(n, bool)
    ok[pz] = LC.same_bits(rows[pz], rows[twin[pz]]).all(1)
    _report(name + " poisoned lanes that do not contribute", ok, lab, lambda s: (rows[twin[s]], rows[s]))
    # determinism: the same case in every wave slot of two workgroups, and in a second launch
    rep = np.nonzero(lab == "repeat")[0]
    assert LC.same_bits(rows[rep], np.tile(rows[rep[0]], (rep.size, 1))).all(), rows[rep]
    again = _run_rank1(fn, contrib, J, r)
    assert LC.same_bits(rows, again, nan_free=True).all(), np.nonzero(~LC.same_bits(rows, again, nan_free=True).all(1))[0]
    fl = np.nonzero(np.isin(lab, ("wide", "cancel", "repeat")))[0]
    if dpp_model is not None:
        ref = dpp_model(contrib[fl], J[fl], r[fl])
        ok = np.ones(n, bool)
        ok[fl] = LC.same_bits(rows[fl][:, :29], ref).all(1)
        _report(name + " against the tree model", ok, lab, lambda s: (rows[s],))
        return
    # matrix cores: |got - exact| <= gamma_66 sum |terms| in any order: at most one rounding of a product (none if fused), at most 64 accumulator
    # additions and the addition that joins the two halves.  The count is an exact integer.
    worst, ok = 0.0, np.ones(n, bool)
    g66 = Fraction(FC.gamma(66))
    for s in fl:
        ex, ab = FC.exact_sums(*terms(contrib[s], J[s], r[s]))
        for c in own_cols:
            err = abs(Fraction(float(rows[s, c])) - ex[c])
            if err > g66 * ab[c]:
                ok[s] = False
            if ab[c] > 0:
                worst = max(worst, float(err / (g66 * ab[c])))
        ok[s] &= rows[s, 28] == float(ex[28])
    print("%s: largest |got - exact| / (gamma_66 sum |terms|) = %.4f over %d cases" % (name, worst, fl.size))
    _report(name + " within gamma_66 of the exact sum", ok, lab, lambda s: (rows[s],))


def test_rank1_mfma(built):
    assert _lib.device_count() >= 1
    _check_rank1("reduce_rank1_mfma_and_store", _lib.lib().fls_debug_rank1_mfma, FC.rank1_cases(), FC.rank1_terms, list(range(29)))


def test_rank1_dpp(built):
    assert _lib.device_count() >= 1
    _check_rank1("reduce_rank1_and_store", _lib.lib().fls_debug_rank1_dpp, FC.rank1_cases(), FC.rank1_terms, list(range(29)), dpp_model=FC.rank1_dpp_model)


def test_rank1x3_mfma(built):
    """column 27 (sum |e|, a DPP sum of the caller) keeps its canary"""
    assert _lib.device_count() >= 1
    _check_rank1("reduce_rank1x3_mfma_and_store", _lib.lib().fls_debug_rank1x3_mfma, FC.rank1x3_cases(), FC.rank1x3_terms, list(range(27)) + [28])


# ---- row reduction and fan-in ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", range(4))
def test_reduce_partials_bit_exact_against_model(built, variant):
    """<256, true, 32> (three straight-line trip variants, switching at 224 / 225 and 256 / 257 rows), <512, true, 16>, <512, true, 32>,
    <1024, false, 16>: all 32 columns bit for bit against the add-by-add model, on rows whose sum depends on the order and on exact integers."""
    assert _lib.device_count() >= 1
    NT, U = FC.REDUCE_VARIANTS[variant]
    wide, ints = FC.partial_rows()
    bad = []
    for name, rows in (("wide", wide), ("ints", ints)):
        for nrows in FC.reduce_row_counts(variant):
            tot = np.full(32, 7.0)
            assert _lib.lib().fls_debug_reduce_partials(0, variant, _p(_c(rows[:nrows])), nrows, _p(tot)) == 0
            ref = FC.reduce_partials_model(rows, nrows, NT, U)
            if not LC.same_bits(tot, ref).all():
                bad.append((name, nrows, np.nonzero(~LC.same_bits(tot, ref))[0].tolist()))
    assert not bad, "reduce_partials<%d, %d>: (rows, nrows, columns that differ) %s" % (NT, U, bad[:8])


@pytest.mark.parametrize("shards", [1, 8])
def test_fanin_last_arriver_is_unique_sees_every_row_and_resets(built, shards):
    """two launches on the same ticket words without a reset in between, with different rows: exactly one workgroup is told it is the last, both
    times; its totals are the exact sums of ALL rows of ITS launch; every ticket word is zero afterwards."""
    assert _lib.device_count() >= 1
    for nb in FC.FANIN_BLOCKS:
        tot = np.full((2, 32), -1.0); last = np.full(2, 99, np.uint32); ticket = np.full(_lib.DEBUG_TICKET_WORDS, 99, np.uint32)
        assert _lib.lib().fls_debug_fanin(0, nb, shards, _p(tot), last.ctypes.data_as(UP), ticket.ctypes.data_as(UP)) == 0
        assert last.tolist() == [1, 1], (nb, shards, last)
        assert np.array_equal(tot, FC.fanin_totals(nb)), (nb, shards, tot, FC.fanin_totals(nb))
        assert not ticket.any(), (nb, shards, np.nonzero(ticket)[0])


# ---- the assembled system ------------------------------------------------------------------------------------------------------------------
def _scene(mode):
    if mode == "PointToPlane_IVOX":
        cfg = synth.make_config(1, scale=0.05); return reg.YAML_NCLT_IVOX, [cfg["map"]], cfg["scan"], None, False
    if mode == "IcpOptimized":
        cfg = synth.make_config(0); return reg.YAML_NCLT_ICP, [cfg["map"]], cfg["scan"], None, True
    if mode == "IncrementalNDT":
        cfg = synth.make_config(2, scale=0.1); return reg.YAML_NCLT_NDT, [cfg["map"]], cfg["scan"], None, False
    if mode == "LoamFull_KdTree":
        cfg = synth.make_config(3, scale=0.1); return reg.YAML_NCLT_LOAM_FULL, [cfg["map"], cfg["corner_map"]], cfg["scan"], cfg["corner_scan"], False
    cfg = synth.make_config(1, scale=0.1); return reg.YAML_NCLT_LOC_KDTREE, [cfg["map"]], cfg["scan"], None, True


@pytest.mark.parametrize("mode", ["PointToPlane_IVOX", "IcpOptimized", "IncrementalNDT", "LoamFull_KdTree", "PointToPlane_KdTree"])
def test_last_system_against_oracle(built, mode):
    """GnState::H, g after ONE iteration against the oracle's last_H, last_g (all five tails store them: loam_tail and lu_tail).  Per entry
    |delta| <= 2 gamma_N A: A the oracle's sum of the absolute values of the finest-grain terms, N the number of those terms plus the partial rows the
    tail summed -- the row count is a launch detail the handle does not report; a workgroup holds at least 32 points, so ceil(points / 32) + 8 (one
    row per shard of slack) bounds it from above -- and both sides are within gamma_N A of the exact sum.  H is symmetric to the bit."""
    assert _lib.device_count() >= 1
    y, maps, scan, corner, loc = _scene(mode)
    y = dict(y, optimization_iter_num=1)
    m = reg.make_matcher(mode, y, is_localization_mode=loc)
    o = util.oracle_for(mode, y, loc)
    m.AddCloudToLocalMap(maps)
    o.AddCloudToLocalMap(*maps)
    T = np.eye(4)
    m.Match(util.cluster_for(mode, scan, corner), T, update_map=False)
    o.Match(scan, np.eye(4), src1=corner, update_map=False)
    assert m.stats.iterations == o.stats.iterations == 1
    assert m.stats.n_valid == o.stats.n_valid and m.stats.n_valid_corner == o.stats.n_valid_corner and o.stats.n_valid > 100
    H = np.full(36, 7.0); g = np.full(6, 7.0)
    assert _lib.lib().fls_debug_last_system(m._h, _p(H), _p(g)) == 0
    H = H.reshape(6, 6, order="F")
    Ho, go = o.last_system()
    Ha, ga, terms = o.last_abs_system()
    assert terms >= o.stats.n_valid and (np.abs(Ho) <= Ha * (1 + 1e-12)).all() and (np.abs(go) <= ga * (1 + 1e-12)).all()
    assert LC.same_bits(H, H.T).all(), H - H.T
    n_points = scan.shape[0] + (corner.shape[0] if corner is not None else 0)
    N = terms + (n_points + 31) // 32 + 8
    bound_H, bound_g = 2 * FC.gamma(N) * Ha, 2 * FC.gamma(N) * ga
    with np.errstate(divide="ignore", invalid="ignore"):
        rH = np.where(bound_H > 0, np.abs(H - Ho) / bound_H, np.where(H == Ho, 0.0, np.inf))
        rg = np.where(bound_g > 0, np.abs(g - go) / bound_g, np.where(g == go, 0.0, np.inf))
    print("%s: n_valid %d, terms %d, N %d; largest |H - H_oracle| / (2 gamma_N A) = %.3e, g: %.3e" % (mode, o.stats.n_valid, terms, N, rH.max(), rg.max()))
    assert rH.max() <= 1.0 and rg.max() <= 1.0, (rH, rg)
    m.close()
    o.close()
