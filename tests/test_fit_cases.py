"""The cases of tests/fit_cases.py do what they say, by the oracle and the numpy models alone (no GPU): every family reaches the gate or the branch
it is named after, at least 100 systems sit on each side of each gate, at least 20 are valid with NaN Jacobians, the integer family is exact in
every order, the fixed-order models ARE order dependent on the wide rows, and the models are sums.  Without this file
tests/test_gpu_fit_stages.py could pass by having nothing to compare."""
from fractions import Fraction

import numpy as np

from tests import fit_cases as FC, linalg_cases as LC


def _fam(lab, f):
    return lab == f


def test_plane_residual_families_reach_their_gates():
    nn, ps, pt, T, gate, lab = FC.plane_residual_cases()
    valid, J, d = FC.oracle_plane_residual()
    n = lab.shape[0]
    assert 1000 <= n <= 1600
    print("plane residual:", {f: (int((lab == f).sum()), int(valid[lab == f].sum())) for f in dict.fromkeys(lab)})
    # the threshold gate, exactly: max |r| / nrm is not above itself; the next double towards zero is below it
    assert valid[_fam(lab, "thres_at_gate")].all() and int(_fam(lab, "thres_at_gate").sum()) >= 100
    assert not valid[_fam(lab, "thres_below_gate")].any() and int(_fam(lab, "thres_below_gate").sum()) >= 100
    # range against 81 d^2, within 1e-6 relative: the oracle decided, both sides are there
    rg = _fam(lab, "range_gate")
    assert int(valid[rg].sum()) >= 100 and int((~valid[rg]).sum()) >= 100
    rng_ = np.sqrt((ps[rg] ** 2).sum(1))
    big = FC.oracle_plane_residual_far_source()
    assert (np.abs(rng_ / (81.0 * big ** 2) - 1.0) <= 1.2e-6).all()
    # the workload's own gate on noisy planes: both outcomes
    for f in ("noisy_plane", "far_mm"):
        assert int(valid[_fam(lab, f)].sum()) >= 15 and int((~valid[_fam(lab, f)]).sum()) >= 15, f
    # d == 0: s = -1 (d > 0 is false), d_abs = +0, J[3:6] = -n with n the normalised fit
    for f, sgn in (("d_zero", -1.0), ("d_negative", -1.0), ("d_positive", 1.0)):
        idx = np.nonzero(_fam(lab, f))[0]
        assert idx.size >= 60 and valid[idx].all()
        for s in idx:
            nrm_n, _ = FC._plane_normal_and_gate(nn[s])
            assert LC.same_bits(J[s, 3:6], nrm_n * sgn).all(), (f, s)
        assert (d[idx] == 0.0).all() if f == "d_zero" else (d[idx] > 0.05).all()
    # NaN norm: valid, every J entry NaN (pinned: the reference lambda does not reject it either, each of its comparisons with a NaN is false)
    z = _fam(lab, "zeros")
    assert int(z.sum()) >= 20 and valid[z].all() and np.isnan(J[z]).all() and np.isnan(d[z]).all()
    # rank-deficient neighbour sets: the oracle terminates; what it returns is what the device must return
    assert int(_fam(lab, "identical").sum()) == 50 and int(_fam(lab, "collinear").sum()) == 100
    # only the rotation enters J
    a, b = _fam(lab, "pose_a"), _fam(lab, "pose_b")
    assert valid[a].all() and valid[b].all() and LC.same_bits(J[a], J[b]).all() and LC.same_bits(d[a], d[b]).all()
    assert (np.abs(T[b][:, 12:15]).max(1) > 1e4).all() and np.array_equal(T[a][:, :12], T[b][:, :12])
    # where invalid the outputs are untouched
    assert (J[~valid] == FC.CANARY).all() and (d[~valid] == FC.CANARY).all()


def test_line_residual_families_reach_their_gates():
    nn, ps, pt, T, gate, lab = FC.line_residual_cases()
    valid, J, d = FC.oracle_line_residual()
    assert 800 <= lab.shape[0] <= 1200
    print("line residual:", {f: (int((lab == f).sum()), int(valid[lab == f].sum())) for f in dict.fromkeys(lab)})
    at = np.char.startswith(lab, "ratio_")
    assert int(valid[at].sum()) >= 100 and int((~valid[at]).sum()) >= 100
    # S0 <= ratio S1 is monotonic in the ratio: two doubles below S0 / S1 is valid, two above is not; the three in between are the oracle's to decide
    assert valid[_fam(lab, "ratio_m2")].all() and not valid[_fam(lab, "ratio_p2")].any()
    nl = _fam(lab, "noisy_line")
    assert int(valid[nl].sum()) >= 50 and int((~valid[nl]).sum()) >= 20
    dz = _fam(lab, "dist_zero")
    assert int(dz.sum()) >= 20 and valid[dz].all() and (d[dz] == 0.0).all() and np.isnan(J[dz]).all()
    assert not valid[_fam(lab, "identical")].any() and not valid[_fam(lab, "zeros")].any()   # S = 0: 0 <= ratio * 0
    assert valid[_fam(lab, "collinear")].all()                                                  # S1 = 0 exactly or nearly: S0 > ratio S1
    a, b = _fam(lab, "pose_a"), _fam(lab, "pose_b")
    assert valid[a].all() and valid[b].all() and LC.same_bits(J[a], J[b]).all() and LC.same_bits(d[a], d[b]).all()
    fin = valid & ~dz
    assert np.isfinite(J[fin]).all() and (d[fin] > 0).all()
    # J[3:6] = n x u is a unit vector's cross product with a unit vector orthogonal to it: norm 1
    assert np.abs(np.linalg.norm(J[fin][:, 3:6], axis=1) - 1.0).max() < 1e-6


def test_icp_point_rows_model_is_the_icp_jacobian():
    T, p, m, lab = FC.icp_point_rows_cases()
    J, e, res = FC.icp_point_rows_model(T, p, m)
    n = T.shape[0]
    assert n == 460 and np.isfinite(J).all()
    Jm = J.reshape(n, 6, 3).transpose(0, 2, 1)   # column-major 3 x 6 -> [s, row, col]
    assert (Jm[:, :, :3] == np.eye(3)).all()
    R = T.reshape(n, 4, 4).transpose(0, 2, 1)[:, :3, :3]
    hat = np.zeros((n, 3, 3))
    hat[:, 0, 1], hat[:, 0, 2], hat[:, 1, 2] = -p[:, 2], p[:, 1], -p[:, 0]
    hat -= hat.transpose(0, 2, 1)
    assert np.abs(Jm[:, :, 3:] + R @ hat).max() <= 1e-12 * 2500.0
    q = np.einsum("nij,nj->ni", R, p) + T[:, 12:15]
    assert (np.abs(e - (q - m)) <= 1e-6 * (1.0 + np.abs(q).max(1, keepdims=True) + np.abs(p).max(1, keepdims=True))).all()   # (float transform)
    assert np.abs(res - np.linalg.norm(e, axis=1)).max() <= 1e-12 * 5000.0
    ez = lab == "e_zero"
    assert int(ez.sum()) == 40 and (e[ez] == 0.0).all() and (res[ez] == 0.0).all()
    og = lab == "origin"
    assert (Jm[og][:, :, 3:] == 0.0).all() and np.signbit(Jm[og][:, :, 3:]).any()   # zeros of both signs: the bit comparison sees them
    assert (np.abs(p[lab == "far"]).max(1) > 100.0).all()


def _int_expected(x, y):
    return (x * y).sum(0)   # exact: integers below 2^20 times 64


def test_rank1_families():
    for cases, terms in ((FC.rank1_cases(), FC.rank1_terms), (FC.rank1x3_cases(), FC.rank1x3_terms)):
        contrib, J, r, lab, twin = cases
        n = lab.shape[0]
        ints = np.char.startswith(lab, "int_")
        assert int(ints.sum()) == 2 * len(FC.lane_masks()) and len(FC.lane_masks()) == 2 + 64 + 8 + 4
        for s in np.nonzero(ints)[0]:
            x, y = terms(contrib[s], J[s], r[s])
            assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 1024 and np.abs(y).max() <= 1024
            ex, _ = FC.exact_sums(x, y)
            assert [Fraction(float(v)) for v in _int_expected(x, y)] == ex   # the float sum IS the exact sum
            if twin[s] >= 0:   # poisoned: the lanes that do not contribute (and, three-row form, that own nothing) carry NaN, Inf or 1e308
                t = twin[s]
                x2, y2 = terms(contrib[t], J[t], r[t])
                assert np.array_equal(x, x2) and np.array_equal(y, y2) and np.array_equal(contrib[s], contrib[t])
                used = contrib[s] & ((np.arange(64) % 8 == 0) if J.shape[2] == 18 else True)
                assert used.all() or not np.isfinite(J[s][~used]).all() or (np.abs(J[s][~used]) >= 1e308).any()
                assert (J[t][~used] == 0.0).all() and (r[t][~used] == 0.0).all()
        if J.shape[2] == 6:   # the DPP model on the integer family is the exact sum too (any order is)
            model = FC.rank1_dpp_model(contrib[ints], J[ints], r[ints])
            want = np.stack([_int_expected(*terms(contrib[s], J[s], r[s])) for s in np.nonzero(ints)[0]])
            assert np.array_equal(model, want)
            # and on the wide family it is NOT the left-to-right sum: the order shows in the bits
            w = lab == "wide"
            model = FC.rank1_dpp_model(contrib[w], J[w], r[w])
            ltr = np.zeros_like(model)
            for k, s in enumerate(np.nonzero(w)[0]):
                x, y = terms(contrib[s], J[s], r[s])
                for l in range(64):
                    ltr[k] = ltr[k] + x[l] * y[l]
            assert (model[:, :27] != ltr[:, :27]).mean() > 0.5
        # the family built to cancel does: in most cases some column's sum is below 1e-6 of the sum of its terms' magnitudes
        hit = 0
        for s in np.nonzero(lab == "cancel")[0]:
            ex, ab = FC.exact_sums(*terms(contrib[s], J[s], r[s]))
            hit += int(any(a > 0 and abs(e) <= a * Fraction(1, 10 ** 6) for e, a in zip(ex, ab)))
        assert hit >= 12, hit
        rep = np.nonzero(lab == "repeat")[0]
        assert sorted(set(int(s) % 4 for s in rep)) == [0, 1, 2, 3] and len(set(int(s) // 4 for s in rep)) == 2   # every wave slot, two workgroups
        assert n <= 400


def test_reduce_partials_model_is_a_sum_in_its_own_order():
    wide, ints = FC.partial_rows()
    differ = total = 0
    for variant, (NT, U) in enumerate(FC.REDUCE_VARIANTS):
        NG = NT // 32
        counts = FC.reduce_row_counts(variant)
        assert {1, NG, 205, 225, 457} <= set(counts) and max(counts) <= 1100
        if variant == 0:   # where the three straight-line variants of the 256-thread form switch
            assert {223, 224, 225, 255, 256, 257} <= set(counts)
        for nrows in counts:
            assert np.array_equal(FC.reduce_partials_model(ints, nrows, NT, U), ints[:nrows].sum(0))   # integers: exact in any order
            got = FC.reduce_partials_model(wide, nrows, NT, U)
            ltr = np.zeros(32)
            for k in range(nrows):
                ltr = ltr + wide[k]
            exact = np.array([float(sum((Fraction(float(v)) for v in wide[:nrows, c]), Fraction(0))) for c in (0, 31)])
            assert (np.abs(got[[0, 31]] - exact) <= FC.gamma(nrows + NG) * np.abs(wide[:nrows, [0, 31]]).sum(0)).all()
            total += 1
            differ += int(not np.array_equal(got, ltr))
    print("reduce_partials model differs from the left-to-right sum for %d of %d row counts" % (differ, total))
    assert differ >= 0.75 * total


def test_fanin_totals():
    for nb in FC.FANIN_BLOCKS:
        t = FC.fanin_totals(nb)
        assert t.shape == (2, 32) and t[0, 0] == nb * (nb + 1) / 2 and t[1, 0] == nb * (nb + 1) + 1000 * nb * (nb - 1) / 2
        assert t.max() < 2.0 ** 40
