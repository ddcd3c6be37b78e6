"""The generators of tests/linalg_cases.py do what they say, by the oracle alone (no GPU): every family reaches the branch it is named after
(counted per family, asserted as minimums that follow from how the family is built), the oracle terminates with finite values on every finite
input, agrees with numpy on the non-degenerate families to the conditioning of each system, and the numpy model of the wave sum is a sum and
is NOT the left-to-right sum.  Without this file tests/test_gpu_linalg.py could pass on inputs that never leave the main path."""
import math

import numpy as np

from oracle import oracle as O
from tests import linalg_cases as LC

EPS = LC.EPS


def _count(labels, mask):
    return {f: int(mask[labels == f].sum()) for f in sorted(set(labels[mask]))}


def test_plane_fit_families_reach_their_branches():
    A, lab = LC.plane_fit_cases()
    x = LC.oracle_plane_fit()
    assert 1000 <= A.shape[0] <= 4000 and np.isfinite(A).all()
    # the oracle terminates, finite, on every family (also the planes through the origin) but one: on the all-zero matrix Eigen's own rule leaves
    # all three pivots in (ColPivHouseholderQR: `biggest_col_sq_norm < threshold_helper * (rows - k)` is 0 < 0, false, nonzeroPivots() stays 3;
    # solve() returns zero only for nonzeroPivots() == 0), so the back substitution divides -1 by 0: x = (NaN, NaN, -/+inf), not 0.  The plane
    # kernels reject such a fit (every comparison with the NaN norm is false).  Pinned here; the device must give the same (test_gpu_linalg.py).
    z = lab == "zeros"
    assert np.isfinite(x[~z]).all()
    assert np.isnan(x[z][:, :2]).all() and np.array_equal(x[z][:, 2], [-np.inf, np.inf, -np.inf, np.inf])
    f32 = lab != "general_f64"
    assert np.array_equal(A[f32], A[f32].astype(np.float32).astype(np.float64))  # what a float4 can hold
    assert not np.array_equal(A[~f32], A[~f32].astype(np.float32).astype(np.float64))
    nz = (x == 0.0).sum(1)
    all_zero, some_zero = _count(lab, nz == 3), _count(lab, (nz == 1) | (nz == 2))
    print("plane fit: x == 0 exactly:", all_zero, "; one or two exact zeros:", some_zero)
    assert all_zero == {}                                 # (no family ends at nonzeroPivots() == 0: see above)
    assert some_zero.get("axis_zero_column", 0) == 75     # a zero column is never a pivot: its component is an exact 0
    assert some_zero.get("identical", 0) >= 25            # rank 1: the integer points leave exact zeros behind the first reflection
    assert some_zero.get("collinear", 0) >= 50            # rank <= 2
    # pivot ties are ties: the two / three columns have bit-equal computed norms (squares summed in row order, as both sides do)
    for s in np.nonzero(np.char.startswith(lab, "norm_tie"))[0]:
        n2 = np.zeros(3)
        for r in range(5):
            n2 = n2 + A[s, r] * A[s, r]
        assert len(set(n2.tolist())) <= (1 if lab[s] == "norm_tie3" else 2), (s, n2)
    # the down-date's recompute branch: after the first reflection the partner column keeps less than sqrt(eps) of its squared norm
    hits = 0
    for s in np.nonzero(lab == "near_parallel")[0]:
        Q, _ = np.linalg.qr(A[s][:, [int(np.argmax((A[s] ** 2).sum(0)))]], mode="complete")
        rest = (Q.T @ A[s])[1:]
        hits += int((((rest ** 2).sum(0) / (A[s] ** 2).sum(0)) <= 1.4901161193847656e-08).sum() >= 2)  # the pivot itself and its partner
    assert hits >= 140, hits
    d = A[lab == "diagonal_only"]
    big = np.argmax((d ** 2).sum(1), axis=1)
    assert all((d[s, 1:, big[s]] == 0.0).all() and d[s, 0, big[s]] != 0.0 for s in range(d.shape[0]))  # tail == 0: tau = 0


def test_plane_fit_oracle_against_lstsq():
    A, lab = LC.plane_fit_cases()
    x = LC.oracle_plane_fit()
    checked = 0
    for s in np.nonzero(np.isin(lab, ["noisy_plane", "small_int", "general_f64", "norm_tie2", "norm_tie3", "near_parallel", "axis_const_column"]))[0]:
        sv = np.linalg.svd(A[s], compute_uv=False)
        if sv[-1] <= 1e-7 * sv[0]:
            continue  # numerically rank-deficient: the basic solution of Eigen's solve is not lstsq's minimum-norm solution
        cond = sv[0] / sv[-1]
        ref = np.linalg.lstsq(A[s], -np.ones(5), rcond=None)[0]
        # least squares: the error grows with cond^2 times the relative residual; the residual is at most |b| = sqrt(5)
        bound = 64 * EPS * (cond + cond * cond * math.sqrt(5.0) / (sv[0] * max(np.linalg.norm(ref), 1e-300))) * np.linalg.norm(ref)
        assert np.abs(x[s] - ref).max() <= bound, (s, lab[s], x[s], ref, cond)
        checked += 1
    assert checked >= 1200, checked


def test_svd3_families_reach_their_branches():
    A, lab = LC.svd3_cases()
    U, S, V = LC.oracle_svd3()
    assert 1000 <= A.shape[0] <= 4000 and np.isfinite(A).all()
    assert np.isfinite(S).all() and np.isfinite(V).all() and np.isfinite(U).all()
    assert (np.diff(S, axis=1) <= 0).all() and (S >= 0).all()
    s1_zero, tie01 = _count(lab, S[:, 1] == 0.0), _count(lab, S[:, 0] == S[:, 1])
    print("svd3: S[1] == 0:", s1_zero, "; S[0] == S[1]:", tie01)
    assert s1_zero.get("rank0", 0) == 3 and s1_zero.get("diagonal", 0) >= 25 and s1_zero.get("two_equal", 0) >= 12
    r1 = lab == "rank1"
    assert (S[r1, 1] <= 4 * EPS * S[r1, 0]).all() and (S[r1, 0] > 0).all()  # (exact rank 1 going in; the rotations may leave a rounding behind)
    assert tie01.get("isotropic", 0) == 12 and tie01.get("two_equal", 0) >= 60 and tie01.get("rank0", 0) == 3
    sym = np.array([np.array_equal(a, a.T) for a in A])
    assert sym[lab == "cov5"].all() and not sym[lab == "general"].any()  # d = m10 - m01 != 0 only off the symmetric families
    ex = np.frexp(np.abs(A[lab == "scales"]).max(axis=(1, 2)))[1]
    assert ex.min() < -800 and ex.max() > 800
    # against numpy: singular values to eps * the largest, V a right singular basis (A V = U S), orthogonal
    for s in range(A.shape[0]):
        ref = np.linalg.svd(A[s], compute_uv=False)
        assert np.abs(S[s] - ref).max() <= 32 * EPS * max(ref[0], 1e-300), (s, lab[s], S[s], ref)
        scale = max(ref[0], 1e-300)
        assert np.abs((A[s] / scale) @ V[s] - U[s] * (S[s] / scale)).max() <= 32 * EPS, (s, lab[s])
        assert np.abs(V[s].T @ V[s] - np.eye(3)).max() <= 32 * EPS, (s, lab[s])


def test_lu6_families_reach_their_branches():
    H, b, lab = LC.lu6_cases()
    inv, det, x = LC.oracle_lu6()
    assert 3000 <= H.shape[0] <= 5000 and np.isfinite(H).all() and np.isfinite(b).all()
    Hg, gg = LC.gn_systems()
    assert np.array_equal(H[:3000], Hg) and np.array_equal(b[:3000], gg)  # every system of tests/test_gpu_solver.py
    bad_inv = ~np.isfinite(inv).all(axis=(1, 2))
    zero, neg, nonfinite = _count(lab, det == 0.0), _count(lab, det < 0), _count(lab, bad_inv)
    print("lu6: det == 0:", zero, "; det < 0:", neg, "; non-finite inverse:", nonfinite)
    assert zero.get("zero", 0) == 2 and zero.get("equal_rows", 0) == 100 and zero.get("gn_kind5", 0) == 300
    for j in range(6):
        assert zero.get("zero_col%d" % j, 0) == 20 and nonfinite.get("zero_col%d" % j, 0) == 20
    assert nonfinite.get("equal_rows", 0) == 100 and nonfinite.get("zero", 0) == 2
    assert zero.get("pow2", 0) >= 5                     # 2^(6 e) det(A) underflows for e < -180
    assert np.isinf(det[lab == "pow2"]).sum() >= 5      # ... and overflows for e > 171
    for t in range(6):                                  # sign of det = parity of the transpositions
        d = det[lab == "perm_t%d" % t]
        m = H[lab == "perm_t%d" % t]
        assert d.shape[0] == 40 and (np.sign(d) == np.sign(np.linalg.det(m))).all()
        assert (d < 0).sum() >= 10 and (d > 0).sum() >= 10  # (the diagonal's own signs mix with the parity)
    assert neg.get("general", 0) >= 150 and neg.get("pivot_tie", 0) >= 50
    # ties of the pivot search: some column's largest |entry| at or below the diagonal occurs twice in the very first step
    tie = H[lab == "pivot_tie"]
    a0 = np.abs(tie[:, :, 0])
    assert ((a0 == a0.max(1, keepdims=True)).sum(1) >= 2).sum() >= 150


def test_lu6_oracle_against_numpy():
    H, b, lab = LC.lu6_cases()
    inv, det, x = LC.oracle_lu6()
    checked = 0
    for s in np.nonzero(np.isin(lab, ["general", "pivot_tie", "gn_kind0", "gn_kind8", "gn_kind9", "pow2"]) | np.char.startswith(lab, "perm_t"))[0]:
        cond = np.linalg.cond(H[s])
        if not np.isfinite(cond) or cond > 1e12:
            continue
        ref = np.linalg.inv(H[s])
        assert np.abs(inv[s] - ref).max() <= 64 * cond * EPS * np.abs(ref).max(), (s, lab[s], cond)
        if np.isfinite(det[s]) and abs(det[s]) > 1e-300:  # (a subnormal determinant has lost bits)
            sign, logdet = np.linalg.slogdet(H[s])
            assert np.sign(det[s]) == sign and abs(math.log(abs(det[s])) - logdet) <= 1e-9, (s, lab[s])
        xr = ref @ b[s]
        assert np.abs(x[s] - xr).max() <= 64 * cond * EPS * max(np.abs(ref).max() * np.abs(b[s]).max(), 1e-300), (s, lab[s])
        checked += 1
    assert checked >= 1500, checked


def test_so3_families_and_the_oracles_error():
    """E_o: the oracle's largest elementwise distance from a numpy.longdouble Rodrigues formula.  tests/test_gpu_linalg.py measures the device's E_d
    the same way and asserts E_d <= 4 max(E_o, 2^-53)."""
    v, R, lab = LC.so3_cases()
    Rd = LC.oracle_so3()
    assert np.isfinite(Rd).all()
    ident = (Rd == np.eye(3)).all(axis=(1, 2))
    cnt = _count(lab, ident)
    print("so3: exact identity:", cnt)
    assert cnt == {"zero": 2, "tiny_1e-17": 20, "eps_exact": 6, "underflow_1e-170": 20, "subnormal": 32}
    assert not ident[lab == "eps_next"].any()   # one ulp above DBL_EPS: Rodrigues
    err = LC.so3_max_error(v, Rd)
    fam = {f: float(err[lab == f].max()) for f in sorted(set(lab))}
    print("so3: oracle error per family:", fam)
    print("so3: E_o = %.3e" % err.max())
    # glibc's sin / cos are below 1 ulp; each enters one product and one sum on entries <= 1, and theta itself carries a rounding of the
    # square root: |theta| eps / 2 moves the angle, so the bound grows with |v|
    th = np.linalg.norm(v, axis=1)
    assert (err <= 4 * EPS * (1.0 + th)).all(), float((err / (EPS * (1.0 + th))).max())
    assert np.abs(np.einsum("nji,njk->nik", Rd, Rd) - np.eye(3)).max() <= 8 * EPS
    orth = np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max()
    assert orth <= 8 * EPS and (R[::5] == np.eye(3)).all()


def test_wave_sum_model_is_a_sum_and_not_the_sequential_one():
    rows, lab = LC.wave_sum_cases()
    tot = LC.wave_sum_model(rows)
    differ = 0
    for s in range(rows.shape[0]):
        exact = math.fsum(rows[s])
        assert abs(tot[s] - exact) <= 64 * EPS * np.abs(rows[s]).sum(), (s, lab[s])
        seq = 0.0
        for q in range(64):
            seq += rows[s, q]
        differ += int(lab[s] == "wide" and seq != tot[s])
    wide = int((lab == "wide").sum())
    print("wave sum: %d of %d wide rows differ from the left-to-right sum" % (differ, wide))
    assert wide >= 100 and 2 * differ >= wide
    assert (tot[lab == "zeros"] == 0.0).all()
    single = rows[lab == "single"]
    assert single.shape[0] == 64 and np.array_equal(np.nonzero(single)[1], np.arange(64))
    assert np.array_equal(tot[lab == "single"], single.sum(1))  # a lone value survives the tree unchanged, from every lane
