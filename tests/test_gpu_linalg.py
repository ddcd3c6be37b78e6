"""The device linear-algebra primitives, each on its own, against the oracle's restatement (oracle/flo_linalg.h) or a numpy model -- never against
another device path: plane_fit_5x3, jacobi_svd3_v, so3_exp_dev, mat3_mul_dev (csrc/linalg_dev.hpp), lu6_solve_wave, wave_sum_dpp
(csrc/wave_solve.hpp), through the hooks of include/fls_debug_linalg.h, which call the __forceinline__ routines themselves the way the matcher
kernels do.  BIT FOR BIT wherever both sides execute the same IEEE operations (everything but the sine and cosine of SO3Exp).  The inputs and
what they reach are tests/linalg_cases.py and tests/test_oracle_linalg_cases.py; one launch per routine."""
import ctypes as C

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib
from tests import linalg_cases as LC

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)


def _p(a):
    assert a.flags["C_CONTIGUOUS"] and a.dtype == np.float64
    return a.ctypes.data_as(DP)


def _report(name, ok, labels, show):
    """ok: (n,) bool.  Names the families of the failing systems and prints the first few."""
    bad = np.nonzero(~ok)[0]
    if bad.size:
        fam = {}
        for s in bad:
            fam[str(labels[s])] = fam.get(str(labels[s]), 0) + 1
        for s in bad[:5]:
            print(name, "system", int(s), "family", labels[s], *show(int(s)))
        pytest.fail("%s: %d of %d systems differ from the oracle, by family %s" % (name, bad.size, ok.size, fam))


def test_plane_fit_5x3_bit_exact_against_oracle(built):
    assert _lib.device_count() >= 1
    A, lab = LC.plane_fit_cases()
    n = A.shape[0]
    Ac = np.ascontiguousarray(A.transpose(0, 2, 1)).reshape(n, 15)  # column-major per system
    x = np.full((n, 3), 7.0)
    assert _lib.lib().fls_debug_plane_fit_5x3(0, _p(Ac), n, _p(x)) == 0
    ref = LC.oracle_plane_fit()
    # exact zeros are equal whatever their sign; the NaNs of the all-zero matrix (see test_oracle_linalg_cases.py) are NaNs on both sides
    ok = LC.same_bits(x, ref, zero_sign_free=True, nan_free=True).all(1)
    _report("plane_fit_5x3", ok, lab, lambda s: (A[s].tolist(), ref[s], x[s]))
    assert np.isfinite(x[lab != "zeros"]).all()


def test_svd3_bit_exact_against_oracle(built):
    assert _lib.device_count() >= 1
    A, lab = LC.svd3_cases()
    n = A.shape[0]
    Ac = np.ascontiguousarray(A.transpose(0, 2, 1)).reshape(n, 9)
    S = np.full((n, 3), 7.0); V = np.full((n, 9), 7.0)
    assert _lib.lib().fls_debug_svd3(0, _p(Ac), n, _p(S), _p(V)) == 0
    V = V.reshape(n, 3, 3).transpose(0, 2, 1)  # column-major -> V[s][row, col]
    _, Sref, Vref = LC.oracle_svd3()
    ok = LC.same_bits(S, Sref).all(1) & LC.same_bits(V, Vref).all(axis=(1, 2))
    _report("jacobi_svd3_v", ok, lab, lambda s: (A[s].tolist(), Sref[s], S[s], Vref[s].tolist(), V[s].tolist()))


def test_lu6_bit_exact_against_oracle(built):
    assert _lib.device_count() >= 1
    H, b, lab = LC.lu6_cases()
    n = H.shape[0]
    Hc = np.ascontiguousarray(H.transpose(0, 2, 1)).reshape(n, 36)
    det = np.full(n, 7.0); inv = np.full((n, 36), 7.0); x = np.full((n, 6), 7.0)
    assert _lib.lib().fls_debug_lu6(0, _p(Hc), _p(np.ascontiguousarray(b)), n, _p(det), _p(inv), _p(x)) == 0
    inv = inv.reshape(n, 6, 6).transpose(0, 2, 1)
    inv_ref, det_ref, x_ref = LC.oracle_lu6()
    # det: the same bits (a NaN, which only an overflowing product can make, is a NaN on both sides), and exactly the same systems at det == 0.0:
    # the reference's "skip the update" branch (icp_optimized.h:129)
    ok_det = LC.same_bits(det, det_ref, nan_free=True) & ((det == 0.0) == (det_ref == 0.0))
    _report("lu6 det", ok_det, lab, lambda s: (det_ref[s], det[s]))
    assert int((det == 0.0).sum()) >= 1000 and int((det < 0).sum()) >= 400
    # inverse: the same bits where finite or infinite; a NaN position on one side is a NaN position on the other (payload and sign of a NaN
    # differ between x86 and the GPU)
    ok_inv = LC.same_bits(inv, inv_ref, nan_free=True).all(axis=(1, 2)) & (np.isnan(inv) == np.isnan(inv_ref)).all(axis=(1, 2))
    _report("lu6 inverse", ok_inv, lab, lambda s: (H[s].tolist(), inv_ref[s].tolist(), inv[s].tolist()))
    # x = inverse * b, summed left to right from 0.0 over the ORACLE's inverse
    ok_x = LC.same_bits(x, x_ref, nan_free=True).all(1) & (np.isnan(x) == np.isnan(x_ref)).all(1)
    _report("lu6 inverse * b", ok_x, lab, lambda s: (x_ref[s], x[s]))


def test_so3_exp_and_mat3_mul(built):
    """Rd: identity exactly where the oracle's is; elsewhere the device's libm sincos stands against glibc's sin and cos, so the distance from a
    numpy.longdouble Rodrigues formula is compared: E_d <= 4 max(E_o, 2^-53) with E_o the oracle's own distance (a few-ulp sine and cosine, each
    entering one product and one sum on entries of magnitude <= 1).  Measured: E_o = 7.67e-14 (test_oracle_linalg_cases.py),
    E_d = 7.67e-14 (the rounding of theta = |v| up to 1e3 dominates both sides; family by family the two agree to 1e-17, both values are printed).
    mat3_mul_dev is pinned bit for bit on the device's own Rd, in both orders of the tails."""
    assert _lib.device_count() >= 1
    v, R, lab = LC.so3_cases()
    n = v.shape[0]
    Rc = np.ascontiguousarray(R.transpose(0, 2, 1)).reshape(n, 9)
    out = [np.full((n, 9), 7.0) for _ in range(3)]
    assert _lib.lib().fls_debug_so3(0, _p(np.ascontiguousarray(v)), _p(Rc), n, _p(out[0]), _p(out[1]), _p(out[2])) == 0
    Rd, R_Rd, Rd_R = (o.reshape(n, 3, 3).transpose(0, 2, 1) for o in out)
    Rd_ref = LC.oracle_so3()
    eye = np.eye(3)
    ident, ident_ref = (Rd == eye).all(axis=(1, 2)), (Rd_ref == eye).all(axis=(1, 2))
    _report("so3_exp_dev identity branch", ident == ident_ref, lab, lambda s: (v[s], Rd_ref[s].tolist(), Rd[s].tolist()))
    assert int(ident.sum()) == 80
    ok = LC.same_bits(R_Rd, LC.mat3_mul_model(R, Rd)).all(axis=(1, 2)) & LC.same_bits(Rd_R, LC.mat3_mul_model(Rd, R)).all(axis=(1, 2))
    _report("mat3_mul_dev", ok, lab, lambda s: (R[s].tolist(), Rd[s].tolist(), R_Rd[s].tolist(), Rd_R[s].tolist()))
    err_o, err_d = LC.so3_max_error(v, Rd_ref), LC.so3_max_error(v, Rd)
    for f in sorted(set(lab)):
        print("so3 family %-18s oracle %.3e device %.3e" % (f, err_o[lab == f].max(), err_d[lab == f].max()))
    E_o, E_d = float(err_o.max()), float(err_d.max())
    orth = float(np.abs(np.einsum("nji,njk->nik", Rd, Rd) - eye).max())
    print("so3: E_o = %.3e  E_d = %.3e  |Rd^T Rd - I| = %.3e" % (E_o, E_d, orth))
    assert E_d <= 4 * max(E_o, 2.0 ** -53), (E_d, E_o)
    # the same, system by system, so that the large angles do not hide the small ones: the bound test_oracle_linalg_cases.py holds the oracle to
    # (theta carries half an ulp of its own, which moves sine and cosine by at most theta eps / 2; a few-ulp sincos, one product and one sum each)
    th = np.linalg.norm(v, axis=1)
    _report("so3_exp_dev vs longdouble", err_d <= 4 * LC.EPS * (1.0 + th), lab, lambda s: (v[s], err_o[s], err_d[s]))
    assert orth <= 8 * LC.EPS, orth


def test_wave_sum_dpp_bit_exact_against_tree_model(built):
    assert _lib.device_count() >= 1
    rows, lab = LC.wave_sum_cases()
    n = rows.shape[0]
    tot = np.full(n, 7.0)
    assert _lib.lib().fls_debug_wave_sum(0, _p(np.ascontiguousarray(rows)), n, _p(tot)) == 0
    ref = LC.wave_sum_model(rows)
    _report("wave_sum_dpp", LC.same_bits(tot, ref), lab, lambda s: (ref[s], tot[s]))


def test_hooks_validate_before_the_device(built):
    L = _lib.lib()
    a = np.zeros(64)
    inv = _lib.FLS_ERR_INVALID
    assert L.fls_debug_plane_fit_5x3(0, None, 1, _p(a)) == inv and L.fls_debug_plane_fit_5x3(0, _p(a), 1, None) == inv
    assert L.fls_debug_svd3(0, _p(a), -1, _p(a), _p(a)) == inv and L.fls_debug_lu6(0, _p(a), None, 1, _p(a), _p(a), _p(a)) == inv
    assert L.fls_debug_so3(0, _p(a), _p(a), 1, _p(a), None, _p(a)) == inv and L.fls_debug_wave_sum(0, _p(a), -3, _p(a)) == inv
    assert L.fls_debug_wave_sum(0, _p(a), 0, _p(a)) == 0 and L.fls_debug_lu6(0, _p(a), _p(a), 0, _p(a), _p(a), _p(a)) == 0
