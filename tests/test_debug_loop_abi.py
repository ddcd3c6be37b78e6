"""include/fls_debug_loop.h without a GPU: every declared symbol is exported by both libraries and listed in DEBUG_LOOP_SYMBOLS, the list shares
nothing with the other symbol lists, the header's own revision is 1 while FLS_ABI_REVISION and the other debug headers stay what they were, and
every NULL pointer position and every negative size of every hook is refused before the device is looked at, the outputs left alone."""
import ctypes as C
import os
import re

import numpy as np

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP, DP, IP, LP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src))


def test_debug_loop_symbols_exported_declared_and_listed(built):
    L = _lib.lib()
    declared = _declared("fls_debug_loop.h")
    assert len(declared) == 6 and declared == set(_lib.DEBUG_LOOP_SYMBOLS) and len(_lib.DEBUG_LOOP_SYMBOLS) == 6
    for s in declared:
        assert hasattr(L, s), s
    src = open(os.path.join(ROOT, "include", "fls_debug_loop.h")).read()
    assert "#define FLS_DEBUG_LOOP_REVISION 1" in src and L.fls_debug_loop_revision() == 1
    others = (_lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.KEYFRAMES_SYMBOLS + _lib.LOCALMAP_SYMBOLS + _lib.BATCH_SYMBOLS +
              _lib.BATCH_IVOX_SYMBOLS + _lib.DEBUG_LINALG_SYMBOLS + _lib.DEBUG_FIT_SYMBOLS + _lib.DEBUG_NDT_SYMBOLS + _lib.NDT_IMAGE_SYMBOLS + _lib.KD_IMAGE_SYMBOLS +
              _lib.IVOX_BLOB_SYMBOLS + _lib.DEBUG_KNN_SYMBOLS)
    assert not set(_lib.DEBUG_LOOP_SYMBOLS) & set(others)
    dpp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libfls_reg_dpp.so"))
    for s in declared:
        assert hasattr(dpp, s), s
    assert "fls_debug_loop.h" in open(os.path.join(ROOT, "funny_lidar_slam_amd", "csrc", "Makefile")).read()


def test_the_other_headers_are_untouched(built):
    L = _lib.lib()
    assert L.fls_abi_revision() == 9 and L.fls_abi_version() == 1
    assert L.fls_debug_linalg_revision() == 1 and L.fls_debug_fit_revision() == 1 and L.fls_debug_ndt_revision() == 1
    assert "#define FLS_ABI_REVISION 9" in open(os.path.join(ROOT, "include", "fls_reg.h")).read()
    assert len(_declared("fls_debug_linalg.h")) == 6 and _declared("fls_debug_linalg.h") == set(_lib.DEBUG_LINALG_SYMBOLS)
    assert len(_declared("fls_debug_fit.h")) == 10 and _declared("fls_debug_fit.h") == set(_lib.DEBUG_FIT_SYMBOLS)
    assert len(_declared("fls_debug_ndt.h")) == 2 and _declared("fls_debug_ndt.h") == set(_lib.DEBUG_NDT_SYMBOLS)
    assert len(_lib.EXPORTED_SYMBOLS) == 44


def test_debug_loop_invalid_arguments_need_no_device(built):
    """every NULL pointer position and every negative size of every hook: FLS_ERR_INVALID here, where there is no device to look at, and no
    output is written"""
    L = _lib.lib()
    inv = _lib.FLS_ERR_INVALID
    f = np.zeros(32 * 4, np.float32)            # clouds of up to 32 rows of 4 floats, T[16]
    d = np.zeros(32 * 9)                        # covariances, Mahalanobis rows, p, x, R; score / grad / hess / v / sums
    i32 = np.zeros(32, np.int32)                # corr in (all zero: valid ids for nt >= 1), corr / leaves / sparse out
    i64 = np.zeros(1, np.int64)
    F, D, I, Q = f.ctypes.data_as(FP), d.ctypes.data_as(DP), i32.ctypes.data_as(IP), i64.ctypes.data_as(LP)

    def sweep(fn, args, pointers, sizes):
        """fn(*args) with each pointer position in turn NULL, then each size position in turn -1"""
        for k in pointers:
            q = list(args); q[k] = None
            assert fn(*q) == inv, (fn.__name__, "NULL at", k)
        for k in sizes:
            q = list(args); q[k] = -1
            assert fn(*q) == inv, (fn.__name__, "-1 at", k)

    # (device, src, ns, tgt, nt, stride, resolution, p, want_hessian, score, grad, hess, pairs, leaves, sparse)
    a = [0, F, 32, F, 32, 4, 3.0, D, 1, D, D, D, Q, I, I]
    sweep(L.fls_debug_loop_ndt, a, (1, 3, 7, 9, 10, 11, 12, 13, 14), (2, 4))
    for stride, res in ((2, 3.0), (4, 0.0), (4, -1.0), (4, float("nan")), (4, float("inf"))):
        q = list(a); q[5] = stride; q[6] = res
        assert L.fls_debug_loop_ndt(*q) == inv
    # (device, cloud, n, stride, cell, epsilon, host_grid, cov)
    a = [0, F, 32, 4, 1.5, 0.001, 0, D]
    sweep(L.fls_debug_loop_gicp_cov, a, (1, 7), (2,))
    for n in (0, 1, 19):  # LoopMatcher::run never launches the kernel below 20 points
        q = list(a); q[2] = n
        assert L.fls_debug_loop_gicp_cov(*q) == inv
    for k, v in ((3, 2), (4, 0.0), (4, float("nan")), (5, 0.0), (6, 2), (6, -1)):
        q = list(a); q[k] = v
        assert L.fls_debug_loop_gicp_cov(*q) == inv
    # (device, moved, ns, tgt, nt, stride, T, R, cov_src, cov_tgt, corr_dist, host_grid, corr, mahal)
    a = [0, F, 32, F, 32, 4, F, D, D, D, 2.0, 0, I, D]
    sweep(L.fls_debug_loop_gicp_corr, a, (1, 3, 6, 7, 8, 9, 12, 13), (2, 4))
    for k, v in ((5, 2), (10, 0.0), (10, -2.0), (10, float("nan")), (11, 2)):
        q = list(a); q[k] = v
        assert L.fls_debug_loop_gicp_corr(*q) == inv
    # (device, moved, ns, tgt, nt, stride, x, corr, mahal, want_grad, v)
    a = [0, F, 32, F, 32, 4, D, I, D, 1, D]
    sweep(L.fls_debug_loop_gicp_fdf, a, (1, 3, 6, 7, 8, 10), (2, 4))
    q = list(a); q[5] = 2
    assert L.fls_debug_loop_gicp_fdf(*q) == inv
    for bad in (-2, 32, 2 ** 31 - 1):  # a correspondence outside [-1, nt): the kernel would index the target with it
        i32[5] = bad
        assert L.fls_debug_loop_gicp_fdf(*a) == inv, bad
        i32[5] = 0
    # (device, src, ns, tgt, nt, stride, T, host_grid, sum_d2, count)
    a = [0, F, 32, F, 32, 4, F, 0, D, Q]
    sweep(L.fls_debug_loop_fitness, a, (1, 3, 6, 8, 9), (2, 4))
    for k, v in ((5, 2), (7, 2)):
        q = list(a); q[k] = v
        assert L.fls_debug_loop_fitness(*q) == inv
    assert (f == 0).all() and (d == 0.0).all() and (i32 == 0).all() and (i64 == 0).all()


def test_debug_loop_empty_inputs_need_no_device(built):
    """zero points where the hook's meaning allows it: FLS_OK and zero results without a launch"""
    L = _lib.lib()
    f = np.zeros(32 * 4, np.float32)
    d = np.full(64, 7.0)
    i32 = np.full(8, 7, np.int32)
    i64 = np.full(1, 7, np.int64)
    F, D, I, Q = f.ctypes.data_as(FP), d.ctypes.data_as(DP), i32.ctypes.data_as(IP), i64.ctypes.data_as(LP)
    D1 = C.cast(C.addressof(D.contents) + 8, DP)   # score d[0], grad d[1:7], hess d[7:43]
    D7 = C.cast(C.addressof(D.contents) + 56, DP)
    six = np.zeros(6)
    X = six.ctypes.data_as(DP)
    for ns, nt in ((0, 32), (32, 0), (0, 0)):
        d[:] = 7.0; i32[:] = 7; i64[:] = 7
        assert L.fls_debug_loop_ndt(0, F, ns, F, nt, 4, 3.0, X, 1, D, D1, D7, Q, I, C.cast(C.addressof(I.contents) + 4, IP)) == _lib.FLS_OK
        assert (d[:43] == 0.0).all() and d[43] == 7.0 and i64[0] == 0 and i32[0] == 0 and i32[1] == 0 and i32[2] == 7
        d[:] = 7.0; i64[:] = 7
        assert L.fls_debug_loop_fitness(0, F, ns, F, nt, 4, F, 0, D, Q) == _lib.FLS_OK
        assert d[0] == 0.0 and i64[0] == 0
    d[:] = 7.0
    assert L.fls_debug_loop_gicp_fdf(0, F, 0, F, 32, 4, X, I, X, 1, D) == _lib.FLS_OK and (d[:14] == 0.0).all() and d[14] == 7.0
    d[:] = 7.0; i32[:] = 7
    assert L.fls_debug_loop_gicp_corr(0, F, 0, F, 32, 4, F, D, D, D, 2.0, 0, I, D) == _lib.FLS_OK and (d == 7.0).all() and (i32 == 7).all()
    big = np.full(4 * 9, 7.0)
    assert L.fls_debug_loop_gicp_corr(0, F, 4, F, 0, 4, F, D, D, D, 2.0, 0, I, big.ctypes.data_as(DP)) == _lib.FLS_OK
    assert (i32[:4] == -1).all() and (i32[4:] == 7).all() and np.isnan(big).all()
