"""include/fls_debug_knn.h without a GPU: every declared symbol is exported by both libraries and listed in DEBUG_KNN_SYMBOLS, the list shares
nothing with the other symbol lists, the header's own revision is 1 while FLS_ABI_REVISION and the other debug headers stay what they were, and
every invalid argument of every hook is refused before the device is looked at, the outputs left alone; empty inputs are answered without a launch."""
import ctypes as C
import os
import re

import numpy as np

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP, DP, IP, BP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
NAN, INF = float("nan"), float("inf")


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src))


def test_debug_knn_symbols_exported_declared_and_listed(built):
    L = _lib.lib()
    declared = _declared("fls_debug_knn.h")
    assert len(declared) == 4 and declared == set(_lib.DEBUG_KNN_SYMBOLS) and len(_lib.DEBUG_KNN_SYMBOLS) == 4
    for s in declared:
        assert hasattr(L, s), s
    src = open(os.path.join(ROOT, "include", "fls_debug_knn.h")).read()
    assert "#define FLS_DEBUG_KNN_REVISION 1" in src and L.fls_debug_knn_revision() == 1
    others = (_lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.KEYFRAMES_SYMBOLS + _lib.LOCALMAP_SYMBOLS + _lib.BATCH_SYMBOLS +
              _lib.BATCH_IVOX_SYMBOLS + _lib.DEBUG_LINALG_SYMBOLS + _lib.DEBUG_FIT_SYMBOLS + _lib.DEBUG_NDT_SYMBOLS + _lib.DEBUG_LOOP_SYMBOLS + _lib.NDT_IMAGE_SYMBOLS +
              _lib.KD_IMAGE_SYMBOLS + _lib.IVOX_BLOB_SYMBOLS)
    assert not set(_lib.DEBUG_KNN_SYMBOLS) & set(others)
    dpp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libfls_reg_dpp.so"))
    for s in declared:
        assert hasattr(dpp, s), s
    assert "fls_debug_knn.h" in open(os.path.join(ROOT, "funny_lidar_slam_amd", "csrc", "Makefile")).read()


def test_the_other_headers_are_untouched(built):
    L = _lib.lib()
    assert L.fls_abi_revision() == 9 and L.fls_abi_version() == 1
    assert L.fls_debug_linalg_revision() == 1 and L.fls_debug_fit_revision() == 1 and L.fls_debug_ndt_revision() == 1 and L.fls_debug_loop_revision() == 1
    assert "#define FLS_ABI_REVISION 9" in open(os.path.join(ROOT, "include", "fls_reg.h")).read()
    assert len(_declared("fls_debug_linalg.h")) == 6 and _declared("fls_debug_linalg.h") == set(_lib.DEBUG_LINALG_SYMBOLS)
    assert len(_declared("fls_debug_fit.h")) == 10 and _declared("fls_debug_fit.h") == set(_lib.DEBUG_FIT_SYMBOLS)
    assert len(_declared("fls_debug_ndt.h")) == 2 and _declared("fls_debug_ndt.h") == set(_lib.DEBUG_NDT_SYMBOLS)
    assert len(_declared("fls_debug_loop.h")) == 6 and _declared("fls_debug_loop.h") == set(_lib.DEBUG_LOOP_SYMBOLS)
    assert len(_lib.EXPORTED_SYMBOLS) == 44


def _buffers():
    f = np.zeros(32 * 5 * 4, np.float32)   # clouds of up to 32 rows of 4 floats; out_pts[32][5][4]; out_kth
    d = np.eye(4).reshape(16).copy()       # T16
    i32 = np.zeros(32, np.int32)           # out_id, out_has_window
    u8 = np.zeros(32, np.uint8)            # out_cnt, out_eff
    return f, d, i32, u8


def test_debug_knn_invalid_arguments_need_no_device(built):
    """every NULL pointer position, every negative size and every value outside its domain: FLS_ERR_INVALID here, where there is no device to look
    at, and no output is written"""
    L = _lib.lib()
    inv = _lib.FLS_ERR_INVALID
    f, d, i32, u8 = _buffers()
    F, D, I, B = f.ctypes.data_as(FP), d.ctypes.data_as(DP), i32.ctypes.data_as(IP), u8.ctypes.data_as(BP)

    def sweep(fn, args, pointers, sizes, values):
        """fn(*args) with each pointer position in turn NULL, each size position in turn -1, each (position, value) in turn"""
        for k in pointers:
            q = list(args); q[k] = None
            assert fn(*q) == inv, (fn.__name__, "NULL at", k)
        for k in sizes:
            q = list(args); q[k] = -1
            assert fn(*q) == inv, (fn.__name__, "-1 at", k)
        for k, v in values:
            q = list(args); q[k] = v
            assert fn(*q) == inv, (fn.__name__, v, "at", k)

    # (device, map, nm, query, nq, stride, cell, rings, gate, T16, host_grid, out_pts, out_cnt, out_kth, out_has_window)
    a = [0, F, 32, F, 32, 4, 1.0001, 1, 1.0, D, 0, F, B, F, I]
    sweep(L.fls_debug_grid_knn5, a, (1, 3, 9, 11, 12, 13, 14), (2, 4),
          ((5, 2), (5, 0), (6, 0.0), (6, -1.0), (6, NAN), (6, INF), (7, 0), (7, 3), (7, -1), (8, NAN), (10, 2), (10, -1)))
    # (device, map_a, nm_a, query_a, nq_a, cell_a, rings_a, gate_a, map_b, nm_b, query_b, nq_b, cell_b, rings_b, gate_b, stride, T16, host_grid,
    #  out_pts_a, out_cnt_a, out_kth_a, out_has_window_a, out_pts_b, out_cnt_b, out_kth_b, out_has_window_b)
    a = [0, F, 32, F, 32, 0.50005, 2, 1.0, F, 32, F, 32, 1.0001, 1, 1.0, 4, D, 0, F, B, F, I, F, B, F, I]
    sweep(L.fls_debug_grid_knn5_dual, a, (1, 3, 8, 10, 16, 18, 19, 20, 21, 22, 23, 24, 25), (2, 4, 9, 11),
          ((15, 2), (5, 0.0), (5, NAN), (5, INF), (12, 0.0), (12, -0.5), (12, NAN), (6, 0), (6, 3), (13, 0), (13, 3), (7, NAN), (14, NAN), (17, 2), (17, -1),
           (7, INF), (14, INF),             # the dual kernel has no un-gated form
           (2, 0), (4, 0), (9, 0), (11, 0)))  # nor is it launched with an empty class
    # (device, map, nm, query, nq, stride, cell, max_corr_sq, T16, host_grid, out_id, out_eff, out_has_window)
    a = [0, F, 32, F, 32, 4, 1.0001, 1.0, D, 0, I, B, I]
    sweep(L.fls_debug_icp_knn1, a, (1, 3, 8, 10, 11, 12), (2, 4), ((5, 2), (6, 0.0), (6, NAN), (6, INF), (7, 0.0), (7, -1.0), (7, NAN), (7, INF), (9, 2), (9, -1)))
    assert (f == 0).all() and np.array_equal(d, np.eye(4).reshape(16)) and (i32 == 0).all() and (u8 == 0).all()


def test_debug_knn_empty_inputs_need_no_device(built):
    """no map point or no query: FLS_OK without a launch -- counts 0, ids -1, the 5th distance infinite, no window; the rest of the arrays left alone"""
    L = _lib.lib()
    for nm, nq in ((0, 3), (3, 0), (0, 0)):
        f, d, i32, u8 = _buffers()
        pts, kth = np.full(4 * 5 * 4, 7.0, np.float32), np.full(4, 7.0, np.float32)
        i32[:] = 7; u8[:] = 7
        F, D, I, B = f.ctypes.data_as(FP), d.ctypes.data_as(DP), i32.ctypes.data_as(IP), u8.ctypes.data_as(BP)
        assert L.fls_debug_grid_knn5(0, F, nm, F, nq, 4, 1.0001, 1, INF, D, 0, pts.ctypes.data_as(FP), B, kth.ctypes.data_as(FP), I) == _lib.FLS_OK
        rows = pts.reshape(4, 5, 4)
        assert (rows[:nq, :, :3] == 0).all() and (rows[:nq].view(np.int32)[:, :, 3] == -1).all() and (rows[nq:] == 7.0).all()
        assert (u8[:nq] == 0).all() and (u8[nq:] == 7).all() and np.isinf(kth[:nq]).all() and (kth[nq:] == 7.0).all()
        assert i32[0] == 0 and (i32[1:] == 7).all()
        i32[:] = 7; u8[:] = 7
        win = np.full(1, 7, np.int32)
        assert L.fls_debug_icp_knn1(0, F, nm, F, nq, 4, 1.0001, 1.0, D, 1, I, B, win.ctypes.data_as(IP)) == _lib.FLS_OK
        assert (i32[:nq] == -1).all() and (i32[nq:] == 7).all() and (u8[:nq] == 0).all() and (u8[nq:] == 7).all() and win[0] == 0
