"""include/fls_loop_device.h and include/fls_debug_loop_leaves.h without a GPU: the declared symbols are exported by both libraries and listed
in _lib, the headers have revisions of their own while FLS_ABI_REVISION, FLS_KEYFRAMES_REVISION and FLS_DEBUG_LOOP_REVISION stay what they were,
argument errors are refused before any device is opened (here there is none: a call that got as far as the device would answer
FLS_ERR_DEVICE), and an unknown counter slot is 0.  What needs a device is in tests/test_gpu_loop_device.py and tests/test_gpu_loop_leaves.py."""
import ctypes as C
import os
import re

import numpy as np

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP, DP, IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src))


def test_symbols_exported_declared_and_listed(built):
    L = _lib.lib()
    dpp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libfls_reg_dpp.so"))
    for header, listed, n in (("fls_loop_device.h", _lib.LOOP_DEVICE_SYMBOLS, 4), ("fls_debug_loop_leaves.h", _lib.DEBUG_LOOP_LEAVES_SYMBOLS, 3)):
        declared = _declared(header)
        assert declared == set(listed) and len(listed) == n, header
        for s in declared:
            assert hasattr(L, s) and hasattr(dpp, s), s
        assert header in open(os.path.join(ROOT, "funny_lidar_slam_amd", "csrc", "Makefile")).read()
        assert header in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    others = (_lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.FEATURES_DEVICE_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.KEYFRAMES_SYMBOLS + _lib.LOCALMAP_SYMBOLS +
              _lib.BATCH_SYMBOLS + _lib.BATCH_IVOX_SYMBOLS + _lib.DEBUG_LINALG_SYMBOLS + _lib.DEBUG_FIT_SYMBOLS + _lib.DEBUG_NDT_SYMBOLS + _lib.DEBUG_LOOP_SYMBOLS +
              _lib.DEBUG_KNN_SYMBOLS + _lib.DEBUG_IVOX_KNN_SYMBOLS + _lib.DEBUG_IVOX_UPDATE_SYMBOLS + _lib.NDT_IMAGE_SYMBOLS + _lib.KNN_ORDER_SYMBOLS)
    assert not (set(_lib.LOOP_DEVICE_SYMBOLS) | set(_lib.DEBUG_LOOP_LEAVES_SYMBOLS)) & set(others)
    assert not set(_lib.LOOP_DEVICE_SYMBOLS) & set(_lib.DEBUG_LOOP_LEAVES_SYMBOLS)


def test_revisions(built):
    L = _lib.lib()
    assert "#define FLS_LOOP_DEVICE_REVISION 1" in open(os.path.join(ROOT, "include", "fls_loop_device.h")).read() and L.fls_loop_device_revision() == 1
    assert "#define FLS_DEBUG_LOOP_LEAVES_REVISION 1" in open(os.path.join(ROOT, "include", "fls_debug_loop_leaves.h")).read()
    assert L.fls_debug_loop_leaves_revision() == 1
    # the headers this one stands beside keep their revisions and their symbols
    assert L.fls_abi_revision() == 9 and L.fls_abi_version() == 1 and L.fls_keyframes_revision() == 1 and L.fls_debug_loop_revision() == 1
    assert "#define FLS_ABI_REVISION 9" in open(os.path.join(ROOT, "include", "fls_reg.h")).read()
    kf = open(os.path.join(ROOT, "include", "fls_keyframes.h")).read()
    assert "#define FLS_KEYFRAMES_REVISION 1" in kf and _declared("fls_keyframes.h") == set(_lib.KEYFRAMES_SYMBOLS)
    assert "is not part of revision 1" not in kf and "fls_loop_device.h" in kf
    assert len(_lib.EXPORTED_SYMBOLS) == 44 and _declared("fls_debug_loop.h") == set(_lib.DEBUG_LOOP_SYMBOLS)


def test_invalid_arguments_need_no_device(built):
    """every refusal below is FLS_ERR_INVALID with T, fitness and stats left alone; 0x1000 stands for a device address that is never read"""
    L = _lib.lib()
    inv = _lib.FLS_ERR_INVALID
    T = np.full(16, 7.0)
    fit = C.c_float(7.0)
    p, tp, fp = 0x1000, T.ctypes.data_as(DP), C.byref(fit)
    good = [p, p, p, p, 10, p, p, p, p, 10]

    def call(args, t=tp, f=fp):
        return L.fls_loop_match_device(0, *args, t, f, None)

    assert call(good, t=None) == inv and call(good, f=None) == inv
    for k in (0, 1, 2, 5, 6, 7):  # a NULL x, y or z plane of a cloud that has points (the intensity planes 3 and 8 may be NULL)
        a = list(good)
        a[k] = None
        assert call(a) == inv, k
    assert call([None, None, None, None, 10, p, p, p, p, 10]) == inv, "n_src points and no planes"
    assert call([p, p, p, p, 10, None, None, None, None, 3]) == inv, "n_tgt points and no planes"
    for k in (0, 3, 7, 8):  # a plane that is not 4-byte aligned
        a = list(good)
        a[k] = p + 2
        assert call(a) == inv, k
    a = list(good)
    a[4] = 4000000001
    assert call(a) == inv, "more points than the keyframe store merges"
    assert (T == 7.0).all() and fit.value == 7.0
    # the keyframe form: no handle
    ids = np.zeros(2, np.int32)
    poses = np.tile(np.eye(4).reshape(-1), 2)
    assert L.fls_keyframes_loop_match_device(None, ids.ctypes.data_as(IP), poses.ctypes.data_as(DP), 2, ids.ctypes.data_as(IP), poses.ctypes.data_as(DP), 2, tp, fp,
                                             None) == inv
    assert (T == 7.0).all() and fit.value == 7.0


def test_unknown_stat_slot_is_zero(built):
    L = _lib.lib()
    assert len(_lib.LOOP_DEVICE_STAT_SLOTS) == 7
    for slot in (-1, 7, 8, 1 << 20):
        assert L.fls_loop_device_stat(0, slot) == 0, slot
        assert L.fls_loop_device_stat(-3, slot) == 0 and L.fls_loop_device_stat(99, slot) == 0


def test_debug_hooks_refuse_bad_arguments(built):
    L = _lib.lib()
    inv = _lib.FLS_ERR_INVALID
    t = np.zeros((8, 3), np.float32)
    cell, npts, mean, icov, cen = np.full(8, -7, np.int32), np.full(8, -7, np.int32), np.full(24, 7.0), np.full(72, 7.0), np.full(24, 7.0, np.float32)
    nl, sp = C.c_int32(-7), C.c_int32(-7)

    def leaves(tgt=t.ctypes.data_as(FP), nt=8, stride=3, res=2.0, on_device=1, cap=8, n_leaves=C.byref(nl), sparse=C.byref(sp), c=cell.ctypes.data_as(IP)):
        return L.fls_debug_loop_leaves(0, tgt, nt, stride, res, on_device, c, npts.ctypes.data_as(IP), mean.ctypes.data_as(DP), icov.ctypes.data_as(DP),
                                       cen.ctypes.data_as(FP), cap, n_leaves, sparse)

    assert leaves(tgt=None) == inv and leaves(nt=-1) == inv and leaves(stride=2) == inv and leaves(res=0.0) == inv and leaves(res=float("nan")) == inv
    assert leaves(on_device=2) == inv and leaves(cap=-1) == inv and leaves(n_leaves=None) == inv and leaves(sparse=None) == inv and leaves(c=None) == inv
    assert nl.value == -7 and sp.value == -7 and (cell == -7).all() and (mean == 7.0).all()
    assert leaves(nt=0) == _lib.FLS_OK and nl.value == 0 and sp.value == 0, "an empty target has no leaves: no device is looked at"
    score, pairs, lv, sps = C.c_double(7.0), C.c_int64(-7), C.c_int32(-7), C.c_int32(-7)
    g, H, pose = np.full(6, 7.0), np.full(36, 7.0), np.zeros(6)

    def ndt(src=t.ctypes.data_as(FP), ns=8, res=2.0, p=pose.ctypes.data_as(DP)):
        return L.fls_debug_loop_ndt_device(0, src, ns, t.ctypes.data_as(FP), 8, 3, res, p, 1, C.byref(score), g.ctypes.data_as(DP), H.ctypes.data_as(DP),
                                           C.byref(pairs), C.byref(lv), C.byref(sps))

    assert ndt(src=None) == inv and ndt(ns=-1) == inv and ndt(res=-1.0) == inv and ndt(p=None) == inv
    assert score.value == 7.0 and pairs.value == -7 and (g == 7.0).all() and (H == 7.0).all()
    assert ndt(ns=0) == _lib.FLS_OK and score.value == 0.0 and pairs.value == 0 and lv.value == 0 and (g == 0.0).all() and (H == 0.0).all()
