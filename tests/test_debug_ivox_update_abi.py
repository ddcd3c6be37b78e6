"""include/fls_debug_ivox_update.h without a GPU: both declared symbols are exported by both libraries and listed in DEBUG_IVOX_UPDATE_SYMBOLS, the
list shares nothing with the other symbol lists, the header has a revision of its own while FLS_ABI_REVISION and fls_reg.h's symbols stay what they
were, and the argument errors that need no handle are refused with nothing written.  The errors that need a handle -- another kind, a code above 2
on a live handle, a replica, a localization-mode handle, a handle without its first cloud -- are in tests/test_gpu_ivox_update.py: no handle exists
without a device."""
import ctypes as C
import os
import re

import numpy as np

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src))


def test_debug_ivox_update_symbols_exported_declared_and_listed(built):
    L = _lib.lib()
    declared = _declared("fls_debug_ivox_update.h")
    assert declared == set(_lib.DEBUG_IVOX_UPDATE_SYMBOLS) and len(_lib.DEBUG_IVOX_UPDATE_SYMBOLS) == 2
    dpp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libfls_reg_dpp.so"))
    for s in declared:
        assert hasattr(L, s) and hasattr(dpp, s), s
    src = open(os.path.join(ROOT, "include", "fls_debug_ivox_update.h")).read()
    assert "#define FLS_DEBUG_IVOX_UPDATE_REVISION 1" in src and L.fls_debug_ivox_update_revision() == 1
    others = (_lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.FEATURES_DEVICE_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.KEYFRAMES_SYMBOLS + _lib.LOCALMAP_SYMBOLS +
              _lib.BATCH_SYMBOLS + _lib.BATCH_IVOX_SYMBOLS + _lib.DEBUG_LINALG_SYMBOLS + _lib.DEBUG_FIT_SYMBOLS + _lib.DEBUG_NDT_SYMBOLS + _lib.DEBUG_LOOP_SYMBOLS +
              _lib.DEBUG_KNN_SYMBOLS + _lib.DEBUG_IVOX_KNN_SYMBOLS + _lib.NDT_IMAGE_SYMBOLS + _lib.KD_IMAGE_SYMBOLS + _lib.IVOX_BLOB_SYMBOLS + _lib.KNN_ORDER_SYMBOLS)
    assert not set(_lib.DEBUG_IVOX_UPDATE_SYMBOLS) & set(others)
    assert "fls_debug_ivox_update.h" in open(os.path.join(ROOT, "funny_lidar_slam_amd", "csrc", "Makefile")).read()
    assert "fls_debug_ivox_update.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_other_headers_are_untouched(built):
    L = _lib.lib()
    assert L.fls_abi_revision() == 9 and L.fls_abi_version() == 1 and L.fls_debug_ndt_revision() == 1 and L.fls_debug_ivox_knn_revision() == 1
    assert "#define FLS_ABI_REVISION 9" in open(os.path.join(ROOT, "include", "fls_reg.h")).read()
    assert len(_lib.EXPORTED_SYMBOLS) == 44 and not _declared("fls_reg.h") & set(_lib.DEBUG_IVOX_UPDATE_SYMBOLS)
    assert _declared("fls_debug_ivox_knn.h") == set(_lib.DEBUG_IVOX_KNN_SYMBOLS) and _declared("fls_debug_ndt.h") == set(_lib.DEBUG_NDT_SYMBOLS)


def test_invalid_arguments_need_no_device(built):
    """a NULL handle, whatever the other arguments are: FLS_ERR_INVALID here, where there is no device to look at, and nothing is written"""
    L = _lib.lib()
    inv = _lib.FLS_ERR_INVALID
    xyz = np.zeros((4, 3), np.float32)
    code = np.array([1, 2, 0, 1], np.uint8)
    fp, bp = xyz.ctypes.data_as(C.POINTER(C.c_float)), code.ctypes.data_as(C.POINTER(C.c_uint8))
    st = C.c_uint32(77)
    assert L.fls_debug_ivox_add_points(None, fp, bp, 4, C.byref(st)) == inv
    assert L.fls_debug_ivox_add_points(None, None, None, 0, C.byref(st)) == inv
    assert L.fls_debug_ivox_add_points(None, None, bp, 4, C.byref(st)) == inv and L.fls_debug_ivox_add_points(None, fp, None, 4, C.byref(st)) == inv
    assert L.fls_debug_ivox_add_points(None, fp, bp, 4, None) == inv
    code[2] = 3
    assert L.fls_debug_ivox_add_points(None, fp, bp, 4, C.byref(st)) == inv
    assert st.value == 77
