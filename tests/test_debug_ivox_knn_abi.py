"""include/fls_debug_ivox_knn.h without a GPU: every declared symbol is exported by both libraries and listed in DEBUG_IVOX_KNN_SYMBOLS, the list
shares nothing with the other symbol lists, the header has a revision of its own, the limits are what the kernel's resource bounds allow, and a NULL
pointer is refused with nothing written."""
import ctypes as C
import os
import re

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_debug_ivox_knn_symbols_exported_declared_and_listed(built):
    L = _lib.lib()
    src = open(os.path.join(ROOT, "include", "fls_debug_ivox_knn.h")).read()
    declared = set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    assert declared == set(_lib.DEBUG_IVOX_KNN_SYMBOLS) and len(_lib.DEBUG_IVOX_KNN_SYMBOLS) == 2
    dpp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libfls_reg_dpp.so"))
    for s in declared:
        assert hasattr(L, s) and hasattr(dpp, s), s
    assert "#define FLS_DEBUG_IVOX_KNN_REVISION 1" in src and L.fls_debug_ivox_knn_revision() == 1
    others = (_lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.KEYFRAMES_SYMBOLS + _lib.LOCALMAP_SYMBOLS + _lib.BATCH_SYMBOLS +
              _lib.BATCH_IVOX_SYMBOLS + _lib.DEBUG_LINALG_SYMBOLS + _lib.DEBUG_FIT_SYMBOLS + _lib.DEBUG_NDT_SYMBOLS + _lib.DEBUG_LOOP_SYMBOLS + _lib.DEBUG_KNN_SYMBOLS +
              _lib.NDT_IMAGE_SYMBOLS + _lib.KD_IMAGE_SYMBOLS + _lib.IVOX_BLOB_SYMBOLS)
    assert not set(_lib.DEBUG_IVOX_KNN_SYMBOLS) & set(others)
    assert "fls_debug_ivox_knn.h" in open(os.path.join(ROOT, "funny_lidar_slam_amd", "csrc", "Makefile")).read()


def test_limits_and_null_pointers(built):
    L = _lib.lib()
    r, c = C.c_int(-7), C.c_int(-7)
    assert L.fls_debug_ivox_knn_limits(None, C.byref(c)) == _lib.FLS_ERR_INVALID and L.fls_debug_ivox_knn_limits(C.byref(r), None) == _lib.FLS_ERR_INVALID
    assert (r.value, c.value) == (-7, -7)
    assert L.fls_debug_ivox_knn_limits(C.byref(r), C.byref(c)) == _lib.FLS_OK
    # one probe pass of 64 lanes holds 19 lanes per run; four staged rows per lane; 16 bytes per staged row, 20,480 bytes of LDS per workgroup of four waves
    assert 1 <= r.value and 19 * r.value <= 64 and 1 <= c.value <= 4 * 64 and 4 * 16 * c.value <= 20480
