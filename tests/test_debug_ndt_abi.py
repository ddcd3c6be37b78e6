"""include/fls_debug_ndt.h without a GPU: both declared symbols are exported and listed in DEBUG_NDT_SYMBOLS, the list shares nothing with the
other symbol lists, the header's own revision is 1 while FLS_ABI_REVISION and the symbol list of fls_reg.h stay what they were, and invalid
arguments are refused before the device is looked at."""
import ctypes as C
import os
import re

import numpy as np

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src))


def test_debug_ndt_symbols_exported_declared_and_listed(built):
    L = _lib.lib()
    declared = _declared("fls_debug_ndt.h")
    assert declared == set(_lib.DEBUG_NDT_SYMBOLS) and len(_lib.DEBUG_NDT_SYMBOLS) == 2
    for s in declared:
        assert hasattr(L, s), s
    src = open(os.path.join(ROOT, "include", "fls_debug_ndt.h")).read()
    assert "#define FLS_DEBUG_NDT_REVISION 1" in src and L.fls_debug_ndt_revision() == 1
    others = (_lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.KEYFRAMES_SYMBOLS + _lib.DEBUG_LINALG_SYMBOLS + _lib.DEBUG_FIT_SYMBOLS +
              _lib.BATCH_SYMBOLS + _lib.BATCH_IVOX_SYMBOLS)
    assert not set(_lib.DEBUG_NDT_SYMBOLS) & set(others)
    dpp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libfls_reg_dpp.so"))  # the -DFLS_FIT_MFMA=0 build carries the same read-out
    for s in declared:
        assert hasattr(dpp, s), s


def test_the_other_headers_are_untouched(built):
    L = _lib.lib()
    assert L.fls_abi_revision() == 9 and L.fls_abi_version() == 1 and L.fls_debug_fit_revision() == 1 and L.fls_debug_linalg_revision() == 1
    assert "#define FLS_ABI_REVISION 9" in open(os.path.join(ROOT, "include", "fls_reg.h")).read()
    assert len(_lib.EXPORTED_SYMBOLS) == 44 and not _declared("fls_reg.h") & set(_lib.DEBUG_NDT_SYMBOLS)
    assert len(_declared("fls_debug_fit.h")) == 10 and _declared("fls_debug_fit.h") == set(_lib.DEBUG_FIT_SYMBOLS)


def test_debug_ndt_invalid_arguments_need_no_device(built):
    """a NULL handle, a NULL count and, with cap > 0, every array in turn NULL: FLS_ERR_INVALID here, where there is no device to look at (the
    NULL handle is refused first, so the array checks are exercised through the order the entry point states: handle, count, kind, arrays)"""
    L = _lib.lib()
    inv = _lib.FLS_ERR_INVALID
    i32 = np.zeros(8 * 3, np.int32); u8 = np.zeros(8, np.uint8); f64 = np.zeros(8 * 9)
    ip, bp, dp = i32.ctypes.data_as(C.POINTER(C.c_int32)), u8.ctypes.data_as(C.POINTER(C.c_uint8)), f64.ctypes.data_as(C.POINTER(C.c_double))
    n = C.c_size_t(77)
    full = [ip, ip, ip, bp, bp, dp, dp, dp]
    assert L.fls_debug_ndt_voxels(None, 8, *full, C.byref(n)) == inv
    assert L.fls_debug_ndt_voxels(None, 0, *([None] * 8), C.byref(n)) == inv
    assert L.fls_debug_ndt_voxels(None, 8, *full, None) == inv
    for k in range(8):
        q = list(full); q[k] = None
        assert L.fls_debug_ndt_voxels(None, 8, *q, C.byref(n)) == inv, k
    assert n.value == 77 and not i32.any() and not u8.any() and not f64.any()
