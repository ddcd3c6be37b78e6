"""include/fls_batch.h without a GPU: every declared symbol is exported and listed, the header's own revision is 1 while the ABI revision and
the symbol list of fls_reg.h / fls_features.h stay what they were, invalid arguments are refused before the device is looked at, and an empty
batch is FLS_OK."""
import ctypes as C
import os
import re

import numpy as np

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP, DP, SP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_size_t)


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src))


def test_batch_symbols_exported_declared_and_listed(built):
    L = _lib.lib()
    declared = _declared("fls_batch.h")
    assert len(declared) == 3 and declared == set(_lib.BATCH_SYMBOLS)
    for s in declared:
        assert hasattr(L, s), s
    assert L.fls_batch_revision() == 1
    assert "#define FLS_BATCH_REVISION 1" in open(os.path.join(ROOT, "include", "fls_batch.h")).read()


def test_existing_abi_is_untouched(built):
    L = _lib.lib()
    assert L.fls_abi_revision() == 9 and L.fls_abi_version() == 1
    assert set(_lib.EXPORTED_SYMBOLS) == _declared("fls_reg.h") | _declared("fls_features.h")
    others = _lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.KEYFRAMES_SYMBOLS + _lib.DEBUG_LINALG_SYMBOLS + _lib.DEBUG_FIT_SYMBOLS
    assert not set(_lib.BATCH_SYMBOLS) & set(others)
    assert len(_lib.EXPORTED_SYMBOLS) == 44
    assert "#define FLS_ABI_REVISION 9" in open(os.path.join(ROOT, "include", "fls_reg.h")).read()


def test_batch_invalid_arguments_need_no_device(built):
    L = _lib.lib()
    inv = _lib.FLS_ERR_INVALID
    pts = np.zeros((16, 4), np.float32)
    src = (FP * 1)(pts.ctypes.data_as(FP))
    none_src = (FP * 1)()  # one NULL cloud
    n = (C.c_size_t * 1)(16)
    T = np.eye(4).reshape(-1).copy()
    Tp = T.ctypes.data_as(DP)
    st, status = (_lib.Stats * 1)(), (C.c_int32 * 1)(77)
    fake = C.c_void_p(1)  # never dereferenced: the argument checks below come first
    assert L.fls_match_batch_fused(None, 1, src, n, None, None, 4, Tp, st, status, 4) == inv
    assert L.fls_match_batch_fused(None, 0, None, None, None, None, 4, None, None, None, 4) == inv
    assert L.fls_match_batch_fused(fake, 1, None, n, None, None, 4, Tp, st, status, 4) == inv
    assert L.fls_match_batch_fused(fake, 1, src, None, None, None, 4, Tp, st, status, 4) == inv
    assert L.fls_match_batch_fused(fake, 1, src, n, None, None, 4, None, st, status, 4) == inv
    assert L.fls_match_batch_fused(fake, 1, src, n, None, None, 2, Tp, st, status, 4) == inv  # stride_floats < 3
    assert L.fls_match_batch_fused(fake, 1, src, n, src, None, 4, Tp, st, status, 4) == inv  # src1 without n1
    assert L.fls_match_batch_fused(fake, 1, src, n, None, n, 4, Tp, st, status, 4) == inv  # n1 without src1
    assert L.fls_match_batch_fused(fake, 1, none_src, n, None, None, 4, Tp, st, status, 4) == inv  # a NULL cloud with points
    assert status[0] == 77 and np.array_equal(T, np.eye(4).reshape(-1))  # nothing was written
    assert L.fls_batch_stat(None, 0) == 0 and L.fls_batch_stat(None, 3) == 0


def test_empty_batch_is_ok_without_a_device(built):
    L = _lib.lib()
    fake = C.c_void_p(1)  # an empty batch touches neither the handle nor the device
    assert L.fls_match_batch_fused(fake, 0, None, None, None, None, 4, None, None, None, 4) == _lib.FLS_OK
    assert L.fls_match_batch_fused(fake, 0, None, None, None, None, 3, None, None, None, 0) == _lib.FLS_OK
    assert L.fls_match_batch_fused(fake, 0, None, None, None, None, 2, None, None, None, 4) == _lib.FLS_ERR_INVALID
