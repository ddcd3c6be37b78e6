"""include/fls_debug_fit.h without a GPU: every declared symbol is exported and listed in DEBUG_FIT_SYMBOLS, the list shares nothing with the
other symbol lists, the header's own revision is 1 while FLS_ABI_REVISION and fls_debug_linalg.h stay what they were, invalid arguments are
refused before the device is looked at, and n == 0 is FLS_OK without a launch."""
import ctypes as C
import os
import re

import numpy as np

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP, UP = C.POINTER(C.c_double), C.POINTER(C.c_uint32)


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src))


def test_debug_fit_symbols_exported_declared_and_listed(built):
    L = _lib.lib()
    declared = _declared("fls_debug_fit.h")
    assert len(declared) == 10 and declared == set(_lib.DEBUG_FIT_SYMBOLS) and len(_lib.DEBUG_FIT_SYMBOLS) == 10
    for s in declared:
        assert hasattr(L, s), s
    src = open(os.path.join(ROOT, "include", "fls_debug_fit.h")).read()
    assert "#define FLS_DEBUG_FIT_REVISION 1" in src and L.fls_debug_fit_revision() == 1
    assert "#define FLS_DEBUG_TICKET_WORDS %d" % _lib.DEBUG_TICKET_WORDS in src
    others = (_lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.KEYFRAMES_SYMBOLS + _lib.DEBUG_LINALG_SYMBOLS + _lib.BATCH_SYMBOLS +
              _lib.BATCH_IVOX_SYMBOLS)
    assert not set(_lib.DEBUG_FIT_SYMBOLS) & set(others)
    # the -DFLS_FIT_MFMA=0 build carries the same hooks: the routines are compiled in both
    dpp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libfls_reg_dpp.so"))
    for s in declared:
        assert hasattr(dpp, s), s


def test_the_other_headers_are_untouched(built):
    L = _lib.lib()
    assert L.fls_abi_revision() == 9 and L.fls_abi_version() == 1 and L.fls_debug_linalg_revision() == 1
    assert "#define FLS_ABI_REVISION 9" in open(os.path.join(ROOT, "include", "fls_reg.h")).read()
    assert len(_declared("fls_debug_linalg.h")) == 6 and _declared("fls_debug_linalg.h") == set(_lib.DEBUG_LINALG_SYMBOLS)
    assert len(_lib.EXPORTED_SYMBOLS) == 44


def _p(a):
    return a.ctypes.data_as(DP)


def test_debug_fit_invalid_arguments_need_no_device(built):
    """every NULL pointer position and a negative n of every hook: FLS_ERR_INVALID here, where there is no device to look at; n == 0: FLS_OK"""
    L = _lib.lib()
    inv = _lib.FLS_ERR_INVALID
    a = np.zeros(64 * 18)
    u = np.zeros(_lib.DEBUG_TICKET_WORDS, np.uint32)
    up = u.ctypes.data_as(UP)

    def each_null(fn, head, ptrs, n, tail):
        """fn(*head, *ptrs[:k], n, *ptrs[k:]) with every pointer in turn NULL, then n < 0, then n == 0"""
        k = len(ptrs) - len(tail)
        for i in range(len(ptrs)):
            q = list(ptrs); q[i] = None
            assert fn(*head, *q[:k], n, *q[k:]) == inv, (fn.__name__, i)
        assert fn(*head, *ptrs[:k], -1, *ptrs[k:]) == inv, fn.__name__
        assert fn(*head, *ptrs[:k], 0, *ptrs[k:]) == _lib.FLS_OK, fn.__name__

    P = _p(a)
    for fn in (L.fls_debug_plane_residual, L.fls_debug_line_residual):
        each_null(fn, (0,), [P] * 8, 1, [P] * 3)
    each_null(L.fls_debug_icp_point_rows, (0,), [P] * 6, 1, [P] * 3)
    for fn in (L.fls_debug_rank1_mfma, L.fls_debug_rank1_dpp, L.fls_debug_rank1x3_mfma):
        each_null(fn, (0,), [P] * 4, 1, [P])
    for v in range(4):
        each_null(L.fls_debug_reduce_partials, (0, v), [P] * 2, 1, [P])
    assert L.fls_debug_reduce_partials(0, 4, P, 1, P) == inv and L.fls_debug_reduce_partials(0, -1, P, 1, P) == inv
    assert L.fls_debug_fanin(0, 1, 8, None, up, up) == inv and L.fls_debug_fanin(0, 1, 8, P, None, up) == inv and L.fls_debug_fanin(0, 1, 8, P, up, None) == inv
    assert L.fls_debug_fanin(0, 0, 8, P, up, up) == inv and L.fls_debug_fanin(0, -1, 8, P, up, up) == inv and L.fls_debug_fanin(0, 65536, 8, P, up, up) == inv
    assert L.fls_debug_fanin(0, 1, 0, P, up, up) == inv
    assert L.fls_debug_last_system(None, P, P) == inv
    assert (a == 0.0).all() and (u == 0).all()
