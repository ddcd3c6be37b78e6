"""include/fls_debug_tail.h without a GPU: every declared symbol is exported and listed in DEBUG_TAIL_SYMBOLS, the list shares nothing with the
other symbol lists, the header's own revision is 1 while FLS_ABI_REVISION and fls_debug_fit.h stay what they were, the two structs have the
sizes the ctypes mirrors have, and invalid arguments are refused before the device is looked at, with nothing written."""
import ctypes as C
import os
import re

import numpy as np

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src))


def test_debug_tail_symbols_exported_declared_and_listed(built):
    L = _lib.lib()
    declared = _declared("fls_debug_tail.h")
    assert len(declared) == 3 and declared == set(_lib.DEBUG_TAIL_SYMBOLS) and len(_lib.DEBUG_TAIL_SYMBOLS) == 3
    for s in declared:
        assert hasattr(L, s), s
    src = open(os.path.join(ROOT, "include", "fls_debug_tail.h")).read()
    assert "#define FLS_DEBUG_TAIL_REVISION 1" in src and L.fls_debug_tail_revision() == 1
    assert "#define FLS_DEBUG_TAIL_MAX_ITER %d" % _lib.DEBUG_TAIL_MAX_ITER in src and "#define FLS_DEBUG_TAIL_MAX_ROWS %d" % _lib.DEBUG_TAIL_MAX_ROWS in src
    others = (_lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.KEYFRAMES_SYMBOLS + _lib.DEBUG_LINALG_SYMBOLS + _lib.DEBUG_FIT_SYMBOLS +
              _lib.BATCH_SYMBOLS + _lib.BATCH_IVOX_SYMBOLS + _lib.DEBUG_KNN_SYMBOLS + _lib.DEBUG_LOOP_SYMBOLS + _lib.DEBUG_IVOX_DECIDE_SYMBOLS)
    assert not set(_lib.DEBUG_TAIL_SYMBOLS) & set(others)
    # the -DFLS_FIT_MFMA=0 build carries the same hooks
    dpp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libfls_reg_dpp.so"))
    for s in declared:
        assert hasattr(dpp, s), s


def test_the_other_headers_are_untouched(built):
    L = _lib.lib()
    assert L.fls_abi_revision() == 9 and L.fls_abi_version() == 1 and L.fls_debug_fit_revision() == 1 and L.fls_debug_linalg_revision() == 1
    assert "#define FLS_ABI_REVISION 9" in open(os.path.join(ROOT, "include", "fls_reg.h")).read()
    assert "#define FLS_DEBUG_FIT_REVISION 1" in open(os.path.join(ROOT, "include", "fls_debug_fit.h")).read()
    assert len(_lib.DEBUG_FIT_SYMBOLS) == 10 and len(_lib.EXPORTED_SYMBOLS) == 44


def test_struct_mirrors(built):
    """GnState: 68 doubles, 6 ints, 16 stamps, the three logs; Mailbox: 24 doubles, 5 ints, seq (the library pins both against the device structs
    field by field at compile time)"""
    assert C.sizeof(_lib.DebugGnState) == 68 * 8 + 6 * 4 + 16 * 8 + 64 * (16 * 8 + 8 + 4) == 9656
    assert C.sizeof(_lib.DebugMailbox) == 24 * 8 + 6 * 4 == 216
    assert _lib.DebugGnState.iter.offset == 544 and _lib.DebugGnState.dbg.offset == 568 and _lib.DebugGnState.log_T.offset == 696
    assert _lib.DebugGnState.log_res.offset == 696 + 8192 and _lib.DebugGnState.log_nv.offset == 696 + 8192 + 512
    assert _lib.DebugMailbox.sum_res.offset == 128 and _lib.DebugMailbox.last_dx.offset == 144 and _lib.DebugMailbox.iter.offset == 192
    assert _lib.DebugMailbox.seq.offset == 212
    src = open(os.path.join(ROOT, "include", "fls_debug_tail.h")).read()
    for cls, name in ((_lib.DebugGnState, "fls_debug_gn_state"), (_lib.DebugMailbox, "fls_debug_mailbox")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
        fields = [f.strip().split("[")[0] for decl in re.findall(r"(?:double|int32_t|uint32_t|int64_t)\s+([^;]+);", body) for f in decl.split(",")]
        assert fields == [f[0] for f in cls._fields_], (name, fields)


def test_debug_tail_invalid_arguments_need_no_device(built):
    L = _lib.lib()
    inv = _lib.FLS_ERR_INVALID
    T0 = np.eye(4).reshape(-1)
    rows = np.ones((4, 32))
    st = np.full(C.sizeof(_lib.DebugGnState), 0xA5, np.uint8)
    mb = np.full(C.sizeof(_lib.DebugMailbox), 0x5A, np.uint8)
    P, R, S, M = T0.ctypes.data_as(DP), rows.ctypes.data_as(DP), st.ctypes.data, mb.ctypes.data
    top = _lib.DEBUG_TAIL_MAX_ROWS

    def loam(variant=0, T=P, state=S, ra=R, na=4, rb=R, nb=4, mbox=M):
        return L.fls_debug_loam_tail(0, variant, 1, T, state, ra, na, rb, nb, 1.0, 1.0, 0, mbox)

    def lu(variant=0, T=P, state=S, r=R, n=4, mode=0, mbox=M):
        return L.fls_debug_lu_tail(0, variant, 1, T, state, r, n, mode, 1.0, 1.0, 0, 0, mbox)

    for kw in (dict(T=None), dict(state=None), dict(rb=None), dict(ra=None), dict(variant=-1), dict(variant=3), dict(nb=0), dict(nb=-1), dict(nb=top + 1),
               dict(na=-1), dict(na=top + 1), dict(ra=None, na=0, nb=0), dict(ra=None, na=0, rb=None), dict(mbox=None, variant=7)):
        assert loam(**kw) == inv, kw
    for kw in (dict(T=None), dict(state=None), dict(r=None), dict(variant=-1), dict(variant=3), dict(n=0), dict(n=-1), dict(n=top + 1), dict(mode=-1),
               dict(mode=2), dict(mbox=None, mode=5)):
        assert lu(**kw) == inv, kw
    assert (st == 0xA5).all() and (mb == 0x5A).all() and (rows == 1.0).all()
