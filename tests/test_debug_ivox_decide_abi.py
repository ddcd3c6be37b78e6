"""include/fls_debug_ivox_decide.h without a GPU: the four declared symbols are exported by both libraries and listed in DEBUG_IVOX_DECIDE_SYMBOLS,
the list shares nothing with the other symbol lists, the header has a revision of its own while FLS_ABI_REVISION and the other headers stay what
they were, and the argument errors -- all of which are found before the device is looked at -- are refused with nothing written.  What the hooks
compute is in tests/test_ivox_decide_cases.py (the host rule) and tests/test_gpu_ivox_decide.py (the launches)."""
import ctypes as C
import os
import re

import numpy as np

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fls_[a-z_0-9]+)\s*\(", src))


def test_debug_ivox_decide_symbols_exported_declared_and_listed(built):
    L = _lib.lib()
    declared = _declared("fls_debug_ivox_decide.h")
    assert declared == set(_lib.DEBUG_IVOX_DECIDE_SYMBOLS) and len(_lib.DEBUG_IVOX_DECIDE_SYMBOLS) == 4
    dpp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libfls_reg_dpp.so"))
    for s in declared:
        assert hasattr(L, s) and hasattr(dpp, s), s
    src = open(os.path.join(ROOT, "include", "fls_debug_ivox_decide.h")).read()
    assert "#define FLS_DEBUG_IVOX_DECIDE_REVISION 1" in src and L.fls_debug_ivox_decide_revision() == 1
    assert "#define FLS_DEBUG_IVOX_DECIDE_FILL 0x%02X" % _lib.DEBUG_IVOX_DECIDE_FILL in src
    assert "#define FLS_DEBUG_IVOX_DECIDE_MAP_PAD %d" % _lib.DEBUG_IVOX_DECIDE_MAP_PAD in src
    assert C.sizeof(_lib.DebugIvoxGate) == 16 + 128
    others = (_lib.EXPORTED_SYMBOLS + _lib.PREPROCESS_SYMBOLS + _lib.FEATURES_DEVICE_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.KEYFRAMES_SYMBOLS + _lib.LOCALMAP_SYMBOLS +
              _lib.BATCH_SYMBOLS + _lib.BATCH_IVOX_SYMBOLS + _lib.DEBUG_LINALG_SYMBOLS + _lib.DEBUG_FIT_SYMBOLS + _lib.DEBUG_NDT_SYMBOLS + _lib.DEBUG_LOOP_SYMBOLS +
              _lib.LOOP_DEVICE_SYMBOLS + _lib.DEBUG_LOOP_LEAVES_SYMBOLS + _lib.DEBUG_KNN_SYMBOLS + _lib.DEBUG_IVOX_KNN_SYMBOLS + _lib.DEBUG_IVOX_UPDATE_SYMBOLS +
              _lib.NDT_IMAGE_SYMBOLS + _lib.KD_IMAGE_SYMBOLS + _lib.IVOX_BLOB_SYMBOLS + _lib.KNN_ORDER_SYMBOLS)
    assert not set(_lib.DEBUG_IVOX_DECIDE_SYMBOLS) & set(others)
    assert "fls_debug_ivox_decide.h" in open(os.path.join(ROOT, "funny_lidar_slam_amd", "csrc", "Makefile")).read()
    assert "fls_debug_ivox_decide.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hip = open(os.path.join(ROOT, "funny_lidar_slam_amd", "csrc", "fls_reg.hip")).read()
    assert re.search(r'#include "abi_debug_ivox_update\.hpp"[^\n]*\n#include "abi_debug_ivox_decide\.hpp"', hip)


def test_the_other_headers_are_untouched(built):
    L = _lib.lib()
    assert L.fls_abi_revision() == 9 and L.fls_abi_version() == 1 and L.fls_debug_ndt_revision() == 1 and L.fls_debug_ivox_knn_revision() == 1
    assert L.fls_debug_ivox_update_revision() == 1 and L.fls_debug_fit_revision() == 1 and L.fls_debug_knn_revision() == 1 and L.fls_debug_linalg_revision() == 1
    assert L.fls_debug_loop_revision() == 1 and L.fls_knn_order_revision() == 1 and L.fls_batch_ivox_revision() == 1
    assert "#define FLS_ABI_REVISION 9" in open(os.path.join(ROOT, "include", "fls_reg.h")).read()
    assert len(_lib.EXPORTED_SYMBOLS) == 44 and not _declared("fls_reg.h") & set(_lib.DEBUG_IVOX_DECIDE_SYMBOLS)
    assert _declared("fls_debug_ivox_update.h") == set(_lib.DEBUG_IVOX_UPDATE_SYMBOLS) and len(_lib.DEBUG_IVOX_UPDATE_SYMBOLS) == 2
    assert _declared("fls_debug_ivox_knn.h") == set(_lib.DEBUG_IVOX_KNN_SYMBOLS) and _declared("fls_debug_fit.h") == set(_lib.DEBUG_FIT_SYMBOLS)


class _Args:
    """a valid call of fls_debug_ivox_decide on four points, every output set to a canary"""

    def __init__(self):
        fp, bp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
        self.src = np.zeros((4, 3), np.float32)
        self.T = np.eye(4).reshape(-1)
        self.rows = np.full((4, 5, 4), 2.0, np.float32)
        self.cnt = np.array([0x85, 0x80, 0x81, 0x85], np.uint8)
        self.ids = np.zeros((4, 8), np.uint32)
        self.map = np.ones((8, 4), np.float32)
        self.sen = np.full(4, 9.0, np.float32)
        self.gate = _lib.DebugIvoxGate(1, 3, 50, 10, (C.c_double * 16)(*self.T))
        self.code = np.full(4, 77, np.uint8)
        self.pw = np.full((4, 4), 77.0, np.float32)
        self.lx, self.bt, self.st = np.full((4, 2), 77, np.uint32), np.full((1, 2), 77, np.uint32), np.full(2, 77, np.uint32)
        self.a = dict(device_id=0, src=self.src.ctypes.data_as(fp), n=4, T=self.T.ctypes.data_as(C.POINTER(C.c_double)), fs=0.5, rows=self.rows.ctypes.data_as(fp),
                      cnt=self.cnt.ctypes.data_as(bp), nn_n=4, ids=self.ids.ctypes.data_as(u32p), map=self.map.ctypes.data_as(fp), n_slots=8,
                      sen=self.sen.ctypes.data_as(fp), materialize=1, count=1, gate=C.byref(self.gate), code=self.code.ctypes.data_as(bp),
                      pw=self.pw.ctypes.data_as(fp), lx=self.lx.ctypes.data_as(u32p), bt=self.bt.ctypes.data_as(u32p), st=self.st.ctypes.data_as(u32p))

    def call(self, **kw):
        a = dict(self.a, **kw)
        return _lib.lib().fls_debug_ivox_decide(*[a[k] for k in ("device_id", "src", "n", "T", "fs", "rows", "cnt", "nn_n", "ids", "map", "n_slots", "sen", "materialize",
                                                                 "count", "gate", "code", "pw", "lx", "bt", "st")])

    def untouched(self):
        return ((self.code == 77).all() and (self.pw == 77.0).all() and (self.lx == 77).all() and (self.bt == 77).all() and (self.st == 77).all() and
                (self.rows == 2.0).all() and list(self.cnt) == [0x85, 0x80, 0x81, 0x85])


def test_invalid_arguments_need_no_device(built):
    """every refusal is decided from the arguments alone: FLS_ERR_INVALID here, where there is no device to look at (a device id that cannot exist is
    passed as well), and nothing is written"""
    inv = _lib.FLS_ERR_INVALID
    A = _Args()
    bad = [dict(n=-1), dict(nn_n=-1), dict(n_slots=-1), dict(materialize=2), dict(materialize=-1), dict(count=2), dict(src=None), dict(T=None), dict(sen=None),
           dict(code=None), dict(pw=None), dict(rows=None), dict(cnt=None), dict(map=None), dict(lx=None), dict(bt=None), dict(st=None),
           dict(count=0)]                           # a gate without counting: a launch that skips writes the status words
    for kw in bad:
        assert A.call(device_id=1 << 20, **kw) == inv and A.untouched(), kw
    assert A.call(device_id=1 << 20, n=0) == _lib.FLS_OK and A.untouched()  # nothing to decide: no launch, no device
    assert A.call(device_id=1 << 20, n=0, nn_n=0, rows=None, cnt=None, ids=None, map=None, n_slots=0, gate=None) == _lib.FLS_OK
    # nn_ids == NULL with a list in ids form (bit 7 clear, count non-zero); a count of 0 in ids form needs no ids
    A.cnt[2] = 0x01
    assert A.call(device_id=1 << 20, ids=None, gate=None) == inv
    A.cnt[2] = 0x81
    assert A.untouched()

    fp, bp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    L = _lib.lib()
    m = lambda **kw: L.fls_debug_ivox_nn_materialize(*[dict(dict(d=1 << 20, ids=A.a["ids"], cnt=A.a["cnt"], nn_n=4, map=A.a["map"], n_slots=8, sen=A.a["sen"],
                                                                 rows=A.a["rows"]), **kw)[k] for k in ("d", "ids", "cnt", "nn_n", "map", "n_slots", "sen", "rows")])
    for kw in (dict(nn_n=-1), dict(n_slots=-1), dict(ids=None), dict(cnt=None), dict(rows=None), dict(sen=None), dict(map=None)):
        assert m(**kw) == inv and A.untouched(), kw
    assert m(nn_n=0) == _lib.FLS_OK and A.untouched()

    nn3, cnt, code, pw = np.zeros((4, 5, 3), np.float32), np.full(4, 5, np.uint8), np.full(4, 77, np.uint8), np.full((4, 3), 77.0, np.float32)
    h = lambda **kw: L.fls_debug_ivox_decide_host(*[dict(dict(src=A.a["src"], T=A.a["T"], fs=0.5, nn=nn3.ctypes.data_as(fp), cnt=cnt.ctypes.data_as(bp), n=4,
                                                              code=code.ctypes.data_as(bp), pw=pw.ctypes.data_as(fp)), **kw)[k]
                                                    for k in ("src", "T", "fs", "nn", "cnt", "n", "code", "pw")])
    for kw in (dict(n=-1), dict(src=None), dict(T=None), dict(nn=None), dict(cnt=None), dict(code=None), dict(pw=None)):
        assert h(**kw) == inv and (code == 77).all() and (pw == 77.0).all(), kw
    assert h(n=0) == _lib.FLS_OK and (code == 77).all() and (pw == 77.0).all()
    assert h() == _lib.FLS_OK and (code == 0).all() and (pw == 0.0).all()  # (the valid call does write: five neighbours on the centre's side of the point)
