"""include/fls_knn_order.h without a device: the symbols and the revision, the statuses that are decided before a handle is looked at, the
per-query limit W, and the two counter slots in include/fls_reg.h."""
import ctypes as C
import os

from funny_lidar_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_revision():
    L = _lib.lib()
    for s in _lib.KNN_ORDER_SYMBOLS:
        assert hasattr(L, s), s
    assert L.fls_knn_order_revision() == 1
    hdr = open(os.path.join(ROOT, "include", "fls_knn_order.h")).read()
    assert "#define FLS_KNN_ORDER_REVISION 1" in hdr and "#define FLS_KNN_ORDER_DEFAULT 0" in hdr and "#define FLS_KNN_ORDER_REFERENCE 1" in hdr
    for s in _lib.KNN_ORDER_SYMBOLS:
        assert s + "(" in hdr, s
    assert L.fls_abi_revision() == 9  # fls_reg.h's own revision has not moved


def test_null_and_unknown_mode_statuses():
    L = _lib.lib()
    mode = C.c_int(7)
    assert L.fls_set_knn_order(None, _lib.KNN_ORDER_DEFAULT) == _lib.FLS_ERR_INVALID
    assert L.fls_set_knn_order(None, _lib.KNN_ORDER_REFERENCE) == _lib.FLS_ERR_INVALID
    assert L.fls_set_knn_order(None, 2) == _lib.FLS_ERR_INVALID
    assert L.fls_set_knn_order(None, -1) == _lib.FLS_ERR_INVALID
    assert L.fls_get_knn_order(None, C.byref(mode)) == _lib.FLS_ERR_INVALID and mode.value == 7
    assert L.fls_get_knn_order(None, None) == _lib.FLS_ERR_INVALID
    assert L.fls_knn_order_limits(None) == _lib.FLS_ERR_INVALID


def test_limit_is_at_least_256():
    w = _lib.knn_order_limit()
    assert w >= 256
    src = open(os.path.join(ROOT, "funny_lidar_slam_amd", "csrc", "knn_reference_order.hpp")).read()
    assert f"constexpr int kWork = {w};" in src  # a compile-time constant of the selection's own header


def test_counter_slots_are_documented():
    doc = open(os.path.join(ROOT, "include", "fls_reg.h")).read()
    for slot in ("177 = ", "178 = "):
        assert slot in doc, slot
    assert "fls_knn_order.h" in doc and "#define FLS_ABI_REVISION 9" in doc
