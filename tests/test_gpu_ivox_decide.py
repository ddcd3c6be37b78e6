"""The iVox map-update decision launch itself -- ivox_add_decide_kernel<MATERIALIZE> and ivox_nn_materialize_kernel (csrc/kernels_ivox_coop.hpp), through
the launch functions the matcher uses (include/fls_debug_ivox_decide.h) -- on the constructed launches of tests/ivox_decide_cases.py.  The codes and
world points are the CPU oracle's (flo_ivox_add_decide, the function the oracle's AddCloud calls) on the rows each list resolves to; the lists after
the launch, the block-local counts, the block totals, the status words and the speculative gate are numpy's (ivox_decide_cases.expected).  Every
output is prefilled on the device, so what the kernel must not write is compared as well.  Nothing here has a tolerance: codes, rows, counts, lx, bt
and status are compared exactly, world points bit for bit (NaN where the oracle has NaN: x86 and the device produce NaNs of different sign)."""
import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, registration as reg
from oracle import oracle as O
from tests import ivox_decide_cases as D
from tests.test_ivox_decide_cases import same_points

pytestmark = pytest.mark.gpu

NAMES = list(D.launches())


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"
    assert D.FILL == _lib.DEBUG_IVOX_DECIDE_FILL and D.MAP_PAD == _lib.DEBUG_IVOX_DECIDE_MAP_PAD


@pytest.fixture(scope="module")
def want():
    """every launch's expected outputs, computed once and left unchanged"""
    out = {name: D.expected(l, O.ivox_add_decide) for name, l in D.launches().items()}
    for e in out.values():
        for a in e.values():
            a.setflags(write=False)
    return out


def _f32(words):
    return None if words is None else np.ascontiguousarray(words).view(np.float32)


def run(l):
    return reg.DebugIvoxDecide(l.src, l.T, l.fs, _f32(l.rows), l.cnt, nn_ids=l.ids, map_rows=_f32(l.map_rows), sentinel=D.SENTINEL,
                               materialize=bool(l.materialize), count=bool(l.count), gate=l.gate)


@pytest.mark.parametrize("name", NAMES)
def test_decision_launch(name, want):
    l, e = D.launches()[name], want[name]
    got = run(l)
    assert got["status"] == _lib.FLS_OK
    n = len(l.src)
    bad = np.flatnonzero(got["code"] != e["code"])
    assert bad.size == 0, (name, "codes", bad[:8], got["code"][bad[:8]], e["code"][bad[:8]], l.cnt[bad[:8][bad[:8] < len(l.cnt)]])
    assert same_points(got["pw"][:, :3], e["pw"][:, :3]) and np.array_equal(got["pw"][:, 3].view(np.uint32), e["pw"][:, 3].view(np.uint32)), (name, "world points")
    assert np.array_equal(got["cnt"], e["cnt"]), (name, "count bytes", np.flatnonzero(got["cnt"] != e["cnt"])[:8])
    rows = got["rows"].view(np.uint32).reshape(-1, 5, 4)
    assert np.array_equal(rows, e["rows"]), (name, "rows", np.flatnonzero((rows != e["rows"]).any(axis=(1, 2)))[:8])
    assert not (rows == D.SENTINEL.view(np.uint32)).all(axis=2).any(), (name, "a row read behind the slot bound")
    assert np.array_equal(got["lx"], e["lx"]), (name, "block-local counts", np.flatnonzero((got["lx"] != e["lx"]).any(axis=1))[:8])
    assert np.array_equal(got["bt"], e["bt"]), (name, "block totals", got["bt"], e["bt"])
    assert np.array_equal(got["st"], e["st"]), (name, "status words", got["st"], e["st"])
    if l.count and D.gate_runs(l.gate):  # (what the update chain relies on, said once more in words)
        assert list(got["st"]) == [0, 0] and int(got["bt"][:(n + 255) // 256].sum()) == int((e["code"] != 0).sum())
        assert (got["bt"][(n + 255) // 256:] == D.fill(1, np.uint32)[0]).all()


@pytest.mark.parametrize("name", [k for k in NAMES if D.launches()[k].ids is not None and D.launches()[k].materialize and D.launches()[k].gate is None])
def test_materialize_kernel(name):
    """ivox_nn_materialize_kernel on the same lists: what the decision launch leaves in its materializing form"""
    l = D.launches()[name]
    _, rows, cnt = D.materialized(l)
    rc, got_rows, got_cnt = reg.DebugIvoxNnMaterialize(l.ids, l.cnt, _f32(l.map_rows), _f32(l.rows), sentinel=D.SENTINEL)
    assert rc == _lib.FLS_OK
    assert np.array_equal(got_cnt, cnt), (name, np.flatnonzero(got_cnt != cnt)[:8])
    got = got_rows.view(np.uint32).reshape(-1, 5, 4)
    assert np.array_equal(got, rows), (name, np.flatnonzero((got != rows).any(axis=(1, 2)))[:8])
    assert not (got == D.SENTINEL.view(np.uint32)).all(axis=2).any()
    # a second pass finds every list in rows form and changes nothing
    rc, again_rows, again_cnt = reg.DebugIvoxNnMaterialize(l.ids, got_cnt, _f32(l.map_rows), got_rows, sentinel=D.SENTINEL)
    assert rc == _lib.FLS_OK and np.array_equal(again_cnt, cnt) and np.array_equal(again_rows.view(np.uint32).reshape(-1, 5, 4), rows)


def test_both_templates_decide_alike(want):
    """the two instantiations on the same mixed lists give the same codes, world points and counts (they differ in what they leave in the lists)"""
    for name in D.RULE_CASES:
        a, b = want[name + "/mixed/m0"], want[name + "/mixed/m1"]
        assert np.array_equal(a["code"], b["code"]) and np.array_equal(a["lx"], b["lx"]) and np.array_equal(a["bt"], b["bt"])
        assert np.array_equal(a["rows"], D.launches()[name + "/mixed/m0"].rows) and not np.array_equal(b["cnt"], D.launches()[name + "/mixed/m1"].cnt)
