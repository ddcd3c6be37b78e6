"""The five LOAM feature kernels (csrc/kernels_features.hpp) on the constructed frames of tests/feature_cases.py, against the oracle
(oracle/flo_features.h, ties in index order): the fourteen arrays of test_gpu_features.EXACT and both counts, compared as bytes.  There is no tie
budget and no tolerance.  tests/test_feature_cases.py shows, without a GPU, what every frame reaches: the 20-corner cap and its break, the
unsorted boundary element two sectors share, suppressions that stop at a column step of 11 and not at 10 at every offset on either side,
suppressions that clear candidates still ahead in the walk's 64-element chunk or the next one, whole sectors of tied roughness, roughness equal
to a threshold, sector lengths around the chunk and sort sizes up to the 4096-column ring, the flag rules at equality, the range gates at
equality, every column, a mismatched h_res, first-return-wins across thread blocks, a second raw layout.

Every frame runs on a fresh handle in both modes (arrays read back, arrays kept on the device and fetched by `get`), a sequence of frames runs
on one handle, and eight of refpin's seeded random frames run on the device as well."""
import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, features
from tests import feature_cases as FC
from tests import refpin
from tests.test_gpu_features import EXACT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"


def _handle(p, keep):
    return features.FeatureFrontEnd(p["horizontal_scan"], p["vertical_scan"], p["horizontal_resolution"], p["min_distance"], p["max_distance"],
                                    p["corner_thres"], p["planar_thres"], keep_on_device=keep)


def _oracle(raw, p):
    from oracle import oracle as O
    o = O.OracleFeatures(**p)
    n = o.Project(raw)
    o.ExtractFeatures()
    out = {k: o.get(k) for k in EXACT}
    out["n_ordered"] = n
    o.close()
    return out


def _where(o, name, k):
    """ordered index, ring and sector of element k of array `name`"""
    i = int(o[name][k]) if name in ("corner_idx", "planar_idx") else None
    if name in ("corner", "planar"):
        i = int(o[name + "_idx"][k])
    if name in ("row_start", "row_end"):
        return None, k, None
    i = k if i is None else i
    rs, re_ = o["row_start"].astype(int), o["row_end"].astype(int)
    ring = int(np.searchsorted(rs - 5, i, side="right") - 1)
    t = int((re_[ring] - rs[ring]) / 6)
    sector = min(max((i - rs[ring]) // t, 0), 5) if t > 0 else None
    return i, ring, sector


def _compare(g, n, counts, o, label, events=None):
    assert n == o["n_ordered"], (label, "n_ordered", n, o["n_ordered"])
    for name in EXACT:
        a, b = g.get(name), o[name]
        if a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)):
            continue
        m = min(len(a), len(b))
        diff = np.nonzero((a[:m] != b[:m]).reshape(m, -1).any(axis=1))[0]
        k = int(diff[0]) if len(diff) else m
        msg = f"{label}: {name} differs (device {a.shape}, oracle {b.shape}), {len(diff)} of {m} rows, first at {k}"
        if k < len(b):
            i, ring, sector = _where(o, name, k)
            msg += f": device {a[k].tolist() if k < len(a) else None} oracle {b[k].tolist()}, ordered index {i}, ring {ring}, sector {sector}"
            if events is not None and (ring, sector) in events:
                msg += f"; the model's events there: {events[(ring, sector)]}"
        raise AssertionError(msg)
    assert counts == (len(o["corner_idx"]), len(o["planar_idx"])), (label, counts)


def _run(f, o, keep, label, events=None, handle=None):
    g = handle if handle is not None else _handle(f.params, keep)
    n = g.project(f.raw)
    counts = g.extract()
    _compare(g, n, counts, o, label, events)
    if handle is None:
        g.close()


@pytest.mark.parametrize("keep", [False, True], ids=["host", "resident"])
@pytest.mark.parametrize("name", list(FC.FRAMES))
def test_constructed_frame(name, keep):
    f = FC.frame(name)
    o = FC.oracle_arrays(name)
    _run(f, o, keep, f"{name} keep_on_device={keep}", FC.modelled(name)[2])


@pytest.mark.parametrize("keep", [False, True], ids=["host", "resident"])
def test_one_handle_frame_after_frame(keep):
    """a fully occupied 4096-column frame, then 11 points (no extraction), then an empty cloud, then `cap`: every frame equals a fresh oracle, so
    nothing of an earlier frame (cell owners, flags, selection lists, counts) survives into the next"""
    p = FC.frame(FC.REUSE_ORDER[0]).params
    g = _handle(p, keep)
    for name in FC.REUSE_ORDER + FC.REUSE_ORDER[:2]:
        f = FC.frame(name)
        assert f.params == p
        _run(f, FC.oracle_arrays(name), keep, f"{name} on a reused handle, keep_on_device={keep}", FC.modelled(name)[2], handle=g)
    g.close()


@pytest.mark.parametrize("seed", FC.FUZZ_SEEDS)
def test_fuzz_frame(seed):
    """refpin's seeded random frames (either lidar model, other thresholds and range gates, up to nine returns in ten dropped)"""
    raw, p = refpin.make_feature_case(f"ffuzz{seed}")
    o = _oracle(raw, p)
    f = FC.Frame(raw, p, {})
    for keep in (False, True):
        _run(f, o, keep, f"ffuzz{seed} keep_on_device={keep}")
