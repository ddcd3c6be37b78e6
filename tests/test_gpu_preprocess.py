"""GPU: the per-scan preprocessing of include/fls_preprocess.h (IMU de-skew, range gate, subsample, planar VoxelGrid) and the LoamFull
projection with de-skew, against the test model (tests/host/deskew_model.cpp) bit for bit, plus physical and end-to-end checks."""
import ctypes as C

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib, features, preprocess, registration as reg, synth
from tests import deskew_util as du
from tests.test_oracle_features import VELO64

pytestmark = pytest.mark.gpu

MIN_D, MAX_D, SPAN, LEAF = 4.0, 100.0, 6, 0.5  # config_nclt: lidar_use_min_dist_ / max_dist_ / point_jump_span / planar leaf
STAMP = du.STAMP_US


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"


@pytest.fixture(scope="module")
def scan():
    static, moving, T_gt = du.raw_scan(0)
    t, q = du.imu_for()
    return dict(static=static, raw=moving, T_gt=T_gt, t=t, q=q)


def exact_filter(planar, leaf):
    pts = np.ascontiguousarray(planar, dtype=np.float32)
    out = np.zeros((max(pts.shape[0], 1), 4), np.float32)
    n = C.c_size_t()
    rc = _lib.lib().fls_voxel_grid_cloud(0, 0, pts.ctypes.data_as(C.POINTER(C.c_float)), pts.shape[0], 4, np.float32(leaf),
                                         out.ctypes.data_as(C.POINTER(C.c_float)), out.shape[0], C.byref(n))
    assert rc == _lib.FLS_OK
    return out[:n.value]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_against_model(raw, t, q, T, span=SPAN, leaf=LEAF, stamp=STAMP):
    pre = preprocess.ScanPreprocessor(MIN_D, MAX_D, span, leaf, T)
    out = pre.scan(raw, stamp, t, q)
    m = du.preprocess(raw, stamp, t, q, T, MIN_D, MAX_D, span)
    assert out.imu_status == preprocess.IMU_STATUS[m["status"]]
    assert same_bits(out.ordered, m["ordered"]), "ordered"
    assert same_bits(out.ordered_index, m["ordered_index"]), "ordered_index"
    assert same_bits(out.planar, m["planar"]), "planar"
    if leaf > 0 and m["planar"].shape[0]:
        assert same_bits(out.planar_filtered, exact_filter(m["planar"], leaf)), "planar_filtered"
    if m["status"] == 0:
        st, sq = du.segment(t, q, m["start"], m["end"])
        assert np.array_equal(pre.get("segment_t"), st) and same_bits(pre.get("segment_q"), sq)
        assert (out.cloud_start_us, out.cloud_end_us) == (m["start"], m["end"])
    return out, m, pre


@pytest.mark.parametrize("T", [du.T_NCLT, du.T_GENERAL], ids=["nclt", "general"])
def test_bit_identical_to_model(scan, T):
    out, m, _ = check_against_model(scan["raw"], scan["t"], scan["q"], T)
    assert out.imu_status == "ok" and out.ordered.shape[0] > 100_000 and out.planar_filtered.shape[0] > 1000
    assert out.filter_on_device  # the device VoxelGrid took this cloud


@pytest.mark.parametrize("span", [1, 7])
def test_jump_spans_and_range_edges(scan, span):
    raw = scan["raw"].copy()
    edge = np.arange(5, 4000, 97)
    raw["x"][edge], raw["y"][edge], raw["z"][edge] = 0.0, 0.0, 0.0
    raw["x"][edge[0::3]] = MIN_D                      # depth exactly min: kept
    raw["y"][edge[1::3]] = MAX_D                      # depth exactly max: kept
    raw["z"][edge[2::3]] = np.nextafter(np.float32(MIN_D), np.float32(0))  # just inside the gate's lower edge: dropped
    out, m, _ = check_against_model(raw, scan["t"], scan["q"], du.T_NCLT, span=span)
    kept = set(out.ordered_index.tolist())
    assert all(int(k) in kept for k in edge[0::3]) and all(int(k) in kept for k in edge[1::3]) and not any(int(k) in kept for k in edge[2::3])


def test_superset_imu_and_empty_cloud(scan):
    a, _, _ = check_against_model(scan["raw"], scan["t"], scan["q"], du.T_NCLT)
    t2, q2 = du.imu_for(before_us=2_000_000, after_us=3_000_000)
    b, _, _ = check_against_model(scan["raw"], t2, q2, du.T_NCLT)
    for k in ("ordered", "ordered_index", "planar", "planar_filtered"):
        assert same_bits(getattr(a, k), getattr(b, k)), k
    e, _, _ = check_against_model(scan["raw"][:0], scan["t"], scan["q"], du.T_NCLT)
    assert e.status == _lib.FLS_OK and e.imu_status == "empty_cloud" and e.ordered.shape[0] == 0 and e.planar_filtered.shape[0] == 0


def test_imu_status_cases(scan):
    pre = preprocess.ScanPreprocessor(MIN_D, MAX_D, SPAN, LEAF, du.T_NCLT)
    raw, t, q = scan["raw"], scan["t"], scan["q"]
    late = pre.scan(raw, STAMP, t[5:], q[5:])       # oldest sample after the cloud start
    early = pre.scan(raw, STAMP, t[:-8], q[:-8])    # newest sample before the cloud end
    flat = raw.copy()
    flat["time"] = 0.0
    empty = pre.scan(flat, STAMP, t, q)             # start == end
    assert (late.status, late.imu_status) == (_lib.FLS_ERR_STATE, "drop")
    assert (early.status, early.imu_status) == (_lib.FLS_ERR_STATE, "wait")
    assert (empty.status, empty.imu_status) == (_lib.FLS_OK, "empty_segment")
    for o in (late, early, empty):
        assert o.ordered.shape[0] == o.planar.shape[0] == o.planar_filtered.shape[0] == 0


def test_invalid_inputs(scan):
    pre = preprocess.ScanPreprocessor(MIN_D, MAX_D, SPAN, LEAF, du.T_NCLT)
    raw, t, q = scan["raw"][:1000], scan["t"], scan["q"]
    bad_t = t.copy()
    bad_t[7] = bad_t[6]
    nan_time = raw.copy()
    nan_time["time"][3] = np.nan
    for args in ((raw, t[:1], q[:1]), (raw, bad_t, q), (nan_time, t, q)):
        with pytest.raises(_lib.FlsError) as e:
            pre.scan(args[0], STAMP, args[1], args[2])
        assert e.value.status == _lib.FLS_ERR_INVALID


def test_removes_the_sweep_rotation(scan):
    """Points measured under a known rotation R(t) come back to the header-stamp frame within the nlerp error of the 200 Hz trace."""
    out, _, _ = check_against_model(scan["raw"], scan["t"], scan["q"], np.eye(4), span=1, leaf=0.0)
    truth = scan["static"][out.ordered_index]
    p_true = np.stack([truth["x"], truth["y"], truth["z"]], -1).astype(np.float64)
    err = np.linalg.norm(out.ordered[:, :3] - p_true, axis=1)
    # bound: worst angle between the nlerp of two neighbouring samples of the segment the call used (its two ends are slerps) and the
    # true orientation, on a fine grid of each interval, plus one microsecond of rotation (point times are truncated to us), times the
    # range, plus the float rounding of both clouds
    seg_t, seg_q = du.segment(scan["t"], scan["q"], out.cloud_start_us, out.cloud_end_us)
    ts = (seg_t.astype(np.int64) - STAMP) * 1e-6
    r = np.linspace(0.0, 1.0, 201)
    worst = 0.0
    for k in range(ts.size - 1):
        qn = seg_q[k][None, :] * (1 - r)[:, None] + seg_q[k + 1][None, :] * r[:, None]
        qn /= np.linalg.norm(qn, axis=1, keepdims=True)
        qt = synth.imu_orientation(ts[k] + r * (ts[k + 1] - ts[k]))
        worst = max(worst, float(np.max(2 * np.arccos(np.clip(np.abs(np.sum(qn * qt, axis=1)), 0, 1)))))
    rng_ = np.linalg.norm(p_true, axis=1)
    bound = rng_ * (1.1 * worst + np.deg2rad(120.0) * 1e-6) + 4 * np.spacing(rng_.astype(np.float32)).astype(np.float64) + 1e-6
    assert np.all(err <= bound), float(np.max(err - bound))
    raw_err = np.linalg.norm(np.stack([scan["raw"]["x"], scan["raw"]["y"], scan["raw"]["z"]], -1)[out.ordered_index] - p_true, axis=1)
    assert raw_err.max() > 100 * err.max()  # without the de-skew the sweep is visibly distorted


def _front():
    return features.FeatureFrontEnd(1800, 64, VELO64["horizontal_resolution"], MIN_D, MAX_D, 1.0, 0.1)


FEAT_ALL = ["ordered", "depth", "col", "row_start", "row_end", "raw_index", "roughness", "valid_pre", "valid_post", "is_corner", "corner_idx",
            "planar_idx", "corner", "planar"]


def test_loam_project_deskew_identity_equals_project(scan):
    raw = scan["raw"]
    q_id = np.tile([0.0, 0.0, 0.0, 1.0], (scan["t"].size, 1))
    a, b = _front(), _front()
    n_a = a.project(raw)
    a.extract()
    n_b, st = b.project_deskew(raw, STAMP, scan["t"], q_id, np.eye(4))
    b.extract()
    assert st == "ok" and n_a == n_b > 50_000
    for name in FEAT_ALL:
        assert same_bits(a.get(name), b.get(name)), name


def test_loam_project_deskew_with_motion(scan):
    raw = scan["raw"]
    a, b = _front(), _front()
    a.project(raw)
    a.extract()
    n_b, st = b.project_deskew(raw, STAMP, scan["t"], scan["q"], du.T_GENERAL)
    b.extract()
    assert st == "ok"
    for name in ["depth", "col", "row_start", "row_end", "raw_index", "roughness", "valid_pre", "valid_post", "is_corner", "corner_idx", "planar_idx"]:
        assert same_bits(a.get(name), b.get(name)), name
    m = du.preprocess(raw, STAMP, scan["t"], scan["q"], du.T_GENERAL, MIN_D, MAX_D, 1, want_all=True)["deskew_all"]
    ri = b.get("raw_index")
    assert np.all(m[ri, 3] == 1.0)
    expect = np.concatenate([m[ri, :3], raw["intensity"][ri, None]], 1).astype(np.float32)
    assert same_bits(b.get("ordered"), expect)
    assert same_bits(b.get("corner"), expect[b.get("corner_idx")]) and same_bits(b.get("planar"), expect[b.get("planar_idx")])
    # every ProcessPoint fails on an empty segment (all point times 0): no point claims a cell
    flat = raw.copy()
    flat["time"] = 0.0
    c = _front()
    assert c.project_deskew(flat, STAMP, scan["t"], scan["q"], du.T_GENERAL) == (0, "empty_segment")
    assert c.extract() == (0, 0)


def test_end_to_end_match_is_closer_with_deskew(scan):
    cfg = synth.make_config(1, scale=0.3)
    y = reg.YAML_NCLT_IVOX

    def match(planar):
        m = reg.make_matcher("PointToPlane_IVOX", y)
        m.AddCloudToLocalMap([cfg["map"]])
        T = np.eye(4)
        m.Match(reg.PointcloudCluster(planar_cloud_=np.ascontiguousarray(planar[:, :3])), T, update_map=False)
        return synth.pose_error(T, scan["T_gt"])

    with_deskew = preprocess.ScanPreprocessor(MIN_D, MAX_D, SPAN, LEAF).scan(scan["raw"], STAMP, scan["t"], scan["q"])
    q_id = np.tile([0.0, 0.0, 0.0, 1.0], (scan["t"].size, 1))
    without = preprocess.ScanPreprocessor(MIN_D, MAX_D, SPAN, LEAF).scan(scan["raw"], STAMP, scan["t"], q_id)
    dt_a, dr_a = match(with_deskew.planar_filtered)
    dt_b, dr_b = match(without.planar_filtered)
    assert dr_a < dr_b and dt_a + 0.5 * dr_a < dt_b + 0.5 * dr_b, ((dt_a, dr_a), (dt_b, dr_b))
