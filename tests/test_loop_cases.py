"""tests/loop_cases.py without a GPU: the numpy models that tests/test_gpu_loop_stages.py holds the device to reproduce the CPU oracle, and every
input reaches the branch it was made for -- by the oracle and numpy alone, so that the GPU test cannot pass by comparing with a wrong model or by
never entering a path."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import loop_cases as LC


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def _sorted_d2(cloud):
    c = np.asarray(cloud, np.float32)
    dx, dy, dz = (c[:, None, k] - c[None, :, k] for k in range(3))
    return np.sort((dx * dx + dy * dy) + dz * dz, axis=1)


def test_the_base_pair_is_the_documented_one():
    assert [len(a) for a in LC.filtered(0.6, 0.6)] == [4483, 5673] and [len(a) for a in LC.filtered(0.5, 0.4)] == [5311, 6367]
    assert max(LC.SIZES) <= 4483 and [-(-n // 256) for n in LC.SIZES] == [1, 1, 1, 2, 7, 8, 9, 18]


@pytest.mark.parametrize("xname", ["zero", "moved"])
def test_the_cost_models_reproduce_the_oracle(xname):
    """brute-force correspondences, numpy Mahalanobis matrices, the float transform of apply_state, the exact sums and f / g formed from them: the
    oracle's f, g and number of correspondences (its own kd-tree, covariances and sequential sums) to 1e-12"""
    s, t = LC.filtered(0.5, 0.4)
    cs, ct = LC.gicp_covs()
    x = np.zeros(6) if xname == "zero" else LC.X_MOVED
    corr = LC.corr_model(s, t, np.eye(4), 2.0)
    sums, mags, m = LC.fdf_model(s, t, x, corr, LC.mahal_model(corr, np.eye(3), cs, ct))
    f, g = LC.f_and_g(sums, x)
    fo, go, nc = O.gicp_fdf(s, t, np.eye(4), 2.0, x)
    assert nc == m == sums[13] > 5000
    assert f == pytest.approx(fo, rel=1e-12) and g == pytest.approx(go, rel=1e-12)
    assert (mags >= np.abs(sums)).all()


def test_apply_state_is_a_float_rigid_transform():
    T = LC.apply_state(LC.X_MOVED)
    assert T.dtype == np.float32 and np.array_equal(T[:3, 3], LC.X_MOVED[:3].astype(np.float32))
    R = T[:3, :3].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and np.abs(R - np.eye(3)).max() > 1e-3
    assert np.array_equal(LC.apply_state(np.zeros(6)), np.eye(4, dtype=np.float32))


def test_the_covariance_clouds_reach_their_branches():
    cell = 1.5
    # patch: most points certified by the 27-cell block, the rest by the 125-cell one (column 0 is the point itself)
    d20 = np.sqrt(_sorted_d2(LC.cov_cloud("patch"))[:, 20])
    assert 0.05 < (d20 > cell).mean() < 0.3 and (d20 < 2 * cell).all()
    # submap: a thin slice in voxel order, 20th neighbours from under one cell to beyond rho = 13
    d20 = np.sqrt(_sorted_d2(LC.cov_cloud("submap"))[:, 20])
    assert (d20 < cell).any() and (d20 > 4 * cell).mean() > 0.1 and (d20 > 13 * cell).any()
    # lattice: the 20th and the 21st neighbour at the same float distance for most points
    d = _sorted_d2(LC.cov_cloud("lattice"))
    assert (d[:, 19] == d[:, 20]).mean() > 0.5
    # crowded: one cell with more than kCovMaxCand = 1024 points
    c = LC.cov_cloud("crowded")
    key = np.floor(c.astype(np.float64) / cell).astype(int)
    assert (key[:1100] == 0).all() and (key == 0).all(axis=1).sum() > 1024
    # isolated: the 20 neighbours of the last two points lie beyond rho = 13 cells, inside a window that is larger still
    c = LC.cov_cloud("isolated")
    d20 = np.sqrt(_sorted_d2(c)[-2:, 20])
    assert (d20 > 13 * cell).all() and ((c.max(axis=0) - c.min(axis=0))[:2] > 30 * cell).all()
    assert len(LC.cov_cloud("20")) == 20 and len(LC.cov_cloud("21")) == 21
    for name in ("submap", "patch", "lattice", "crowded", "isolated", "20", "21"):
        Co, Cn, sep = LC.cov_reference(name)
        assert sep.mean() >= 0.6 and np.abs(np.linalg.eigvalsh(Co) - [0.001, 1.0, 1.0]).max() < 1e-9, name
        assert np.abs(Co - Cn)[sep].max() < 1e-4, name  # (the two references agree where they are compared)


def test_the_sparse_leaf_tables():
    """the sub-map with the three strays: sparse (over 32 Mi leaf cells) but without one displaced leaf; the scattered leaves: probe chains"""
    _, t = LC.filtered(0.6, 0.6)
    slots, displaced = LC.leaf_table_displaced(np.concatenate([t, LC.STRAY]), 2.0)
    assert (slots, displaced) == (4096, 0)
    s, tt, stray = LC.chained_leaves()
    assert len(O.ndt_leaves(tt, 3.0)[0]) == len(O.ndt_leaves(np.concatenate([tt, stray]), 3.0)[0]) == 497
    slots, displaced = LC.leaf_table_displaced(np.concatenate([tt, stray]), 3.0)
    assert slots == 1024 and displaced >= 50
    for cloud, res in ((np.concatenate([t, LC.STRAY]), 2.0), (np.concatenate([tt, stray]), 3.0)):
        inv = np.float32(1.0) / np.float32(res)
        div = np.floor(cloud.max(axis=0) * inv) - np.floor(cloud.min(axis=0) * inv) + 1
        assert (32 << 20) < np.prod(div.astype(np.float64)) < 2 ** 31, res  # sparse, and still a grid build_target accepts


def test_the_pair_count_of_the_oracle():
    """flo_ndt_derivatives_pairs: the sums of flo_ndt_derivatives, and a count that a permutation of the source leaves alone"""
    s, t = LC.filtered(0.6, 0.6)
    so, go, Ho = O.ndt_derivatives(s[:700], t, 3.0, LC.P_MOVED)
    s2, g2, H2, pairs = O.ndt_derivatives_pairs(s[:700], t, 3.0, LC.P_MOVED)
    assert so == s2 and np.array_equal(go, g2) and np.array_equal(Ho, H2) and pairs > 700
    assert O.ndt_derivatives_pairs(s[:700][::-1], t, 3.0, LC.P_MOVED)[3] == pairs
    assert O.ndt_derivatives_pairs(s[:1], t[:5], 3.0, LC.P_MOVED) == (0.0, pytest.approx(np.zeros(6)), pytest.approx(np.zeros((6, 6))), 0)
