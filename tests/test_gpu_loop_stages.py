"""The loop-closure kernels one stage at a time (include/fls_debug_loop.h): ndt_p2d_kernel, gicp_cov_kernel, gicp_corr_kernel, gicp_fdf_kernel,
loop_fitness_kernel and the shared loop_block_reduce, launched by the hooks on fls_loop_match's own LoopMatcher, against the CPU oracle's pieces
(flo_ndt_derivatives, flo_ndt_leaves, flo_gicp_covariances, flo_gicp_fdf) and numpy models of the discrete parts.  tests/test_gpu_loop.py only
sees these kernels through the pose of a whole Match (1e-4 m, 2 mm when the GICP traces part ways); here every discrete result must be equal and
every sum is held to a bound that comes from the reference or from the arithmetic, never from the device (see each test).  Inputs:
tests/loop_cases.py, at most a few thousand points.

Figures measured at commit 35e4517 plus this change (CPU: oracle and numpy only; device: MI355X) are quoted in the docstrings below."""
import numpy as np
import pytest

from funny_lidar_slam_amd import _lib
from oracle import oracle as O
from tests import loop_cases as LC

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built):
    assert _lib.device_count() >= 1, "gpu tests need an MI355X (gfx950): the HIP path has no CPU fallback"


# ========================================================================================================================================
# NDT sums
# ========================================================================================================================================
# The oracle's own summation-order spread: largest deviation, per array, of flo_ndt_derivatives over 8 random permutations of the 4483-point
# source cloud (numpy default_rng(5)) from the unpermuted result, for the 5673-point target.  (resolution, pose): (score, gradient, Hessian).
# Magnitudes for orientation: score 1e4 .. 8e4, largest gradient entry 1.7e5 .. 4.3e5, largest Hessian entry 1.5e7 .. 2.7e7, i.e. the spreads
# are ~1e-14 of the largest entry.
NDT_SPREAD = {
    (10.0, "moved"): (6.26e-10, 1.28e-09, 8.38e-08), (10.0, "zero"): (3.49e-10, 1.34e-09, 5.96e-08),
    (3.0, "moved"): (1.02e-10, 2.10e-09, 1.60e-07), (3.0, "zero"): (2.55e-10, 3.09e-09, 1.83e-07),
    (2.0, "moved"): (4.00e-11, 6.98e-10, 1.15e-07), (2.0, "zero"): (5.64e-11, 1.22e-09, 1.08e-07),
}
NDT_FACTOR = 16.0  # the device's fixed tree is one more order, and its exp differs from glibc's by an ulp per term
POSES = {"moved": LC.P_MOVED, "zero": np.zeros(6)}  # "zero" takes the |angle| < 1e-4 branch of angle_derivatives


def _ndt_bounds(res, pose):
    return tuple(NDT_FACTOR * s for s in NDT_SPREAD[(res, pose)])


def _same_ndt(a, b):
    return (a["score"] == b["score"] and a["pairs"] == b["pairs"] and a["leaves"] == b["leaves"] and np.array_equal(a["grad"], b["grad"]) and
            np.array_equal(a["hess"], b["hess"]))


def _check_ndt(src, tgt, res, pose, label):
    """hook against the oracle: leaves and pairs equal, sums within 16 x the oracle's permutation spread; Hessian off: the same score and pairs
    bit for bit, the gradient within its bound.  Returns the with-Hessian result."""
    bs, bg, bh = _ndt_bounds(res, pose)
    p = POSES[pose]
    so, go, Ho, pairs = O.ndt_derivatives_pairs(src, tgt, res, p)
    r = LC.ndt(src, tgt, res, p, True)
    r0 = LC.ndt(src, tgt, res, p, False)
    ds, dg, dh = abs(r["score"] - so), np.abs(r["grad"] - go).max(), np.abs(r["hess"] - Ho).max()
    print(f"{label}: res {res} {pose}: {len(src)} points, {r['leaves']} leaves, {r['pairs']} pairs; device - oracle: score {ds:.2e} (bound {bs:.2e}), "
          f"gradient {dg:.2e} ({bg:.2e}), Hessian {dh:.2e} ({bh:.2e})")
    assert r["leaves"] == len(O.ndt_leaves(tgt, res)[0]) == r0["leaves"], label
    assert r["pairs"] == pairs, (label, r["pairs"], pairs)
    assert ds <= bs and dg <= bg and dh <= bh, (label, ds, dg, dh)
    assert r0["score"] == r["score"] and r0["pairs"] == r["pairs"], (label, "Hessian off / on")
    assert np.abs(r0["grad"] - go).max() <= bg, label
    assert (r0["hess"] == 7.0).all(), "without the Hessian the hook leaves hess alone"
    return r


@pytest.mark.parametrize("pose", ["moved", "zero"])
@pytest.mark.parametrize("res", [10.0, 3.0, 2.0])
def test_ndt_sums_equal_the_oracle(res, pose):
    """4483 source points against the 5673-point target's leaves (83 / 236 / 311 at 10 / 3 / 2 m; 17098, 10566, 8180 pairs at the moved pose).
    Bounds = 16 x NDT_SPREAD, e.g. at 3 m, moved: score 1.6e-9 of 2.3e4, gradient 3.4e-8 of 4.3e5, Hessian 2.6e-6 of 2.1e7.
    Observed device - oracle on an MI355X, largest over the six cases: score 7.6e-11, gradient 1.5e-9, Hessian 1.6e-7 (3 m, zero pose) -- at most
    0.06 of the bound, i.e. inside the oracle's own spread."""
    s, t = LC.filtered(0.6, 0.6)
    _check_ndt(s, t, res, pose, "full cloud")


@pytest.mark.parametrize("n", LC.SIZES)
def test_ndt_size_ladder_is_exact_in_rows_and_repeatable(n):
    """prefixes of the source cloud: 1, 7, 8, 9 and 18 partial rows -- the 8-wide trips and the tail of loop_block_reduce -- with a last row of
    1, 255, 256 or 5 points.  Against the oracle on the same prefix with the full cloud's bounds (a prefix sums fewer terms); twice in a row and
    once more after another size: bit-identical (a ticket or sequence word left dirty shows here)."""
    s, t = LC.filtered(0.6, 0.6)
    assert n <= len(s)
    a = _check_ndt(s[:n], t, 3.0, "moved", f"prefix {n}")
    b = LC.ndt(s[:n], t, 3.0, LC.P_MOVED, True)
    other = LC.ndt(s[:LC.SIZES[(LC.SIZES.index(n) + 3) % len(LC.SIZES)]], t, 3.0, LC.P_MOVED, True)
    c = LC.ndt(s[:n], t, 3.0, LC.P_MOVED, True)
    assert _same_ndt(a, b) and _same_ndt(a, c), n
    assert not _same_ndt(a, other)


def test_ndt_sparse_leaf_table_gives_the_dense_sums_bit_for_bit():
    """three stray points kilometres away push the 2 m leaf grid over 32 Mi cells: build_target keeps {cell, row} pairs in an open-addressing table
    (311 leaves in 1024 slots: probe chains form).  The strays form no leaf and the sum order is unchanged, so everything equals the dense run."""
    s, t = LC.filtered(0.6, 0.6)
    dense = LC.ndt(s, t, 2.0, LC.P_MOVED, True)
    sparse = LC.ndt(s, np.concatenate([t, LC.STRAY]), 2.0, LC.P_MOVED, True)
    assert dense["sparse"] == 0 and sparse["sparse"] == 1
    assert dense["leaves"] == sparse["leaves"] == len(O.ndt_leaves(t, 2.0)[0])
    assert _same_ndt(dense, sparse)
    assert _same_ndt(dense, LC.ndt(s, t, 2.0, LC.P_MOVED, True)), "the dense table after the sparse one"


def test_ndt_sparse_leaf_table_with_probe_chains():
    """497 scattered leaves in the 1024 slots of the sparse table: 120 of them sit behind another one's slot (the model of the table counts them), so
    the probe sequence of ndt_leaf_row is walked.  Leaves and pairs equal the oracle's, everything equals the dense run without the strays bit for
    bit.  (The sub-map's 311 leaves land in 4096 slots without a single collision: the case above never probes twice.)"""
    s, t, stray = LC.chained_leaves()
    p = np.zeros(6)
    slots, displaced = LC.leaf_table_displaced(np.concatenate([t, stray]), 3.0)
    assert slots == 1024 and displaced >= 50, (slots, displaced)
    dense = LC.ndt(s, t, 3.0, p, True)
    sparse = LC.ndt(s, np.concatenate([t, stray]), 3.0, p, True)
    assert dense["sparse"] == 0 and sparse["sparse"] == 1
    so, go, Ho, pairs = O.ndt_derivatives_pairs(s, t, 3.0, p)
    assert dense["leaves"] == sparse["leaves"] == len(O.ndt_leaves(t, 3.0)[0]) == 497
    assert dense["pairs"] == sparse["pairs"] == pairs and pairs > 1000, (dense["pairs"], sparse["pairs"], pairs)
    assert _same_ndt(dense, sparse)
    # the oracle's permutation spread on this cloud (8 permutations, as NDT_SPREAD): score 5.46e-12 of 3.2e3, gradient 2.18e-11 of 4.0e3,
    # Hessian 3.54e-08 of 2.1e7; the device is allowed 16 x that
    ds, dg, dh = abs(sparse["score"] - so), np.abs(sparse["grad"] - go).max(), np.abs(sparse["hess"] - Ho).max()
    assert ds <= NDT_FACTOR * 5.46e-12 and dg <= NDT_FACTOR * 2.18e-11 and dh <= NDT_FACTOR * 3.54e-08, (ds, dg, dh)
    print(f"sparse table: {slots} slots, {displaced} of 497 leaves displaced, {pairs} pairs; device - oracle: score {ds:.2e}, gradient {dg:.2e}, Hessian {dh:.2e}")


@pytest.mark.parametrize("res", [3.0, 2.0])
def test_ndt_source_points_outside_the_target_bounds(res):
    """a copy of the source 10 km away (contributes nothing) and points within one leaf of each face of the target's bounding box, inside and
    outside: the bounds checks of the 27-leaf walk.  pairs and sums equal the oracle's (the full cloud's bounds: the same terms and a few more)."""
    s, t = LC.filtered(0.6, 0.6)
    rng = np.random.default_rng(31)
    mn, mx = t.min(axis=0), t.max(axis=0)
    extra = []
    for a in range(3):
        for side in (0, 1):
            q = t[rng.integers(0, len(t), 40)].astype(np.float64)
            off = rng.uniform(-1.0, 1.0, 40) * res  # up to one leaf inside (-) or outside (+) the face
            q[:, a] = mn[a] - off if side == 0 else mx[a] + off
            extra.append(q)
    far = s.astype(np.float64) + [10000.0, 0.0, 0.0]
    src = np.concatenate([s, far] + extra).astype(np.float32)  # (p = 0: the transform is the identity, the faces are where the points are)
    r = _check_ndt(src, t, res, "zero", "outside")
    inside = _check_ndt(s, t, res, "zero", "inside only")
    assert r["pairs"] >= inside["pairs"]


def test_ndt_target_without_a_leaf_of_six_points():
    """5 points in each 3 m cell: no leaf Gaussian, FLS_OK with leaves = 0 and zero sums (and the next ordinary call is unaffected)"""
    rng = np.random.default_rng(7)
    cells = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    t = (cells[:, None, :] * 3.0 + rng.uniform(0.2, 2.8, (len(cells), 5, 3))).reshape(-1, 3).astype(np.float32)
    s = rng.uniform(0.0, 12.0, (300, 3)).astype(np.float32)
    assert len(O.ndt_leaves(t, 3.0)[0]) == 0
    for hess in (True, False):
        r = LC.ndt(s, t, 3.0, LC.P_MOVED, hess)
        assert r["leaves"] == 0 and r["pairs"] == 0 and r["score"] == 0.0 and (r["grad"] == 0.0).all()
        assert (r["hess"] == (0.0 if hess else 7.0)).all()
    fs, ft = LC.filtered(0.6, 0.6)
    _check_ndt(fs[:257], ft, 3.0, "moved", "after the empty target")


# ========================================================================================================================================
# GICP covariances
# ========================================================================================================================================
@pytest.mark.parametrize("name", ["submap", "patch", "lattice", "crowded", "isolated", "20", "21"])
def test_gicp_covariances_equal_the_oracle(name):
    """gicp_cov_kernel against flo_gicp_covariances (kd-tree, ties by (d2, index) like the device's rank keys), entry by entry for the points whose
    20-NN covariance has a separated normal (S1 - S2 > 1e-3 S0 in a float64 numpy SVD of the brute-force neighbours); symmetric with eigenvalues
    (0.001, 1, 1) to 1e-9 for the rest.  Bound: 4 x the largest |C_oracle - C_numpy| over the compared points of the case -- the reference against
    an independent float64 evaluation of the same neighbours, computed here on the CPU.  Measured (points, compared share, that figure):
        submap    1500  100 %   9.9e-07     first 1500 points of the 0.5 m source cloud (voxel order: a thin slice, 20th neighbours 1 .. 50 m away)
        patch     1500  100 %   1.3e-06     the 1500 points around its middle: the 27-cell block certifies 85 %, the 125-cell block the rest
        lattice    576   65.3 % 3.3e-14     12 x 12 x 4 at 0.25 m: exact distance ties at the 20th / 21st neighbour throughout
        crowded   1400  100 %   1.4e-05     1100 points in one 1.5 m cell + 300 over +-6 m: total > kCovMaxCand, lane 0's serial knn_grid<20>
        isolated   402  100 %   4.1e-07     a slab + two points 50 - 60 m away: rho 4, 6, 9, 13 .. to the `whole` exit
        20, 21      20 / 21  100 %  5.3e-10 / 7.8e-10    the smallest clouds run() launches on: every point's neighbours are the whole cloud
    Device and oracle share the float products, the neighbour order and the Jacobi SVD under -ffp-contract=off: the observed device - oracle maximum
    on an MI355X is 0.0 in every case, over all points (equal bits).  The device build of the cloud's grid and the host build give the same bits."""
    c = LC.cov_cloud(name)
    Co, Cn, sep = LC.cov_reference(name)
    assert sep.mean() >= 0.6, (name, sep.mean())  # (a broken mask cannot hide a failure)
    ref_dev = np.abs(Co - Cn)[sep].max()
    bound = 4.0 * ref_dev
    Cd = LC.gicp_cov(c, 1.5, 0.001, 0)
    Ch = LC.gicp_cov(c, 1.5, 0.001, 1)
    assert np.array_equal(Cd, Ch), (name, "device-built and host-built grid")
    assert np.isfinite(Cd).all()
    got = np.abs(Cd - Co)[sep].max()
    print(f"covariances {name}: {len(c)} points, {100 * sep.mean():.1f} % compared, |C_oracle - C_numpy| max {ref_dev:.2e}, bound {bound:.2e}, device - oracle max {got:.2e} "
          f"(all points {np.abs(Cd - Co).max():.2e})")
    assert got <= bound, (name, got, bound)
    rest = Cd[~sep]
    if len(rest):
        assert np.abs(rest - rest.transpose(0, 2, 1)).max() <= 1e-9
        assert np.abs(np.linalg.eigvalsh(rest) - [0.001, 1.0, 1.0]).max() <= 1e-9


# ========================================================================================================================================
# correspondences and Mahalanobis matrices
# ========================================================================================================================================
def _check_corr(moved, tgt, T, R, cs, ct, corr_dist, host_grid, label):
    """ids equal to the brute-force model; (C2 + R C1 R^T)^-1 within 1e-11 max|M| per matrix (C1, C2 have eigenvalues in [1e-3, 1]: condition
    <= 1e3, times 2^-52, times ~50 for the adjugate's operations); unmatched rows keep the hook's NaN.  Observed on an MI355X: at most 1.6e-13
    of max|M| (the base pair at the small pose)."""
    corr, M = LC.gicp_corr(moved, tgt, T, R, cs, ct, corr_dist, host_grid)
    want = LC.corr_model(moved, tgt, T, corr_dist)
    assert np.array_equal(corr, want), (label, np.flatnonzero(corr != want)[:10])
    Mr = LC.mahal_model(want, R, cs, ct)
    k = want >= 0
    assert np.isnan(M[~k]).all(), label
    worst = 0.0
    if k.any():
        scale = np.abs(Mr[k]).max(axis=(1, 2))
        rel = np.abs(M[k] - Mr[k]).max(axis=(1, 2)) / scale
        worst = rel.max()
        assert worst <= 1e-11, (label, worst)
    print(f"correspondences {label}: {len(corr)} points, {int(k.sum())} matched, Mahalanobis device - numpy max {worst:.2e} of max|M| (bound 1e-11)")
    return corr, M


@pytest.fixture(scope="module")
def verified():
    """the GICP pair at T = identity, R = identity, corr_dist 2: correspondences and matrices checked here, then fed to the cost-sum tests"""
    s, t = LC.filtered(0.5, 0.4)
    cs, ct = LC.gicp_covs()
    corr, M = _check_corr(s, t, np.eye(4), np.eye(3), cs, ct, 2.0, 0, "base pair, identity")
    assert (corr >= 0).sum() > 1000
    corr.setflags(write=False); M.setflags(write=False)
    return corr, M


def test_corr_base_pair_at_identity_and_at_a_small_pose(verified):
    s, t = LC.filtered(0.5, 0.4)
    cs, ct = LC.gicp_covs()
    T = LC.apply_state(LC.X_MOVED)
    R = T[:3, :3].astype(np.float64)
    assert not np.array_equal(R, np.eye(3))
    corr, _ = _check_corr(s, t, T, R, cs, ct, 2.0, 0, "base pair, small pose")
    assert not np.array_equal(corr, verified[0])
    ch, Mh = LC.gicp_corr(s, t, np.eye(4), np.eye(3), cs, ct, 2.0, 1)
    assert np.array_equal(ch, verified[0]) and np.array_equal(Mh, verified[1], equal_nan=True), "host-built target grid"


@pytest.mark.parametrize("ns", [1, 63, 64, 65])
def test_corr_partial_and_full_waves(ns):
    s, t = LC.filtered(0.5, 0.4)
    cs, ct = LC.gicp_covs()
    _check_corr(s[:ns], t, np.eye(4), np.eye(3), cs[:ns], ct, 2.0, 0, f"{ns} points")


def test_corr_gate_is_strict_and_ties_go_to_the_lower_index():
    cs, ct = LC.gicp_covs()
    o = np.zeros((1, 3), np.float32)
    at = np.array([[2.0, 0.0, 0.0]], np.float32)
    corr, _ = _check_corr(o, at, np.eye(4), np.eye(3), cs[:1], ct[:1], 2.0, 0, "target at exactly corr_dist")
    assert corr[0] == -1  # d2 == 4.0f is not < corr_dist^2
    inside = np.array([[np.nextafter(np.float32(2.0), np.float32(0.0)), 0.0, 0.0]], np.float32)
    corr, _ = _check_corr(o, inside, np.eye(4), np.eye(3), cs[:1], ct[:1], 2.0, 0, "target one float ulp inside")
    assert corr[0] == 0
    # equidistant targets in different cells: index 1 sits in a ring-1 cell and is seen after index 2 and 3 of the query's own cell
    tie = np.array([[5.0, 5.0, 5.0], [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], np.float32)
    for hg in (0, 1):
        corr, _ = _check_corr(o, tie, np.eye(4), np.eye(3), cs[:1], ct[:4], 2.0, hg, "three targets at distance 1")
        assert corr[0] == 1
    corr, _ = _check_corr(o, tie[::-1].copy(), np.eye(4), np.eye(3), cs[:1], ct[:4], 2.0, 0, "the same, reversed")
    assert corr[0] == 0


def _far_queries(t, step):
    """a coarse lattice over the target's bounding box grown by 12 m: queries beside, above and below the window on all six sides, in its voids,
    and next to points; nearest targets from centimetres to beyond corr_dist = 20"""
    mn, mx = t.min(axis=0) - 12.0, t.max(axis=0) + 12.0
    ax = [np.arange(mn[a], mx[a] + step, step) for a in range(3)]
    q = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3) + 0.37
    return q.astype(np.float32)


@pytest.mark.parametrize("form", ["window", "hash"])
def test_corr_far_queries_walk_rings_or_the_hash_table(form):
    """corr_dist = 20 m (13.3 cells): queries whose nearest target is farther than kMaxRing = 4 cells (6 m) walk the rings 5 .. of the dense window,
    from inside and from outside it on each of the six sides.  "hash": one stray target 1.7 km away makes the window too large for either build, so
    knn_scan_cell probes the hash table and the unfinished searches end in the brute-force scan.  Ids and matrices equal the models, and
    the device-built and the host-built grid give the same bits."""
    _, t = LC.filtered(0.5, 0.4)
    cs, ct = LC.gicp_covs()
    q = _far_queries(t, 4.0 if form == "window" else 6.0)
    if form == "hash":
        t = np.concatenate([t, np.array([[1000.0, 1000.0, 1000.0]], np.float32)])
        ct = np.concatenate([ct, ct[:1]])
    c1 = cs[np.arange(len(q)) % len(cs)]
    _, d2 = LC.nearest(q, t)
    d = np.sqrt(d2.astype(np.float64))
    mn, mx = t[:len(t) - (form == "hash")].min(axis=0), t[:len(t) - (form == "hash")].max(axis=0)
    beyond = (d > 6.5) & (d < 19.5)
    for a in range(3):  # ring walks from outside the window, on each side, that end in a match
        assert (beyond & (q[:, a] < mn[a] - 1.5)).any() and (beyond & (q[:, a] > mx[a] + 1.5)).any(), a
    assert (beyond & (q > mn).all(axis=1) & (q < mx).all(axis=1)).any(), "a void inside the window"
    assert (d > 20.5).any() and (d < 1.0).any()
    c0, M0 = _check_corr(q, t, np.eye(4), np.eye(3), c1, ct, 20.0, 0, f"{form}, far queries")
    ch, Mh = LC.gicp_corr(q, t, np.eye(4), np.eye(3), c1, ct, 20.0, 1)
    assert np.array_equal(c0, ch) and np.array_equal(M0, Mh, equal_nan=True)


# ========================================================================================================================================
# cost and gradient sums
# ========================================================================================================================================
def _check_fdf(moved, tgt, x, corr, M, label):
    """the reduced row against the exact sum of the kernel's own terms: |error| <= 2 (m - 1) 2^-53 sum|term| per column for ANY summation order
    (the terms are bit-identical: float transform with the c0 x + (c1 y + (c2 z + c3)) association, float residual, the kernel's products in
    float64); the count is exact.  Without the gradient: the same f sum and count bit for bit.  Observed on an MI355X: at most 0.004 of the
    bound (257 points), under 0.001 from 1792 points on."""
    v = LC.gicp_fdf(moved, tgt, x, corr, M, True)
    sums, mags, m = LC.fdf_model(moved, tgt, x, corr, M)
    assert v[13] == m, (label, v[13], m)
    bound = 2.0 * max(m - 1, 0) * U * mags
    err = np.abs(v - sums)
    assert (err[:13] <= bound[:13]).all(), (label, err, bound)
    v2 = LC.gicp_fdf(moved, tgt, x, corr, M, False)
    assert v2[0] == v[0] and v2[1] == v[13], label
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"cost sums {label}: {len(moved)} points, m = {m}, error / bound per column max {np.nanmax(np.where(bound > 0, err / bound, 0.0)):.3f}")
    return v


@pytest.mark.parametrize("xname", ["zero", "moved"])
@pytest.mark.parametrize("n", LC.SIZES)
def test_fdf_size_ladder(verified, n, xname):
    s, t = LC.filtered(0.5, 0.4)
    corr, M = verified
    x = np.zeros(6) if xname == "zero" else LC.X_MOVED
    a = _check_fdf(s[:n], t, x, corr[:n], M[:n], f"prefix {n}, x {xname}")
    k = LC.SIZES[(LC.SIZES.index(n) + 3) % len(LC.SIZES)]
    LC.gicp_fdf(s[:k], t, x, corr[:k], M[:k], True)
    assert np.array_equal(a, LC.gicp_fdf(s[:n], t, x, corr[:n], M[:n], True)), "repeat after another size"


@pytest.mark.parametrize("xname", ["zero", "moved"])
def test_fdf_full_pair_gives_the_oracles_f_and_g(verified, xname):
    """f = v0 / m and g as LoopMatcher::gicp_fdf forms them from the hook's sums, against flo_gicp_fdf on the unmodified pair (guess = identity,
    its own kd-tree correspondences and covariances): rel 1e-9"""
    s, t = LC.filtered(0.5, 0.4)
    corr, M = verified
    x = np.zeros(6) if xname == "zero" else LC.X_MOVED
    v = _check_fdf(s, t, x, corr, M, f"full pair, x {xname}")
    f, g = LC.f_and_g(v, x)
    fo, go, nc = O.gicp_fdf(s, t, np.eye(4), 2.0, x)
    print(f"f {f!r} oracle {fo!r}; g - oracle relative {np.abs(g / go - 1).max():.2e}")
    assert nc == v[13] == (corr >= 0).sum()
    assert f == pytest.approx(fo, rel=1e-9)
    assert g == pytest.approx(go, rel=1e-9)


def test_fdf_without_correspondences_and_with_one_in_the_last_lane(verified):
    s, t = LC.filtered(0.5, 0.4)
    corr, M = verified
    n = 17 * 256 + 5
    none = np.full(n, -1, np.int32)
    for grad in (True, False):
        v = LC.gicp_fdf(s[:n], t, LC.X_MOVED, none, M[:n], grad)
        assert (v == 0.0).all(), v
    k = np.flatnonzero(corr[:n] >= 0)[-1]
    last = none[:k + 1].copy()
    last[k] = corr[k]  # the only correspondence: the last point of the last block
    v = _check_fdf(s[:k + 1], t, LC.X_MOVED, last, M[:k + 1], "one correspondence, last lane")
    sums, _, m = LC.fdf_model(s[:k + 1], t, LC.X_MOVED, last, M[:k + 1])
    assert m == 1 and np.array_equal(v, sums), "a single term is not rounded by any sum"


# ========================================================================================================================================
# fitness
# ========================================================================================================================================
def _check_fitness(src, tgt, T, host_grid, label):
    """sum of the float nearest squared distances (numpy brute force) added in float64: non-negative terms, so any order is within
    ns 2^-53 sum; every point finds a neighbour (the search is un-gated).  Observed on an MI355X: the sums equal numpy's to the bit."""
    total, count = LC.fitness(src, tgt, T, host_grid)
    _, d2 = LC.nearest(LC.xform(T, src), tgt)
    want = float(np.sum(d2.astype(np.float64)))
    assert count == len(src), (label, count)
    assert abs(total - want) <= len(src) * U * want, (label, total, want)
    print(f"fitness {label}: {len(src)} points, sum {total!r}, model {want!r}, bound {len(src) * U * want:.2e}")
    return total


def test_fitness_base_pair_small_sizes_and_a_far_source():
    s, t = LC.filtered(0.5, 0.4)
    a = _check_fitness(s, t, np.eye(4), 0, "base pair")
    assert _check_fitness(s, t, np.eye(4), 1, "base pair, host grid") == a
    for n in (1, 257):
        _check_fitness(s[:n], t, np.eye(4), 0, f"{n} points")
    far = np.eye(4)
    far[:3, 3] = [300.0, 20.0, -5.0]  # 200 cells from the window: rings until the shell has crossed it
    b = _check_fitness(s[:1024], t, far, 0, "source 300 m away")
    assert _check_fitness(s[:1024], t, far, 1, "source 300 m away, host grid") == b
    assert _check_fitness(s, t, np.eye(4), 0, "base pair again") == a
