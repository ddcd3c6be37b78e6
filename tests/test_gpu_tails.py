"""The Gauss-Newton tails, each launch on its own: loam_tail (csrc/kernels_p2plane.hpp) and lu_tail (csrc/kernels_knn.hpp) in every instantiation
that ships -- <1024, false> as the product kernels gn_solve_loam_kernel / gn_solve_lu_kernel themselves, <256, true> and <512, true> as the fused
launches call them -- through the hooks of include/fls_debug_tail.h, one workgroup per launch, on the cases of tests/tail_cases.py (what they
reach: tests/test_tail_cases.py).  Every word of the returned GnState and mailbox is compared with the model:

  * H, g, sum_res(2), n_valid(2), iter, done, converged, the log slots, every mailbox word, and every byte the tail must not write (dbg, pad,
    unwritten log slots, last_rot / last_pos under lu_tail, converged under loam_tail, last_dx of a skipped update): bit for bit.
  * last_dx with the exact-solver bit: bit for bit the oracle solver's.  On the default path: within 64 cond(H) 2.2e-16 max|x| of it where the
    LDL^T fast path may accept (the bound tests/test_gpu_solver.py holds), and bit for bit where it must decline (singular, indefinite,
    rank-deficient, zero systems).
  * the pose, from the device's own last_dx: translation bit for bit; rotation within (24 (1 + theta) + 3) EPS per entry of
    LC.mat3_mul_model on O.so3_exp (tail_cases.rotation_bound); bit for bit where the step is exactly zero.
  * stop decisions on the default path in two passes: the first launch gives the device's step, the thresholds (and the carried norms of the
    LOAM family's second rule) are then placed at the model norm of THAT step and one double beside it, and the launch is repeated.  The
    reference is the rule applied to the device's step, never the device's flag.

Measured on an MI355X (printed by every run): DESIGN.md, "The Gauss-Newton tails, branch by branch"."""
import ctypes as C
import time

import numpy as np
import pytest

from funny_lidar_slam_amd import _lib
from tests import tail_cases as TC

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
VARIANTS = {0: "product kernels, 1024 threads", 1: "<256, true>", 2: "<512, true>"}


def _dp(a):
    return None if a is None else a.ctypes.data_as(DP)


def _launch(case, variant, first, T0, st_in, mb_in, rot_thr, pos_thr, word):
    st = st_in.copy()
    mb = None if mb_in is None else mb_in.copy()
    T0 = np.ascontiguousarray(T0, dtype=np.float64)
    L = _lib.lib()
    mbp = None if mb is None else mb.ctypes.data
    if case.tail == "loam":
        rc = L.fls_debug_loam_tail(0, variant, first, _dp(T0), st.ctypes.data, _dp(case.rows_a), 0 if case.rows_a is None else case.rows_a.shape[0],
                                   _dp(case.rows_b), case.rows_b.shape[0], rot_thr, pos_thr, word, mbp)
    else:
        rc = L.fls_debug_lu_tail(0, variant, first, _dp(T0), st.ctypes.data, _dp(case.rows_b), case.rows_b.shape[0], case.mode, rot_thr, pos_thr,
                                 case.min_eff, word, mbp)
    return rc, st, mb


def _one_launch(case, variant, exact, state, first, acc):
    """-> (the returned state, the differing words)"""
    word = case.word(exact)
    st_in, mb_in, rt, pt, ref_st, ref_mb, info = TC.run_model(case, exact=exact, state=state, first=first)
    rc, got_st, got_mb = _launch(case, variant, first, case.T0, st_in, mb_in, rt, pt, word)
    if rc != 0:
        return got_st, ["the hook returned %d (%s)" % (rc, _lib.status_string(rc))]
    if info["kind"] == "step":
        dx_dev = got_st[0]["last_dx"].copy()
        if exact or case.fast == "decline":
            if dx_dev.tobytes() != info["dx"].tobytes():
                return got_st, ["last_dx (oracle solver %r, device %r)" % (info["dx"].tolist(), dx_dev.tolist())]
        else:
            bound = 64.0 * np.linalg.cond(info["H"]) * 2.2e-16 * np.abs(info["dx"]).max()
            err = float(np.abs(dx_dev - info["dx"]).max()) if np.isfinite(dx_dev).all() else np.inf
            if not err <= bound:
                return got_st, ["last_dx (fast path: %.3e from the exact solver's, bound %.3e)" % (err, bound)]
            acc["fast"] = max(acc["fast"], err / bound if bound > 0 else 0.0)
            acc["fast_moved"] += int(dx_dev.tobytes() != info["dx"].tobytes())
            # second pass: the same edges at the device's own step
            st_in, mb_in, rt, pt, ref_st, ref_mb, info = TC.run_model(case, exact=exact, dx=dx_dev, state=state, first=first)
            if case.relative:
                rc, got_st, got_mb = _launch(case, variant, first, case.T0, st_in, mb_in, rt, pt, word)
                acc["second_pass"] += 1
                if rc != 0:
                    return got_st, ["the hook returned %d (%s)" % (rc, _lib.status_string(rc))]
                if got_st[0]["last_dx"].tobytes() != dx_dev.tobytes():
                    return got_st, ["last_dx (a second launch on the same rows gave another step)"]
    bad, ratio = TC.compare(got_st, got_mb, ref_st, ref_mb, info)
    acc["rot"] = max(acc["rot"], ratio)
    acc["launches"] += 1
    return got_st, bad


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_tails_against_model(built, variant):
    assert _lib.device_count() >= 1
    t0 = time.time()
    acc = {"rot": 0.0, "fast": 0.0, "fast_moved": 0, "second_pass": 0, "launches": 0}
    ran, failures = {}, []
    for exact in (True, False):
        for case in TC.cases():
            state, first = None, case.first
            for k in range(case.launches):
                state, bad = _one_launch(case, variant, exact, state, first, acc)
                if bad:
                    failures.append((case, exact, k, bad))
                    break
                first = 0
            ran[(exact, case.family)] = ran.get((exact, case.family), 0) + 1
    dt = time.time() - t0
    print("tails variant %d (%s): %d compared launches, %d second passes, %.2f s; worst rotation error / bound = %.3f; worst fast-path |dx - exact| / bound = %.4f "
          "(%d fast-path steps differ from the exact solver's in some bit)" % (variant, VARIANTS[variant], acc["launches"], acc["second_pass"], dt, acc["rot"],
                                                                                acc["fast"], acc["fast_moved"]))
    want = TC.family_counts()
    for exact in (True, False):
        assert {f: n for (e, f), n in ran.items() if e == exact} == want
    if failures:
        fam = {}
        for case, exact, k, bad in failures:
            key = "%s/%s" % (case.tail, case.family)
            fam[key] = fam.get(key, 0) + 1
        for case, exact, k, bad in failures[:8]:
            print("variant", variant, "exact bit" if exact else "default path", case.label, "launch", k, "differs in:", "; ".join(bad))
        pytest.fail("variant %d: %d of %d cases differ from the model, by family %s" % (variant, len(failures), 2 * len(TC.cases()), fam))
    assert acc["rot"] <= 1.0 and acc["fast"] <= 1.0
    assert acc["fast_moved"] > 0   # the default path is not the exact solver: the fast path did take systems


def test_tails_are_deterministic_across_variants(built):
    """the three instantiations of a tail differ in the reduction's shape and loads only: on rows whose sums are exact they return the same bytes"""
    assert _lib.device_count() >= 1
    for case in TC.cases():
        if case.family not in ("plain_continue", "mailbox", "icp_singular"):
            continue
        st_in, mb_in, rt, pt, _, _, _ = TC.run_model(case, exact=False)
        outs = [_launch(case, v, case.first, case.T0, st_in, mb_in, rt, pt, case.word(False)) for v in sorted(VARIANTS)]
        assert all(rc == 0 for rc, _, _ in outs), case.label
        outs = [(st, mb) for _, st, mb in outs]
        for st, mb in outs[1:]:
            assert st.tobytes() == outs[0][0].tobytes(), case.label
            assert (mb is None and outs[0][1] is None) or mb.tobytes() == outs[0][1].tobytes(), case.label
