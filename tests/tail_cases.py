"""Cases and the plain model of the Gauss-Newton tails (loam_tail of csrc/kernels_p2plane.hpp, lu_tail of csrc/kernels_knn.hpp), shared by
tests/test_tail_cases.py (CPU: every family reaches the branch it is named after, by the model alone) and tests/test_gpu_tails.py (GPU: one launch
of one workgroup per case through include/fls_debug_tail.h, every word of GnState and of the mailbox against the model).

Rows with exact sums.  Every entry of columns 0..28 is an integer multiple of 2^-12 with |v| <= 2^20 and there are at most 2048 rows, so every
partial sum is an integer below 2^43 in units of 2^-12: any summation order gives the same double, and H, g, sum_res and n_valid are known
exactly whatever tree reduce_partials uses.  Columns 29..31 are NaN: a tail that read them would show it.  The pieces of a target are scattered
over all rows, negative pieces included.  The 29 targets of a row set are pairwise distinct, and those of the corner rows differ from those of
the planar rows, so that a slip of the index map or a swap of the two row sets shows.

The model is composed from what the suite already trusts: O.fullpiv_qr_solve_6 for the LOAM family, O.lu_inverse_6 with the left-to-right
inverse * b of tests/linalg_cases.py for modes 0 and 1, O.so3_exp, LC.mat3_mul_model, norm3d as sqrt((x^2 + y^2) + z^2).  The stop rules are the
reference's (loam_point_to_plane_ivox.h:181-189, icp_optimized.h:129-148, incremental_ndt.h:306-322), not the kernels'.

A case may state a threshold or a carried norm RELATIVE to the step it will see (the norm itself, the next double, a carried norm exactly 1e-4
away): resolve() turns that into numbers for a given step, so that the GPU test can place the same edge at the device's own fast-path step."""
import functools
import math
from fractions import Fraction

import numpy as np

from funny_lidar_slam_amd import _lib
from tests import linalg_cases as LC

EPS = LC.EPS
Q = 2.0 ** -12                      # the grid of every row entry
ROW_COUNTS = (1, 2, 15, 16, 17, 31, 32, 33, 205, 225, 457, 1025, 2048)
MAX_ITER = _lib.DEBUG_TAIL_MAX_ITER
ST, MB = np.dtype(_lib.DebugGnState), np.dtype(_lib.DebugMailbox)
ST_CANARY, MB_CANARY = 0xA5, 0x5A   # every byte of the state / the mailbox that a case does not set
ID_MASK, EXACT_SHIFT, MAX_IT_SHIFT, MAX_IT_LIMIT = 0x7FFFFF, 23, 24, 255   # LaunchWord (csrc/device_common.hpp)
SLACK = 1.0e30                      # a threshold every norm is below
NEVER = 0.0                         # a threshold no norm is below (strict <)

# what each family must count at the least; tests/test_tail_cases.py holds the model to it, tests/test_gpu_tails.py to having run the same cases
FAMILY_MIN = {
    "plain_continue": 52, "stop_rule1": 3, "rule1_one_side": 6, "loam_rule2": 8, "first_poisoned": 4, "thr_at_norm": 12, "icp_singular": 4,
    "icp_indefinite": 3, "min_effective": 6, "done_on_entry": 3, "iter_on_entry": 12, "mailbox": 20, "loam_rank_deficient": 2, "zero_step": 3,
    "chain": 3,
}


def launch_word(match_id, exact, max_it):
    """LaunchWord::pack"""
    return (match_id & ID_MASK) | ((1 << EXACT_SHIFT) if exact else 0) | (min(max_it, MAX_IT_LIMIT) << MAX_IT_SHIFT)


def seq_word(match_id, done, iterations):
    """SeqWord::pack"""
    return ((match_id & ID_MASK) << 9) | ((1 << 8) if done else 0) | (iterations & 0xFF)


def norm3d(v):
    x, y, z = float(v[0]), float(v[1]), float(v[2])
    return math.sqrt((x * x + y * y) + z * z)


def canary_state():
    return np.frombuffer(bytes([ST_CANARY]) * ST.itemsize, dtype=ST).copy()


def canary_mailbox():
    return np.frombuffer(bytes([MB_CANARY]) * MB.itemsize, dtype=MB).copy()


# ---------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------
def dyadic(a):
    return np.round(np.asarray(a, dtype=np.float64) / Q) * Q


def tri_index(a, b):
    """index of (a, b), a <= b, in the row-wise upper triangle of a 6x6"""
    return a * 6 - (a * (a - 1)) // 2 + (b - a)


def targets(H, g, sum_res, n_valid):
    """the 29 column totals of a row set: 21 upper-triangle entries row-wise, 6 of g, the residual sum, the count"""
    H = np.asarray(H, dtype=np.float64)
    assert np.array_equal(H, H.T)
    t = np.zeros(29)
    for a in range(6):
        for b in range(a, 6):
            t[tri_index(a, b)] = H[a, b]
    t[21:27] = g
    t[27], t[28] = sum_res, n_valid
    assert np.array_equal(t, dyadic(t))
    return t


def scatter_rows(rng, nrows, tot):
    """rows[nrows][32] whose columns 0..28 sum to tot exactly: random pieces of up to 64 in every row, one row per column takes the remainder"""
    assert 1 <= nrows <= 2048
    units = np.round(np.asarray(tot) / Q).astype(np.int64)
    assert np.array_equal(units * Q, tot)
    p = rng.integers(-(1 << 18), (1 << 18) + 1, size=(nrows, 29))
    for c in range(29):
        r = int(rng.integers(nrows))
        p[r, c] += units[c] - p[:, c].sum()
    rows = np.full((nrows, 32), np.nan)
    rows[:, :29] = p.astype(np.float64) * Q
    assert np.abs(rows[:, :29]).max() <= 2.0 ** 20
    return rows


def exact_totals(rows):
    """the column sums of columns 0..28 in exact rational arithmetic"""
    return [sum((Fraction(float(v)) for v in rows[:, c]), Fraction(0)) for c in range(29)]


def totals(rows):
    return np.zeros(29) if rows is None else rows[:, :29].sum(axis=0)


def assemble(tot):
    H = np.zeros((6, 6))
    for i in range(6):
        for j in range(6):
            H[i, j] = tot[tri_index(min(i, j), max(i, j))]
    return H, tot[21:27].copy()


# ---------------------------------------------------------------------------------------------
# systems
# ---------------------------------------------------------------------------------------------
def _sym(A):
    U = np.triu(A)
    return U + np.triu(A, 1).T


def _distinct(*arrays):
    v = np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in arrays])
    return len(set(v.tolist())) == v.size


def spd_system(rng, x, scale=1.0):
    """a well-conditioned SPD H on the grid with pairwise distinct triangle entries, g = H x rounded to the grid (so the step is x to the grid over
    the smallest eigenvalue of H, which is above scale^2)"""
    while True:
        J = rng.normal(size=(60, 6)) * rng.uniform(1.0, 3.0, size=6) * scale
        H = _sym(dyadic(J.T @ J))
        g = dyadic(H @ np.asarray(x))
        t = targets(H, g, 0.0, 0.0)
        if _distinct(t[:27]) and np.linalg.cond(H) < 200.0 and np.linalg.eigvalsh(H).min() > 1.0:
            return H, g


def stat_pair(rng):
    """(sum_res, n_valid) of a planar row set and of a corner row set, all four distinct, none equal to an entry of H"""
    return (float(dyadic(rng.uniform(300.0, 400.0))), int(rng.integers(1000, 30000))), (float(dyadic(rng.uniform(10.0, 20.0))), int(rng.integers(50, 900)))


def rotation(rng):
    Qm, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Qm * np.sign(np.linalg.det(Qm))


def pose(rng, t_scale=20.0):
    T = np.eye(4)
    T[:3, :3] = rotation(rng)
    T[:3, 3] = rng.uniform(-1.0, 1.0, 3) * t_scale
    return T.reshape(-1, order="F").copy()


# ---------------------------------------------------------------------------------------------
# a case
# ---------------------------------------------------------------------------------------------
class TailCase:
    """One launch (or a chain of two).  rot_thr / pos_thr: a float, or f(rn, pn) of the step's rotation and translation norm; fix_state: None or
    f(state, rn, pn), which sets carried words relative to the step.  expect: what the model must find (checked by tests/test_tail_cases.py)."""

    def __init__(self, tail, family, name, rows_b, rows_a=None, mode=0, first=1, T0=None, state=None, rot_thr=NEVER, pos_thr=NEVER, fix_state=None,
                 min_eff=0, max_it=30, match_id=5, mailbox=True, launches=1, fast="accept", expect=None):
        self.tail, self.family, self.name, self.rows_a, self.rows_b, self.mode, self.first = tail, family, name, rows_a, rows_b, mode, first
        self.T0, self.state, self.rot_thr, self.pos_thr, self.fix_state, self.min_eff = T0, state, rot_thr, pos_thr, fix_state, min_eff
        self.max_it, self.match_id, self.mailbox, self.launches, self.fast, self.expect = max_it, match_id, mailbox, launches, fast, dict(expect or {})
        for r in (rows_a, rows_b):
            if r is not None:
                r.setflags(write=False)
        self.relative = callable(rot_thr) or callable(pos_thr) or fix_state is not None

    @property
    def label(self):
        return "%s/%s/%s" % (self.tail, self.family, self.name)

    def word(self, exact):
        return launch_word(self.match_id, exact, self.max_it)


def system_of(case):
    """(H, g, tot_a, tot_b) as the tail assembles them: H = tot_a + tot_b entry by entry (one exact addition)"""
    ta, tb = totals(case.rows_a), totals(case.rows_b)
    H, g = assemble(ta + tb)
    return H, g, ta, tb


def lu_product(inv, b):
    """the tail's inverse * b: s = 0; s += inv[i, q] * b[q], q = 0..5 (tests/linalg_cases.py::oracle_lu6)"""
    x = np.zeros(6)
    for i in range(6):
        s = 0.0
        for q in range(6):
            s += float(inv[i, q]) * float(b[q])
        x[i] = s
    return x


def step_kind(case, H, tb):
    """'early' (incremental_ndt.h:306), 'skip' (icp_optimized.h:129) or 'step'"""
    from oracle import oracle as O
    if case.tail == "lu":
        if case.mode == 1 and int(tb[28]) < case.min_eff:
            return "early"
        if case.mode == 0 and O.lu_inverse_6(H)[1] == 0.0:
            return "skip"
    return "step"


def oracle_step(case, H, g):
    from oracle import oracle as O
    if case.tail == "loam":
        return O.fullpiv_qr_solve_6(H, g)
    with np.errstate(all="ignore"):
        return lu_product(O.lu_inverse_6(H)[0], g)


def step_norms(case, dx):
    """(rotation norm, translation norm) of a step: head / tail for the LOAM family and mode 1, tail / head for mode 0"""
    if case.tail == "lu" and case.mode == 0:
        return norm3d(dx[3:6]), norm3d(dx[0:3])
    return norm3d(dx[0:3]), norm3d(dx[3:6])


def resolve(case, state, rn, pn):
    """(rot_thr, pos_thr, state) of the launch for a step of norms rn, pn"""
    st = state.copy()
    if case.fix_state is not None:
        case.fix_state(st[0], rn, pn)
    rt = case.rot_thr(rn, pn) if callable(case.rot_thr) else case.rot_thr
    pt = case.pos_thr(rn, pn) if callable(case.pos_thr) else case.pos_thr
    return float(rt), float(pt), st


def carried_at(norm, gap):
    """a carried norm c with fl(|norm - c|) == gap exactly (norm < 2e-5, gap ~ 1e-4: c and gap share an ulp, every gap on that grid is reached)"""
    assert 0.0 < norm < 2.0e-5
    c = norm + gap
    for _ in range(64):
        d = abs(norm - c)
        if d == gap:
            return c
        c = float(np.nextafter(c, np.inf if d < gap else 0.0))
    raise AssertionError("no carried norm %r away from %r" % (gap, norm))


def model_launch(case, state, mailbox, first, word, rot_thr, pos_thr, dx=None):
    """One launch on `state` (1,) ST and `mailbox` (1,) MB or None, already resolved.  dx: the step to apply where the tail takes one (None: the
    oracle solver's).  Returns (state, mailbox, info)."""
    from oracle import oracle as O
    st = state.copy()
    mb = None if mailbox is None else mailbox.copy()
    s = st[0]
    if not first and int(s["done"]) != 0:
        return st, mb, {"kind": "done", "dx": None, "theta": 0.0}
    H, g, ta, tb = system_of(case)
    T = (np.asarray(case.T0, dtype=np.float64) if first else s["T"]).copy()
    it = 0 if first else int(s["iter"])
    kind = step_kind(case, H, tb)
    if kind == "step" and dx is None:
        dx = oracle_step(case, H, g)
    s["H"] = H.reshape(-1, order="F")
    s["g"] = g
    dxo = np.zeros(6)
    stop = conv = 0
    theta = 0.0
    T44 = T.reshape(4, 4, order="F").copy()
    if case.tail == "loam":
        last_rot = 0.0 if first else float(s["last_rot"])
        last_pos = 0.0 if first else float(s["last_pos"])
        Rd = O.so3_exp(dx[0:3])
        T44[:3, :3] = LC.mat3_mul_model(Rd[None], T44[None, :3, :3])[0]   # left-multiplicative (loam_point_to_plane_ivox.h:169)
        T44[:3, 3] = T44[:3, 3] + dx[3:6]
        rn, pn = step_norms(case, dx)
        theta = rn
        drot, dpos = abs(rn - last_rot), abs(pn - last_pos)
        stop = 1 if ((rn < rot_thr and pn < pos_thr) or (drot < 1.0e-4 and dpos < 1.0e-4)) else 0
        s["last_rot"], s["last_pos"] = rn, pn
        s["last_dx"] = dx
        s["n_valid"], s["n_valid2"] = int(tb[28]), int(ta[28])
        s["sum_res"], s["sum_res2"] = tb[27], ta[27]
        dxo = np.asarray(dx, dtype=np.float64)
        nv, nv2, sr, sr2 = int(tb[28]), int(ta[28]), tb[27], ta[27]
    else:
        nv, nv2, sr, sr2 = int(tb[28]), 0, tb[27], 0.0
        s["n_valid"], s["sum_res"] = nv, sr
        if kind == "early":
            stop = 1
        elif kind == "skip":
            pass
        else:
            dth, dt = (dx[3:6], dx[0:3]) if case.mode == 0 else (dx[0:3], dx[3:6])
            Rd = O.so3_exp(dth)
            T44[:3, :3] = LC.mat3_mul_model(T44[None, :3, :3], Rd[None])[0]   # right-multiplicative (icp_optimized.h:136, incremental_ndt.h:312)
            T44[:3, 3] = T44[:3, 3] + dt
            rn, pn = step_norms(case, dx)
            theta = rn
            s["last_dx"] = dx
            dxo = np.asarray(dx, dtype=np.float64)
            if rn < rot_thr and pn < pos_thr:
                stop = conv = 1
        s["converged"] = conv
    Tn = T44.reshape(-1, order="F")
    s["T"] = Tn
    s["done"] = stop
    if it < MAX_ITER:
        s["log_T"][16 * it:16 * it + 16] = Tn
        s["log_nv"][it] = nv
        s["log_res"][it] = sr
    s["iter"] = it + 1
    payload = False
    if mb is not None:
        m = mb[0]
        max_it = word >> MAX_IT_SHIFT
        payload = bool(stop or max_it == 0 or it + 1 >= max_it)
        if payload:
            m["T"], m["last_dx"], m["sum_res"], m["sum_res2"] = Tn, dxo, sr, sr2
            m["iter"], m["done"], m["converged"], m["n_valid"], m["n_valid2"] = it + 1, stop, conv, nv, nv2
        m["seq"] = seq_word(word & ID_MASK, stop, it + 1)
    return st, mb, {"kind": kind, "dx": None if kind != "step" else np.asarray(dx, dtype=np.float64).copy(), "theta": theta, "stop": stop, "conv": conv,
                    "payload": payload, "it": it, "H": H, "g": g}


def initial_state(case):
    return canary_state() if case.state is None else case.state.copy()


def run_model(case, exact=True, dx=None, state=None, first=None):
    """The model of one launch of `case`: thresholds and carried words resolved for the step `dx` (None: the oracle's).  Returns
    (state_in, mailbox_in, rot_thr, pos_thr, state_out, mailbox_out, info)."""
    first = case.first if first is None else first
    st0 = initial_state(case) if state is None else state
    H, g, ta, tb = system_of(case)
    entered_done = (not first) and int(st0[0]["done"]) != 0
    kind = "done" if entered_done else step_kind(case, H, tb)
    if kind == "step" and dx is None:
        dx = oracle_step(case, H, g)
    rn, pn = step_norms(case, dx) if kind == "step" else (0.0, 0.0)
    rot_thr, pos_thr, st_in = resolve(case, st0, rn, pn)
    mb_in = canary_mailbox() if case.mailbox else None
    st_out, mb_out, info = model_launch(case, st_in, mb_in, first, case.word(exact), rot_thr, pos_thr, dx)
    return st_in, mb_in, rot_thr, pos_thr, st_out, mb_out, info


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
def _state(T=None, iter_=None, done=None, last_rot=None, last_pos=None):
    st = canary_state()
    s = st[0]
    if T is not None: s["T"] = T
    if iter_ is not None: s["iter"] = iter_
    if done is not None: s["done"] = done
    if last_rot is not None: s["last_rot"] = last_rot
    if last_pos is not None: s["last_pos"] = last_pos
    return st


def _split(rng, H, g, planar, corner):
    """targets of a corner row set and of a planar row set that add up to H, g: the corner part is a random symmetric grid matrix"""
    while True:
        Ha = _sym(dyadic(rng.uniform(-40.0, 40.0, size=(6, 6))))
        ga = dyadic(rng.uniform(-5.0, 5.0, size=6))
        ta = targets(Ha, ga, corner[0], corner[1])
        tb = targets(H - Ha, g - ga, planar[0], planar[1])
        if _distinct(ta, tb):
            return ta, tb


LARGE = np.array([0.11, -0.07, 0.05, 0.4, -0.3, 0.25])          # a step far above every threshold and every 1e-4 gap
SMALL = np.array([6.0e-6, -4.0e-6, 5.0e-6, 7.0e-6, 3.0e-6, -6.0e-6])   # norms below 2e-5: carried_at() can place the 1e-4 gap exactly


def _loam(rng, family, name, x=LARGE, nrows=17, nrows_a=0, scale=1.0, **kw):
    H, g = spd_system(rng, x, scale)
    planar, corner = stat_pair(rng)
    if nrows_a:
        ta, tb = _split(rng, H, g, planar, corner)
        rows_a, rows_b = scatter_rows(rng, nrows_a, ta), scatter_rows(rng, nrows, tb)
    else:
        rows_a, rows_b = None, scatter_rows(rng, nrows, targets(H, g, planar[0], planar[1]))
    kw.setdefault("T0", pose(rng))
    return TailCase("loam", family, name, rows_b, rows_a=rows_a, **kw)


def _lu(rng, family, name, mode, x=LARGE, nrows=17, H=None, g=None, n_valid=None, **kw):
    if H is None:
        H, g = spd_system(rng, x)
    planar, _ = stat_pair(rng)
    rows = scatter_rows(rng, nrows, targets(H, g, planar[0], planar[1] if n_valid is None else n_valid))
    kw.setdefault("T0", pose(rng))
    return TailCase("lu", family, name, rows, mode=mode, **kw)


def _indefinite(rng, want_negative_det):
    """a symmetric grid matrix with eigenvalues of both signs, cond < 1e3, det < 0 or det > 0"""
    while True:
        V = rotation6(rng)
        neg = 1 if want_negative_det else 2
        lam = rng.uniform(20.0, 200.0, size=6) * np.array([-1.0] * neg + [1.0] * (6 - neg))
        H = _sym(dyadic(V @ np.diag(lam) @ V.T))
        w = np.linalg.eigvalsh(H)
        if (np.linalg.det(H) < 0) == want_negative_det and (w < 0).sum() == neg and np.abs(w).min() > 5.0 and _distinct(targets(H, np.zeros(6), 0.0, 0.0)[:21]):
            return H


def rotation6(rng):
    Qm, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    return Qm


@functools.lru_cache(maxsize=None)
def cases():
    """every case, built once; each is read-only"""
    rng = np.random.default_rng(20260117)
    out = []
    nxt = lambda v: float(np.nextafter(v, np.inf))

    # plain step, continues: every row count, both tails, both modes, corner rows absent and present; half without a mailbox
    for k, n in enumerate(ROW_COUNTS):
        na = ROW_COUNTS[(k + 5) % len(ROW_COUNTS)]
        out.append(_loam(rng, "plain_continue", "rows%d" % n, nrows=n, mailbox=bool(k & 1), expect={"stop": 0}))
        out.append(_loam(rng, "plain_continue", "rows%d+corner%d" % (n, na), nrows=n, nrows_a=na, mailbox=not (k & 1), expect={"stop": 0}))
        for mode in (0, 1):
            out.append(_lu(rng, "plain_continue", "mode%d_rows%d" % (mode, n), mode, nrows=n, mailbox=bool((k + mode) & 1), expect={"stop": 0, "conv": 0}))

    # rule 1 stops; one satisfied threshold alone does not
    out.append(_loam(rng, "stop_rule1", "both_slack", rot_thr=SLACK, pos_thr=SLACK, nrows_a=15, expect={"stop": 1}))
    out.append(_loam(rng, "rule1_one_side", "rot_only", rot_thr=SLACK, pos_thr=NEVER, expect={"stop": 0}))
    out.append(_loam(rng, "rule1_one_side", "pos_only", rot_thr=NEVER, pos_thr=SLACK, expect={"stop": 0}))
    for mode in (0, 1):
        out.append(_lu(rng, "stop_rule1", "mode%d_both_slack" % mode, mode, rot_thr=SLACK, pos_thr=SLACK, expect={"stop": 1, "conv": 1}))
        out.append(_lu(rng, "rule1_one_side", "mode%d_rot_only" % mode, mode, rot_thr=SLACK, pos_thr=NEVER, expect={"stop": 0, "conv": 0}))
        out.append(_lu(rng, "rule1_one_side", "mode%d_pos_only" % mode, mode, rot_thr=NEVER, pos_thr=SLACK, expect={"stop": 0, "conv": 0}))

    # LOAM rule 2 alone: the norms are above the thresholds (1e-9), the carried norms sit 1e-4 away, one double less, well inside, far outside
    gap, inside = 1.0e-4, float(np.nextafter(1.0e-4, 0.0))

    def carried(rot_gap, pos_gap):
        def f(s, rn, pn):
            s["last_rot"] = carried_at(rn, rot_gap) if rot_gap else rn * 0.5
            s["last_pos"] = carried_at(pn, pos_gap) if pos_gap else pn * 0.5
        return f

    def carried_far(s, rn, pn):
        s["last_rot"], s["last_pos"] = rn + 0.5, pn * 0.5

    for name, fix, stop in (("rot_at_1e-4", carried(gap, 0), 0), ("rot_one_double_inside", carried(inside, 0), 1), ("pos_at_1e-4", carried(0, gap), 0),
                            ("pos_one_double_inside", carried(0, inside), 1), ("both_at_1e-4", carried(gap, gap), 0),
                            ("both_one_double_inside", carried(inside, inside), 1), ("well_inside", carried(0, 0), 1), ("rot_far", carried_far, 0)):
        out.append(_loam(rng, "loam_rule2", name, x=SMALL, scale=16.0, first=0, state=_state(T=pose(rng), iter_=3, done=0), fix_state=fix, rot_thr=1.0e-9, pos_thr=1.0e-9,
                         nrows_a=(2 if stop else 0), expect={"stop": stop}))

    # first = 1: the incoming state is poison (done = 1, a wild iter, a pose of canary bytes, carried norms that would satisfy rule 2 at once)
    def poison(s, rn, pn):
        s["last_rot"], s["last_pos"] = rn, pn

    for na in (0, 31):
        out.append(_loam(rng, "first_poisoned", "corner%d" % na, first=1, state=_state(iter_=37, done=1), fix_state=poison, nrows_a=na, expect={"stop": 0, "it": 0}))
    for mode in (0, 1):
        out.append(_lu(rng, "first_poisoned", "mode%d" % mode, mode, first=1, state=_state(iter_=61, done=1), expect={"stop": 0, "it": 0}))

    # a threshold at the norm does not stop, the next double does; the other threshold is slack (LOAM: first = 1 and a large step keep rule 2 off)
    edge = (("rot_at_norm", lambda rn, pn: rn, SLACK, 0), ("rot_next_double", lambda rn, pn: nxt(rn), SLACK, 1),
            ("pos_at_norm", SLACK, lambda rn, pn: pn, 0), ("pos_next_double", SLACK, lambda rn, pn: nxt(pn), 1))
    for name, rt, pt, stop in edge:
        out.append(_loam(rng, "thr_at_norm", name, rot_thr=rt, pos_thr=pt, expect={"stop": stop}))
        for mode in (0, 1):
            out.append(_lu(rng, "thr_at_norm", "mode%d_%s" % (mode, name), mode, rot_thr=rt, pos_thr=pt, expect={"stop": stop, "conv": stop}))

    # mode 0, exactly singular H: the update is skipped, the iteration counted, the mailbox gets a zero step
    Hs, gs = spd_system(rng, LARGE)
    Hz = Hs.copy(); Hz[2, :] = 0.0; Hz[:, 2] = 0.0
    He = Hs.copy(); He[4, :] = He[1, :]; He[:, 4] = He[:, 1]; He[4, 4] = He[1, 1]; He[1, 4] = He[4, 1] = He[1, 1]
    Hi = _sym(np.round(Hs)); Hi[5, :] = Hi[0, :]; Hi[:, 5] = Hi[:, 0]; Hi[5, 5] = Hi[0, 0]; Hi[0, 5] = Hi[5, 0] = Hi[0, 0]
    for name, Hx, max_it in (("zero_row_col", Hz, 0), ("equal_rows", He, 30), ("equal_rows_int", Hi, 1), ("zero_matrix", np.zeros((6, 6)), 30)):
        out.append(_lu(rng, "icp_singular", name, 0, H=Hx, g=gs, rot_thr=SLACK, pos_thr=SLACK, max_it=max_it, fast="decline",
                       state=_state(T=pose(rng), iter_=4, done=0), first=0, expect={"kind": "skip", "stop": 0, "conv": 0}))

    # mode 0, negative determinant and indefinite H: the fast path declines, LU solves, the update is applied
    for name, negdet in (("negative_det", True), ("indefinite_positive_det", False), ("negative_det_2", True)):
        Hn = _indefinite(rng, negdet)
        out.append(_lu(rng, "icp_indefinite", name, 0, H=Hn, g=dyadic(Hn @ LARGE), fast="decline", expect={"kind": "step", "stop": 0}))

    # mode 1 stops early below min_effective; mode 0 never does
    for mode in (1, 0):
        for d in (-1, 0, 1):
            early = mode == 1 and d == 1
            out.append(_lu(rng, "min_effective", "mode%d_effective_min%+d" % (mode, -d), mode, n_valid=500 - d, min_eff=500, first=0,
                           state=_state(T=pose(rng), iter_=2, done=0), expect={"kind": "early" if early else "step", "stop": int(early), "conv": 0}))

    # done = 1 on entry, first = 0: nothing is written
    out.append(_loam(rng, "done_on_entry", "loam", first=0, state=_state(T=pose(rng), iter_=6, done=1), rot_thr=SLACK, pos_thr=SLACK, nrows_a=2, expect={"kind": "done"}))
    for mode in (0, 1):
        out.append(_lu(rng, "done_on_entry", "mode%d" % mode, mode, first=0, state=_state(T=pose(rng), iter_=6, done=1 + mode * 6), expect={"kind": "done"}))

    # iter on entry at and beyond the end of the logs
    for it in (62, 63, 64, 200):
        kw = dict(first=0, max_it=255, expect={"it": it, "stop": 0})
        out.append(_loam(rng, "iter_on_entry", "iter%d" % it, state=_state(T=pose(rng), iter_=it, done=0, last_rot=9.0, last_pos=9.0), **kw))
        for mode in (0, 1):
            out.append(_lu(rng, "iter_on_entry", "mode%d_iter%d" % (mode, it), mode, state=_state(T=pose(rng), iter_=it, done=0), **kw))

    # the mailbox: max_iterations 0, above the next iteration count, equal to it; ids 0, 1 and the mask; and a stop below max_iterations
    for tail in ("loam", "lu"):
        for max_it, pay in ((0, True), (9, False), (6, True)):
            for mid in (0, 1, ID_MASK):
                kw = dict(first=0, max_it=max_it, match_id=mid, expect={"payload": pay, "stop": 0, "it": 5})
                if tail == "loam":
                    out.append(_loam(rng, "mailbox", "max_it%d_id%x" % (max_it, mid), nrows_a=16, state=_state(T=pose(rng), iter_=5, done=0, last_rot=9.0, last_pos=9.0), **kw))
                else:
                    out.append(_lu(rng, "mailbox", "max_it%d_id%x" % (max_it, mid), 0, state=_state(T=pose(rng), iter_=5, done=0), **kw))
    out.append(_loam(rng, "mailbox", "stop_below_max_it", rot_thr=SLACK, pos_thr=SLACK, max_it=9, match_id=0x2AAAAA, nrows_a=33, expect={"payload": True, "stop": 1}))
    out.append(_lu(rng, "mailbox", "stop_below_max_it", 1, rot_thr=SLACK, pos_thr=SLACK, max_it=9, match_id=0x555555, expect={"payload": True, "stop": 1, "conv": 1}))

    # LOAM, three constrained directions: integers, so the rank is exactly 3; the fast path declines, the step is the rank-revealing QR's
    for k in range(2):
        while True:
            A = rng.integers(-5, 6, size=(12, 3)).astype(np.float64)
            B = rng.integers(-3, 4, size=(3, 6)).astype(np.float64)
            Jm = A @ B
            Hr = Jm.T @ Jm
            if np.linalg.matrix_rank(Hr) == 3:
                break
        gr = Hr @ dyadic(LARGE * 0.5)
        planar, _ = stat_pair(rng)
        rows = scatter_rows(rng, (33, 457)[k], targets(Hr, gr, planar[0], planar[1]))
        out.append(TailCase("loam", "loam_rank_deficient", "rank3_%d" % k, rows, T0=pose(rng), fast="decline", expect={"kind": "step", "stop": 0}))

    # an exactly zero step: the identity branch of SO3Exp, the pose keeps its bits
    planar, _ = stat_pair(rng)
    out.append(TailCase("loam", "zero_step", "zero_system", scatter_rows(rng, 16, targets(np.zeros((6, 6)), np.zeros(6), planar[0], planar[1])), T0=pose(rng),
                        rot_thr=1.0e-6, pos_thr=1.0e-6, fast="decline", expect={"stop": 1, "zero": True}))
    for mode in (0, 1):
        out.append(_lu(rng, "zero_step", "mode%d_zero_g" % mode, mode, H=Hs, g=np.zeros(6), rot_thr=1.0e-6, pos_thr=1.0e-6, expect={"stop": 1, "conv": 1, "zero": True}))

    # two launches: the second takes the state the first returned
    out.append(_loam(rng, "chain", "loam", nrows=225, nrows_a=32, launches=2, max_it=2, expect={"stop": 0}))
    for mode in (0, 1):
        out.append(_lu(rng, "chain", "mode%d" % mode, mode, nrows=(205, 457)[mode], launches=2, max_it=2, expect={"stop": 0}))

    labels = [c.label for c in out]
    assert len(set(labels)) == len(labels)
    return tuple(out)


def family_counts():
    n = {}
    for c in cases():
        n[c.family] = n.get(c.family, 0) + 1
    return n


# ---------------------------------------------------------------------------------------------
# comparison of a returned state / mailbox with the model's
# ---------------------------------------------------------------------------------------------
def rotation_bound(theta):
    """|R_new - model| per entry, model = mat3_mul_model on O.so3_exp of the same step: the suite holds the device's and the oracle's SO3Exp to
    4 EPS (1 + theta) each against long double; an entry of the product is three terms with |R| <= 1, and three roundings: (24 (1 + theta) + 3) EPS"""
    return (24.0 * (1.0 + theta) + 3.0) * EPS


ROT = [i + 4 * j for j in range(3) for i in range(3)]   # the rotation entries of a column-major 4x4


def _bits_equal(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def compare(got_st, got_mb, ref_st, ref_mb, info):
    """-> (list of the differing words, worst |rotation entry - model| / bound).  Everything bit for bit, except the rotation entries of T, of the
    log slot and of the mailbox pose where a step was taken: those are within rotation_bound of the model, and the log slot and the mailbox pose
    carry the bits of the state's own T."""
    bad, ratio = [], 0.0
    g, r = got_st[0], ref_st[0]
    stepped = info["kind"] == "step" and info["theta"] > EPS
    it = info.get("it", 0)
    for name in ST.names:
        if stepped and name in ("T", "log_T"):
            continue
        if not _bits_equal(g[name], r[name]):
            bad.append(name)
    if stepped:
        bound = rotation_bound(info["theta"])
        mask = np.ones(16, bool); mask[ROT] = False
        if not _bits_equal(g["T"][mask], r["T"][mask]):
            bad.append("T (translation, bottom row)")
        err = float(np.abs(g["T"][ROT] - r["T"][ROT]).max())
        ratio = err / bound
        if not err <= bound:
            bad.append("T (rotation: %.3e > %.3e)" % (err, bound))
        ref_log = r["log_T"].copy()
        if it < MAX_ITER:
            ref_log[16 * it:16 * it + 16] = g["T"]
        if not _bits_equal(g["log_T"], ref_log):
            bad.append("log_T")
    if (got_mb is None) != (ref_mb is None):
        bad.append("mailbox presence")
    elif got_mb is not None:
        gm, rm = got_mb[0], ref_mb[0]
        for name in MB.names:
            want = rm[name]
            if name == "T" and stepped and info["payload"]:
                want = g["T"]
            if not _bits_equal(gm[name], want):
                bad.append("mailbox." + name)
    return bad, ratio
