"""Constructed inputs of the iVox map-update decision -- LoamPointToPlaneIVOX::AddCloudToLocalMap's per-point rule
(include/registration/loam_point_to_plane_ivox.h:79-131) as ivox_add_decide_kernel<MATERIALIZE> and ivox_nn_materialize_kernel
(csrc/kernels_ivox_coop.hpp) and ivox_decide_host (csrc/matcher_p2plane_ivox.hpp) run it -- and numpy models of everything the launch does
besides the rule: the two list forms, the materialization, the block counts, the status words, the speculative gate.

Two layers.  A *case* (cases()) is the rule's own input: source points, a pose, filter_size_map_min, five neighbours and a count per point,
and per point what the case claims about it (`expect`, `kind`).  A *launch* (launches()) is a case dressed as the kernel's arguments: lists in
rows form, in ids form over a map, or both mixed inside every wave; the template flag; counting on or off; a gate.  expected(launch, decide)
gives every output of the launch, the codes and world points by `decide` (the oracle's flo_ivox_add_decide), the rest by numpy.

rule_model() is the rule in numpy doubles, with named mutants (one wrong edge each).  It is not what the device is compared with: the CPU test
(tests/test_ivox_decide_cases.py) requires it to equal the oracle on every case and every mutant to differ from the oracle on the case named
for it, which is how a case proves that it reaches the edge it is named after.  No GPU is needed for anything here."""
import collections
import functools

import numpy as np

FS = 0.5                 # filter_size_map_min of the product (loam_point_to_plane_ivox.h:351)
FILL = 0xA5              # FLS_DEBUG_IVOX_DECIDE_FILL
MAP_PAD = 64             # FLS_DEBUG_IVOX_DECIDE_MAP_PAD
BLOCK = 256              # threads per workgroup of the decision launch
SKIPPED = 16             # kUpdSkipped
MIN_VALID = 50           # the n_valid gate of Match (:201-203)
ROWS_BIT = 0x80          # count byte: the list is in rows form
IDENT = np.eye(4).reshape(-1, order="F")
# behind the slot bound: beyond every face of the cells around the origin where the stale-id case lives, so a decision that read it differs
SENTINEL = np.array([3.3125, -2.8125, 4.5625, 0.0], np.float32)
SENTINEL.view(np.uint32)[3] = 0x7F5A5A5A
STALE_ROW = np.array([0, 0, 0, 0xFFFFFFFF], np.uint32)  # (0, 0, 0, id -1)
MUTANTS = ("ge", "no_eps", "break0", "cnt_gt0", "trunc", "float_pw")

Case = collections.namedtuple("Case", "name src T fs nn cnt expect kind axis mutants")
Launch = collections.namedtuple("Launch", "name case src T fs rows cnt ids map_rows materialize count gate stale")


def f32(x):
    return np.asarray(x, dtype=np.float32)


def nudge(x, k):
    """the float32 k steps above (k > 0) or below (k < 0) x"""
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return x


def transform(src, T, in_float=False):
    """pcl::transformPoint(p, Affine3d(T)): the product in doubles, the result a float (in_float: the product in floats, what it must not be)"""
    T = np.asarray(T, np.float64).reshape(4, 4, order="F")
    src = f32(src).reshape(-1, 3)
    with np.errstate(all="ignore"):
        if in_float:
            Tf, x, y, z = T.astype(np.float32), src[:, 0], src[:, 1], src[:, 2]
            return np.stack([((Tf[r, 0] * x + Tf[r, 1] * y) + Tf[r, 2] * z) + Tf[r, 3] for r in range(3)], axis=1)
        x, y, z = (src[:, a].astype(np.float64) for a in range(3))
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1).astype(np.float32)


def centre(pw, fs, trunc=False):
    """the centre of the cell of pw, in doubles as the rule forms it"""
    with np.errstate(all="ignore"):
        q = f32(pw).astype(np.float64) / fs
        return ((np.trunc(q) if trunc else np.floor(q)) + 0.5) * fs


def sq(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def rule_model(src, T, fs, nn, cnt, mutant=None):
    """(code, pw) by the rule in numpy doubles.  mutant: None, or one wrong edge -- "ge" (>= on the half-cell test), "no_eps" (the 1e-6 missing),
    "break0" (the loop ends after k = 0), "cnt_gt0" (the loop runs for any count above 0), "trunc" (truncation for floor), "float_pw" (the pose
    product in floats)."""
    assert mutant is None or mutant in MUTANTS
    nn, cnt = f32(nn).reshape(-1, 5, 3), np.asarray(cnt).astype(np.int64)
    pw = transform(src, T, in_float=mutant == "float_pw")
    with np.errstate(all="ignore"):
        c = centre(pw, fs, trunc=mutant == "trunc")
        half = 0.5 * fs
        d0 = np.abs(nn[:, 0, :].astype(np.float64) - c)
        two = ((d0 >= half) if mutant == "ge" else (d0 > half)).all(axis=1)
        dist = sq(pw.astype(np.float64) - c)
        f2 = sq(nn.astype(np.float64) - c[:, None, :])
        nearer = f2 < (dist if mutant == "no_eps" else dist + 1.0e-6)[:, None]
        found = nearer[:, 0] if mutant == "break0" else nearer.any(axis=1)
        loop = cnt > 0 if mutant == "cnt_gt0" else cnt >= 5
    code = np.where(cnt == 0, 1, np.where(two, 2, np.where(loop & found, 0, 1))).astype(np.uint8)
    return code, pw


def flippers(src, T, fs, nn, cnt):
    """per point a neighbour that, read in place of its first one, changes the decision: the cell centre where the point is code 2, the centre
    of the cell one step up on every axis otherwise (beyond all three faces: code 2)"""
    code, pw = rule_model(src, T, fs, nn, cnt)
    c = centre(pw, fs)
    with np.errstate(all="ignore"):
        return np.where((code == 2)[:, None], c, c + fs).astype(np.float32)


# ----------------------------------------------------------------- the cases -----------------------------------------------------------------
class _Points:
    def __init__(self):
        self.src, self.nn, self.cnt, self.expect, self.kind, self.axis = [], [], [], [], [], []

    def add(self, src, nn, cnt, expect=None, kind="", axis=-1):
        """expect: 0, 1, 2, "not2" or None (the oracle simply decides)"""
        nn = f32(nn).reshape(-1, 3)
        assert len(nn) in (1, 5)
        self.src.append(f32(src).reshape(3)); self.nn.append(np.repeat(nn, 5, axis=0) if len(nn) == 1 else nn); self.cnt.append(cnt)
        self.expect.append(expect); self.kind.append(kind); self.axis.append(axis)

    def case(self, name, T=IDENT, fs=FS, mutants=()):
        arrs = (np.stack(self.src), np.asarray(T, np.float64).copy(), fs, np.stack(self.nn), np.array(self.cnt, np.uint8), tuple(self.expect),
                tuple(self.kind), tuple(self.axis), tuple(mutants))
        for a in arrs:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        return Case(name, *arrs)


BASE = f32([1.1, 2.3, -0.7])  # cell centre (1.25, 2.25, -0.75): every coordinate of the half-cell constructions is a float, exactly


def _centre32(p, fs=FS):
    c = centre(f32(p).reshape(1, 3), fs)[0]
    assert np.array_equal(c, f32(c).astype(np.float64))
    return f32(c)


def _garbage(rng):
    g = rng.uniform(-1e30, 1e30, (5, 3)).astype(np.float32)
    g[0, 0], g[1, 1], g[2, 2], g[3] = np.nan, np.inf, -np.inf, 0.0
    return g


def _case_count0():
    rng, P = np.random.default_rng(7301), _Points()
    c = _centre32(BASE)
    P.add(BASE, _garbage(rng), 0, 1)
    P.add(BASE, c, 0, 1)                            # every neighbour on the centre: code 0 under any count of 5
    P.add(BASE, c + f32(0.5), 0, 1)                 # every neighbour beyond all faces: code 2 under any count above 0
    for _ in range(5):
        P.add(rng.uniform(-30, 30, 3), _garbage(rng), 0, 1)
    return P.case("count0_garbage_rows")


def _case_low_counts():
    """counts 1 to 4 (and 5 to 7 beside them): every neighbour is nearer the centre than the point, and only a count of 5 and more may look"""
    rng, P = np.random.default_rng(7302), _Points()
    for cnt in (1, 2, 3, 4, 5, 6, 7):
        for _ in range(3):
            c = f32((rng.integers(-80, 80, 3) + 0.5) * 0.5)
            p = f32(c + rng.choice([-1.0, 1.0], 3) * rng.uniform(0.1, 0.24, 3))
            assert np.array_equal(_centre32(p), c)
            P.add(p, c + f32(rng.uniform(-0.01, 0.01, (5, 3))), cnt, 1 if cnt < 5 else 0, kind="all_nearer")
    return P.case("low_counts_all_nearer", mutants=("cnt_gt0",))


def _case_half_cell():
    P = _Points()
    c, h = _centre32(BASE), np.float32(0.25)
    for sgn in (1, -1):
        face = f32([c[a] + sgn * h for a in range(3)])                       # exactly on the face
        out = f32([nudge(face[a], sgn) for a in range(3)])                   # one float beyond it
        ins = f32([nudge(face[a], -sgn) for a in range(3)])                  # one float inside it
        P.add(BASE, out, 1, 2, kind="beyond_all")
        P.add(BASE, out, 5, 2, kind="beyond_all")
        for a in range(3):
            q = out.copy(); q[a] = face[a]
            P.add(BASE, q, 1, "not2", kind="face_eq", axis=a)
            P.add(BASE, q, 5, "not2", kind="face_eq", axis=a)
            q = out.copy(); q[a] = ins[a]
            P.add(BASE, q, 1, "not2", kind="beyond_two", axis=a)
        P.add(BASE, face, 3, "not2", kind="face_eq", axis=0)
        # only the first neighbour counts: 1 to 4 beyond every face and the first inside it, and the converse
        P.add(BASE, np.stack([ins, out, out, out, out]), 5, "not2", kind="first_only")
        P.add(BASE, np.stack([out, ins, c, c, ins]), 5, 2, kind="first_only")
        P.add(BASE, np.stack([out, ins, c, c, ins]), 2, 2, kind="first_only")
    return P.case("half_cell_faces", mutants=("ge",))


def _case_distance_loop():
    P = _Points()
    c = _centre32(BASE)
    p = f32(c + f32([0.2, 0.1, -0.15]))
    far, near = f32(c + f32([0.24, 0.24, 0.24])), f32(c + f32([0.01, 0.0, 0.0]))
    for k in range(5):
        nn = np.stack([far] * 5); nn[k] = near
        P.add(p, nn, 5, 0, kind="only_%d_nearer" % k)
    P.add(p, far, 5, 1, kind="none_nearer")
    P.add(p, near, 5, 0, kind="all_nearer")
    # a neighbour exactly as far from the centre as the point (the point itself, or its mirror image): nearer only by the 1e-6
    P.add(p, np.stack([far, far, p, far, far]), 5, 0, kind="same_dist")
    P.add(p, np.stack([far, far, far, far, f32(2 * c - p)]), 5, 0, kind="same_dist")
    return P.case("distance_loop", mutants=("break0", "no_eps"))


def _case_bracket():
    """strictness of < at equality cannot be pinned with float inputs: a neighbour one float step either side of dist + 1e-6, on each axis"""
    P = _Points()
    c = _centre32(BASE)
    p = f32(c + f32([0.2, 0.1, -0.15]))
    thr = sq(p.astype(np.float64) - c.astype(np.float64)) + 1.0e-6
    far = f32(c + f32([0.24, 0.24, 0.24]))
    for a in range(3):
        for sgn in (1, -1):
            q = c.copy()
            q[a] = np.float32(c[a] + sgn * np.sqrt(thr))
            while sq(q.astype(np.float64) - c) >= thr:
                q[a] = nudge(q[a], -sgn)
            while sq(q.astype(np.float64) - c) < thr:
                lo = q.copy(); q[a] = nudge(q[a], sgn)
            for k in (0, 2, 4):
                nn = np.stack([far] * 5); nn[k] = lo
                P.add(p, nn, 5, 0, kind="bracket_lo", axis=a)
                nn = np.stack([far] * 5); nn[k] = q
                P.add(p, nn, 5, 1, kind="bracket_hi", axis=a)
    return P.case("less_than_bracket", mutants=("no_eps",))


NEG_VALUES = (-1e-7, -0.0, 0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, -0.7, -13.26, 1999.9, -1999.9, 2000.0, -2000.0, 1999.5, -1999.5, -2000.4)


def _case_negative():
    """floor on negative coordinates: just below zero, +-0, exact multiples of fs on both signs, and +-2,000 m where floats are 1.2e-4 apart.
    Per value and axis: a first neighbour one float beyond every face of the right cell (code 2), one exactly on the face of that axis, and a
    list that holds the point itself (code 0)."""
    P = _Points()
    for v in NEG_VALUES:
        for a in range(3):
            p = BASE.copy(); p[a] = np.float32(v)
            c = _centre32(p)
            sgn = np.ones(3, np.int64)
            sgn[a] = 1 if v < 0 else -1                      # towards zero where truncation would pick the next cell
            if c[a] + sgn[a] * np.float32(0.25) == 0:        # (one float beyond 0 is a denormal and vanishes in c + 0.25)
                sgn[a] = -sgn[a]
            face = f32([c[b] + sgn[b] * np.float32(0.25) for b in range(3)])
            out = f32([nudge(face[b], int(sgn[b])) for b in range(3)])
            P.add(p, out, 1, 2, kind="beyond_all", axis=a)
            q = out.copy(); q[a] = face[a]
            P.add(p, q, 1, "not2", kind="face_eq", axis=a)
            P.add(p, p, 5, 0, kind="same_dist", axis=a)
    return P.case("negative_coordinates", mutants=("trunc",))


def _rotation(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q * np.sign(np.linalg.det(Q))


def pose(seed, t_scale=30.0):
    rng = np.random.default_rng(seed)
    T = np.eye(4)
    T[:3, :3] = _rotation(rng)
    T[:3, 3] = rng.uniform(-1.0, 1.0, 3) * t_scale
    return T.reshape(-1, order="F")


def _mixture(P, rng, n, T, fs, spread):
    """points all over +-spread with lists around their own cells: every count, every code"""
    src = f32(rng.uniform(-spread, spread, (n, 3)))
    pw = transform(src, T)
    c = centre(pw, fs)
    for i in range(n):
        cnt = int(rng.choice([0, 1, 2, 3, 4, 5, 5, 5, 5, 5, 5, 6, 7]))
        nn = c[i] + rng.uniform(-0.7, 0.7, (5, 3)) * fs
        if rng.random() < 0.3:
            nn[0] = c[i] + rng.choice([-1.0, 1.0], 3) * rng.uniform(0.52, 0.9, 3) * fs
        if rng.random() < 0.3:
            nn[int(rng.integers(0, 5))] = pw[i]  # the point is in the map already
        P.add(src[i], nn, cnt)


def _case_pose():
    rng, P = np.random.default_rng(7307), _Points()
    T = pose(7317)
    _mixture(P, rng, 200, T, FS, 60.0)
    return P.case("general_pose", T=T, mutants=("float_pw",))


def _case_nonfinite():
    """a NaN and an infinite source coordinate, under the identity (0 * inf = NaN reaches the other rows) and under a general pose"""
    P = _Points()
    c = _centre32(BASE)
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(3):
            p = BASE.copy(); p[a] = bad
            for cnt in (0, 1, 5):
                P.add(p, c, cnt, kind="nonfinite")
                P.add(p, c + f32(0.5), cnt, kind="nonfinite")
    P.add(BASE, c, 5)  # (a finite point in the same wave)
    return P


def _case_fs03():
    rng, P = np.random.default_rng(7309), _Points()
    _mixture(P, rng, 150, IDENT, 0.3, 25.0)
    for v in (-0.3, 0.3, -0.6, 0.9, -1e-7, 0.0, -0.0, 0.15, -0.15, -0.45):  # multiples of an fs that no float holds
        p = f32([v, -v, v])
        c = centre(p.reshape(1, 3), 0.3)[0]
        P.add(p, c + 0.15, 1); P.add(p, c - 0.15, 5); P.add(p, p, 5)
    return P.case("fs_0p3", fs=0.3)


def _sized(n, seed, T=IDENT):
    rng, P = np.random.default_rng(seed), _Points()
    _mixture(P, rng, n, T, FS, 40.0)
    return P.case("n%d" % n, T=T)


def _case_origin():
    """around the origin, where the row (0, 0, 0) a stale id turns into decides: on a face, nearer than the point, farther"""
    rng, P = np.random.default_rng(7311), _Points()
    _mixture(P, rng, 140, IDENT, FS, 0.6)
    return P.case("origin")


SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case}: the rule's inputs"""
    nf = _case_nonfinite()
    out = [_case_count0(), _case_low_counts(), _case_half_cell(), _case_distance_loop(), _case_bracket(), _case_negative(), _case_pose(),
           nf.case("nonfinite_identity"), nf.case("nonfinite_general_pose", T=pose(7318)), _case_fs03(), _case_origin(), _sized(70, 7340, pose(7341)),
           _sized(300, 7342), _sized(1100, 7343)]
    out += [_sized(n, 7320 + k, pose(7330 + k) if k % 2 else IDENT) for k, n in enumerate(SIZES)]
    assert len({c.name for c in out}) == len(out) and max(len(c.src) for c in out) <= 1100
    return {c.name: c for c in out}


RULE_CASES = ("count0_garbage_rows", "low_counts_all_nearer", "half_cell_faces", "distance_loop", "less_than_bracket", "negative_coordinates",
              "general_pose", "nonfinite_identity", "nonfinite_general_pose", "fs_0p3")


# ---------------------------------------------------------------- the launches ----------------------------------------------------------------
def _rows_u32(xyz, ids):
    """(k, 5, 3) float32 + (k, 5) ids -> (k, 5, 4) rows as uint32 words"""
    out = np.empty(xyz.shape[:2] + (4,), np.uint32)
    out[..., :3] = np.ascontiguousarray(xyz, np.float32).view(np.uint32)
    out[..., 3] = ids
    return out


def build_lists(c, form, n=None, nn_n=None, stale=0.0, seed=0):
    """The lists of case c as the kernel takes them.  form: "rows" (every list in rows form, no ids array, no map), "ids", or "mixed" (both
    inside every wave).  A list in rows form keeps its points in `rows`, and its ids row names slots that hold its flipper; a list in ids form
    keeps them in the map, and `rows` holds its flipper five times: whichever form is read in place of the other, the decision changes.  Words 5
    to 7 of every ids row name the slot of the flipper as well.  stale: the share of ids-form lists with ids in [n_slots, n_slots + MAP_PAD).
    n / nn_n: take the first n points and the first nn_n lists of the case (a list beyond n decides nothing, but still becomes rows).
    -> (src, rows (nn_n, 5, 4) uint32, cnt (nn_n,), ids (nn_n, 8) or None, map_rows (n_slots, 4) uint32 or None)"""
    rng = np.random.default_rng(9000 + seed)
    n = len(c.src) if n is None else n
    nn_n = len(c.src) if nn_n is None else nn_n
    nn, cnt = c.nn[:nn_n], c.cnt[:nn_n].copy()
    own_id = 1000 + np.arange(nn_n * 5, dtype=np.uint32).reshape(nn_n, 5)
    if form == "rows":
        return c.src[:n], _rows_u32(nn, own_id), cnt | ROWS_BIT, None, None
    flip = flippers(c.src[:nn_n], c.T, c.fs, nn, cnt)
    i = np.arange(nn_n)
    in_rows = ((i * 7) % 5 < 2) if form == "mixed" else np.zeros(nn_n, bool)
    slot = rng.permutation(nn_n * 6).astype(np.uint32).reshape(nn_n, 6)
    decoy = np.repeat(flip[:, None, :], 5, axis=1)
    map_rows = np.empty((nn_n * 6, 4), np.uint32)
    map_rows[slot[:, :5]] = np.where(in_rows[:, None, None], _rows_u32(decoy, 0x00C0FFEE), _rows_u32(nn, own_id))
    map_rows[slot[:, 5]] = _rows_u32(flip[:, None, :].repeat(5, axis=1), 0x00C0FFEE)[:, 0]
    rows = np.where(in_rows[:, None, None], _rows_u32(nn, own_id), _rows_u32(decoy, 7777))
    ids = np.concatenate([slot[:, :5], slot[:, 5:].repeat(3, axis=1)], axis=1)
    if stale:
        n_slots = len(map_rows)
        hit = (~in_rows) & (rng.random(nn_n) < stale)
        for j in np.flatnonzero(hit):
            k = rng.choice(5, size=int(rng.integers(1, 6)), replace=False)
            ids[j, k] = n_slots + rng.integers(0, MAP_PAD, len(k))
    return c.src[:n], rows, np.where(in_rows, cnt | ROWS_BIT, cnt).astype(np.uint8), ids, map_rows


def _launch(name, c, form, materialize, count=1, gate=None, T=None, stale=0.0, **kw):
    src, rows, cnt, ids, map_rows = build_lists(c, form, stale=stale, **kw)
    for a in (rows, cnt, ids, map_rows):
        if a is not None:
            a.setflags(write=False)
    return Launch(name, c.name, src, c.T if T is None else T, c.fs, rows, cnt, ids, map_rows, materialize, count, gate, stale)


def _gate(done, it, n_valid, max_it, T):
    return {"done": done, "iter": it, "n_valid": n_valid, "max_iterations": max_it, "T": T}


@functools.lru_cache(maxsize=None)
def launches():
    """{name: Launch}.  With materialize = 0 every id is in range: that form answers a stale id with slot 0, and the matcher never launches it
    with a list in ids form (include/fls_debug_ivox_decide.h)."""
    C, out = cases(), []
    for name in RULE_CASES:
        out.append(_launch(name + "/rows/m0", C[name], "rows", 0))
        out.append(_launch(name + "/mixed/m0", C[name], "mixed", 0, seed=1))
        out.append(_launch(name + "/mixed/m1", C[name], "mixed", 1, seed=2))
    out.append(_launch("origin/ids/m1", C["origin"], "ids", 1, seed=3))
    out.append(_launch("origin/stale/m1", C["origin"], "mixed", 1, stale=0.6, seed=4))
    out.append(_launch("origin/all_stale/m1", C["origin"], "ids", 1, stale=1.0, seed=5))
    for k, n in enumerate(SIZES):
        out.append(_launch("n%d/rows/m0" % n, C["n%d" % n], "rows", 0))
        out.append(_launch("n%d/mixed/m1" % n, C["n%d" % n], "mixed", 1, stale=0.2, seed=10 + k))
    # lists beyond the decided points still become rows; points beyond the lists decide as count 0
    out.append(_launch("n300_of_1100/mixed/m1", C["n1100"], "mixed", 1, n=300, nn_n=1100, stale=0.2, seed=20))
    out.append(_launch("n300_of_1100/mixed/m0", C["n1100"], "mixed", 0, n=300, nn_n=1100, seed=21))
    out.append(_launch("n300_lists100/mixed/m1", C["n300"], "mixed", 1, n=300, nn_n=100, stale=0.2, seed=22))
    out.append(_launch("n300_lists100/mixed/m0", C["n300"], "mixed", 0, n=300, nn_n=100, seed=23))
    out.append(_launch("n300_lists100/rows/m0", C["n300"], "rows", 0, n=300, nn_n=100))
    out.append(_launch("n300_no_lists/rows/m1", C["n300"], "rows", 1, n=300, nn_n=0))
    # no counting: lx, bt and the status words keep the fill
    out.append(_launch("n257/mixed/m1/nocount", C["n257"], "mixed", 1, count=0, stale=0.2, seed=24))
    out.append(_launch("n65/rows/m0/nocount", C["n65"], "rows", 0, count=0))
    # the speculative gate: the pose argument is NOT the pose of the update
    g, other = C["n70"], pose(7399)
    for tag, (done, it, nv, mx) in {"not_done": (0, 3, 500, 10), "done_49": (1, 3, 49, 10), "done_50": (1, 3, 50, 10), "max_iter_50": (0, 10, 50, 10),
                                    "max_iter_49": (0, 10, 49, 10), "past_max_iter": (0, 11, 51, 10)}.items():
        out.append(_launch("gate/" + tag, g, "mixed", 1, gate=_gate(done, it, nv, mx, g.T), T=other, stale=0.2, seed=30))
    assert len({l.name for l in out}) == len(out)
    for l in out:
        if not l.materialize and l.ids is not None:
            assert int(l.ids.max()) < len(l.map_rows), l.name
    return {l.name: l for l in out}


def gate_runs(g):
    return g is None or ((g["done"] != 0 or g["iter"] >= g["max_iterations"]) and g["n_valid"] >= MIN_VALID)


def grid_points(l):
    n, nn_n = len(l.src), len(l.cnt)
    return max(n, nn_n) if l.materialize else n


def materialized(l):
    """(gathered, rows, cnt): the rows the ids name -- (0, 0, 0, id -1) for an id beyond the map -- and the two list arrays as a materializing
    launch leaves them: an ids-form list becomes rows and gets the bit (its rows only with a count above 0), a rows-form list is untouched"""
    if l.ids is None:
        return None, l.rows.copy(), l.cnt.copy()
    n_slots = len(l.map_rows)
    w = l.ids[:, :5].astype(np.int64)
    gathered = np.where((w < n_slots)[:, :, None], l.map_rows[np.minimum(w, n_slots - 1)], STALE_ROW)
    ids_form = (l.cnt & ROWS_BIT) == 0
    rows = np.where((ids_form & ((l.cnt & 7) != 0))[:, None, None], gathered, l.rows)
    return gathered, rows, np.where(ids_form, l.cnt | ROWS_BIT, l.cnt).astype(np.uint8)


def rule_inputs(l):
    """what the rule sees of launch l: (nn (n, 5, 3) float32, cnt (n,) plain counts); a point without a list has count 0"""
    n, nn_n = len(l.src), len(l.cnt)
    gathered, _, _ = materialized(l)
    seen = l.rows if gathered is None else np.where(((l.cnt & ROWS_BIT) == 0)[:, None, None], gathered, l.rows)
    m = min(n, nn_n)
    nn, cnt = np.zeros((n, 5, 3), np.float32), np.zeros(n, np.uint8)
    nn[:m] = np.ascontiguousarray(seen[:m, :, :3]).view(np.float32)
    cnt[:m] = l.cnt[:m] & 7
    return nn, cnt


def fill(shape, dtype):
    """an output buffer as the hook prefills it on the device"""
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype).reshape(shape)


def expected(l, decide):
    """every output of launch l: code (n,), pw (n, 4) float32, rows, cnt, lx (n, 2), bt (blocks, 2), st (2,).  decide(src, T, fs, nn, cnt) ->
    (code, pw (n, 3)) is the rule (the oracle's); the rest is numpy."""
    n, m = len(l.src), grid_points(l)
    nb = (m + BLOCK - 1) // BLOCK
    out = {"code": fill(n, np.uint8), "pw": fill((n, 4), np.float32), "rows": l.rows.copy(), "cnt": l.cnt.copy(), "lx": fill((n, 2), np.uint32),
           "bt": fill((nb, 2), np.uint32), "st": fill(2, np.uint32)}
    if not gate_runs(l.gate):
        out["st"][:] = (SKIPPED, 0)
        return out
    nn, cnt = rule_inputs(l)
    code, pw = decide(l.src, l.T if l.gate is None else l.gate["T"], l.fs, nn, cnt)
    out["code"][:] = code
    out["pw"][:, :3] = pw
    out["pw"][:, 3] = 0.0
    if l.materialize:
        _, out["rows"], out["cnt"] = materialized(l)
    if l.count:
        one = np.stack([code == 1, code == 2], axis=1).astype(np.uint32)
        for b in range((n + BLOCK - 1) // BLOCK):  # a block that starts at or beyond n writes no total
            blk = one[b * BLOCK:(b + 1) * BLOCK]
            out["lx"][b * BLOCK:b * BLOCK + len(blk)] = np.cumsum(blk, axis=0) - blk
            out["bt"][b] = blk.sum(axis=0)
        out["st"][:] = 0
    return out
