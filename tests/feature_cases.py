"""Constructed range images, a sequential numpy model and named frames for tests/test_gpu_feature_stages.py: the LOAM feature front-end
(csrc/kernels_features.hpp) on inputs that reach the decisions a ray-cast scene reaches rarely or never.  tests/test_feature_cases.py checks,
without a GPU, that the model equals the oracle (oracle/flo_features.h) bit for bit on every frame and that every frame shows the property it
is named for.  Every cached array is read-only: the tests share it.

A frame is designed as a range image: (ring, column, depth) cells.  raw_from_image() turns it into a raw driver cloud whose points project into
exactly those cells with exactly those depth bits, so roughness values, ties and threshold equalities hold by construction: depths are multiples
of U = 2^-8 m around 20 m, where the ten-term float32 sum and 10 * d are exact.

The model is the reference's sequential walk (feature_extractor.cpp:65-222) in numpy, plus an event record per (ring, sector) that says what the
walk did there; it has no authority of its own, it is compared with the oracle first."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from funny_lidar_slam_amd import synth

F32, F64, I32, U32 = np.float32, np.float64, np.int32, np.uint32
U = F32(2.0 ** -8)          # the depth grid
D0 = F32(20.0)              # the flat depth of most rings
DT_A = synth.RAW_POINT_DTYPE
# a second driver layout: another stride, ring in front of xyz, intensity last
DT_B = np.dtype({"names": ["ring", "x", "y", "z", "time", "intensity"], "formats": ["<u2", "<f4", "<f4", "<f4", "<f4", "<f4"],
                 "offsets": [0, 4, 8, 12, 20, 36], "itemsize": 40})
SHRINKS = (0.9999, 0.9997, 0.9995, 0.999, 0.9985, 0.998)
_OFFS = np.arange(-64, 65, dtype=I32)


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def h_res_for(cols: int) -> float:
    return float(F32(2.0 * np.pi / cols))


def nextf(v, toward):
    return F32(np.nextafter(F32(v), F32(toward)))


# ---- the projector's arithmetic in numpy float32 ----------------------------------------------------------------------------------------
def fast_atan2_f32(y, x):
    """math_function.h:159-186 with Type = float (numpy's float32 +, *, / are single IEEE operations)"""
    y, x = np.asarray(y, F32), np.asarray(x, F32)
    p1, p3, p5, p7 = F32(0.9997878412794807), F32(-0.3258083974640975), F32(0.1555786518463281), F32(-0.04432655554792128)
    ax, ay = np.abs(x), np.abs(y)
    big = ax >= ay
    c = np.where(big, ay, ax) / (np.where(big, ax, ay) + F32(1.1920928955078125e-07))
    c2 = c * c
    poly = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(big, poly, F32(np.pi / 2) - poly)
    a = np.where(x < 0, F32(np.pi) - a, a)
    a = np.where(y < 0, F32(2 * np.pi) - a, a)
    return np.where(a > F32(np.pi), a - F32(2 * np.pi), a).astype(F32)


def col_index(x, y, h_res, cols):
    """pointcloud_projector.cpp:69-74: std::round is half away from zero; one wrap"""
    q = (fast_atan2_f32(y, x) / F32(h_res)).astype(F64)
    col = np.trunc(q + np.copysign(0.5, q)).astype(np.int64) + cols // 2
    return np.where(col >= cols, col - cols, col)


def depth_f32(x, y, z):
    x, y, z = np.asarray(x, F32), np.asarray(y, F32), np.asarray(z, F32)
    return np.sqrt((x * x + y * y) + z * z)


def raw_from_image(cells, cols, h_res, dtype=DT_A):
    """Raw cloud, one point per cell of `cells` in order: (ring, column, depth[, intensity[, variant]]).  The point sits at the column's centre
    azimuth, x and y shrunk by a factor just below one, z searched over neighbouring floats until sqrt((x x + y y) + z z) has exactly the depth's
    bits.  `variant` starts the search at another shrink factor, which gives another z for the same cell and depth.  Raises if a cell misses its
    depth bits or its column."""
    n = len(cells)
    ring = np.array([c[0] for c in cells], np.int64)
    col = np.array([c[1] for c in cells], np.int64)
    d = np.array([c[2] for c in cells], F32)
    inten = np.array([c[3] if len(c) > 3 else float(c[0] * 4096 + c[1]) for c in cells], F32)
    var = np.array([c[4] if len(c) > 4 else 0 for c in cells], np.int64)
    az = (col - cols // 2).astype(F64) * F64(F32(h_res))
    x, y, z = np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, F32)
    todo = np.ones(n, bool)
    for k in range(len(SHRINKS)):
        for v in np.unique(var[todo]):
            i = np.nonzero(todo & (var == v))[0]
            s = SHRINKS[(k + int(v)) % len(SHRINKS)]
            xs, ys = (d[i].astype(F64) * np.cos(az[i]) * s).astype(F32), (d[i].astype(F64) * np.sin(az[i]) * s).astype(F32)
            z2 = d[i].astype(F64) ** 2 - xs.astype(F64) ** 2 - ys.astype(F64) ** 2
            z0 = np.sqrt(np.maximum(z2, 0.0)).astype(F32)
            zc = (z0.view(I32)[:, None] + _OFFS[None, :]).view(F32)
            hit = np.sqrt((xs * xs + ys * ys)[:, None] + zc * zc).view(U32) == d[i].view(U32)[:, None]
            hit &= (col_index(xs, ys, h_res, cols) == col[i])[:, None]
            ok = hit.any(axis=1)
            j = i[ok]
            x[j], y[j], z[j] = xs[ok], ys[ok], zc[ok, hit[ok].argmax(axis=1)]
            todo[j] = False
        if not todo.any():
            break
    if todo.any():
        raise ValueError(f"raw_from_image: {int(todo.sum())} of {n} cells missed their depth bits, first {cells[int(np.nonzero(todo)[0][0])]}")
    raw = np.zeros(n, dtype=dtype)
    raw["x"], raw["y"], raw["z"], raw["intensity"], raw["ring"] = x, y, z, inten, ring.astype(np.uint16)
    return raw


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def project_model(raw, p):
    """PointcloudProjector::Project (:32-133): first point of the stream wins its cell, cells in (ring, column) order"""
    rows, cols = p["vertical_scan"], p["horizontal_scan"]
    x, y, z = raw["x"], raw["y"], raw["z"]
    d = depth_f32(x, y, z)
    c = col_index(x, y, p["horizontal_resolution"], cols)
    ring = raw["ring"].astype(np.int64)
    keep = (d >= F32(p["min_distance"])) & (d <= F32(p["max_distance"])) & (ring < rows) & (c >= 0) & (c < cols)
    k = np.nonzero(keep)[0]
    cell, first = np.unique(ring[k] * cols + c[k], return_index=True)
    win = k[first]
    cnt = np.bincount(cell // cols, minlength=rows)
    base = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    ordered = np.stack([x[win], y[win], z[win], raw["intensity"][win]], axis=1).astype(F32).reshape(-1, 4)
    return dict(ordered=ordered, depth=d[win].astype(F32), col=(cell % cols).astype(I32), raw_index=win.astype(I32),
                row_start=(base + 5).astype(I32), row_end=(base + cnt - 6).astype(I32))


def flags_model(d, col):
    """ComputeRoughness (:48-62) and SelectValidPoints (:65-117), as tests/test_oracle_features.py writes them out, plus which rule fired where:
    rule_a[j]: d[j] - d[j+1] > 0.3, rule_b[j]: d[j+1] - d[j] > 0.3 (both under a column difference below 10), rule_c[j]: both neighbour
    differences above 0.02 d[j]; diff_a / diff_b / f1 / f2 / cd are the compared values; hits counts the rules that zeroed each flag."""
    n = len(d)
    rough = np.zeros(n, F32)
    valid = np.ones(n, np.uint8)
    ev = dict(rule_a=np.zeros(n, bool), rule_b=np.zeros(n, bool), rule_c=np.zeros(n, bool), diff_a=np.zeros(n, F32), diff_b=np.zeros(n, F32),
              f1=np.zeros(n, F32), f2=np.zeros(n, F32), cd=np.zeros(n, np.int64), hits=np.zeros(n, np.int64))
    if n < 12:
        return rough, valid, ev
    i = np.arange(5, n - 5)
    acc = d[i - 5].copy()
    for k in (-4, -3, -2, -1, 1, 2, 3, 4, 5):
        acc = (acc + d[i + k]).astype(F32)
    r = (acc - F32(10.0) * d[i]).astype(F32)
    rough[5:n - 5] = (r * r).astype(F32)
    valid[:5] = 0
    valid[n - 6:] = 0
    c = col.astype(np.int64)
    for j in range(5, n - 6):
        ev["cd"][j] = abs(c[j + 1] - c[j])
        ev["diff_a"][j], ev["diff_b"][j] = F32(d[j] - d[j + 1]), F32(d[j + 1] - d[j])
        ev["f1"][j], ev["f2"][j] = F32(abs(F32(d[j - 1] - d[j]))), F32(abs(F32(d[j + 1] - d[j])))
        if ev["cd"][j] < 10:
            if float(ev["diff_a"][j]) > 0.3:
                ev["rule_a"][j] = True
                valid[j - 5:j + 1] = 0
                ev["hits"][j - 5:j + 1] += 1
            elif float(ev["diff_b"][j]) > 0.3:
                ev["rule_b"][j] = True
                valid[j + 1:j + 7] = 0
                ev["hits"][j + 1:j + 7] += 1
        if float(ev["f1"][j]) > 0.02 * float(d[j]) and float(ev["f2"][j]) > 0.02 * float(d[j]):
            ev["rule_c"][j] = True
            valid[j] = 0
            ev["hits"][j] += 1
    return rough, valid, ev


def _new_events():
    return dict(t=0, cap_hit=False, corners=0, b1_corner=False, b1_candidate_invalid=False, b1_planar_accept=False, b1_planar_emitted=False,
                b0_planar_again=False, cuts=set(), passed10=set(), both_sides=set(), ahead=set(), accept_lanes={"corner": set(), "planar": set()},
                accept_chunks={"corner": set(), "planar": set()},
                ties_corner=0, ties_planar=0, eq_corner_thr=0, eq_planar_thr=0)


def select_model(pr, p, rough, valid_pre):
    """SelectFeatures (:119-222), ties in ascending position (the oracle's sort_mode 0).  Returns the arrays and events[(ring, sector)]:
      cap_hit                 a 21st valid candidate above the corner threshold was met (the walk broke there)
      b1_corner / b1_candidate_invalid / b1_planar_accept / b1_planar_emitted / b0_planar_again
                              what happened to the unsorted boundary element b1, and whether this sector emitted its b0 a second time
      cuts                    (loop, 'f' | 'b', k, step): a suppression stopped at offset k on that side because of a column step above 10
      passed10                (loop, 'f' | 'b', k): a suppression went on over a column step of exactly 10 at offset k
      both_sides              (loop, kf, kb): one suppression cut on both sides
      ahead                   (loop, 'same' | 'later', taken, side): a suppression cleared a still valid element that the walk had yet to
                              visit, in the accepting element's 64-element chunk or a later one; taken: it passed the loop's threshold, so
                              the walk would have accepted it; side: below ('lo') or above ('hi') the accepting position
      accept_lanes / accept_chunks   the lanes (walk index mod 64) and chunks (walk index / 64) of the accepted elements, per loop
      ties_corner / ties_planar   adjacent pairs of equal roughness in the sorted sector above the corner / below the planar threshold
      eq_corner_thr / eq_planar_thr   sector elements whose roughness equals a threshold"""
    col = pr["col"].astype(np.int64)
    n = len(col)
    cthr, pthr = F32(p["corner_thres"]), F32(p["planar_thres"])
    v = valid_pre.copy()
    is_corner = np.zeros(n, np.uint8)
    corner_idx, planar_idx = [], []
    events = {}
    if n < 12:
        return dict(valid_post=v, is_corner=is_corner, corner_idx=np.zeros(0, I32), planar_idx=np.zeros(0, I32)), events

    def suppress(q, e, loop, ev, pos, length):
        nf = nb = 5
        for k in range(1, 6):
            step = abs(col[q + k] - col[q + k - 1])
            if step > 10:
                nf = k - 1
                ev["cuts"].add((loop, "f", k, int(step)))
                break
            if step == 10:
                ev["passed10"].add((loop, "f", k))
        for k in range(1, 6):
            step = abs(col[q - k] - col[q - k + 1])
            if step > 10:
                nb = k - 1
                ev["cuts"].add((loop, "b", k, int(step)))
                break
            if step == 10:
                ev["passed10"].add((loop, "b", k))
        if nf < 5 and nb < 5:
            ev["both_sides"].add((loop, nf + 1, nb + 1))
        w = (length - e) if loop == "corner" else e
        ev["accept_lanes"][loop].add(w % 64)
        ev["accept_chunks"][loop].add(w // 64)
        for q2 in range(q - nb, q + nf + 1):
            if q2 != q and v[q2] and q2 in pos:
                e2 = pos[q2]
                if (e2 < e) if loop == "corner" else (e2 > e):
                    w2 = (length - e2) if loop == "corner" else e2
                    taken = bool(rough[q2] > cthr) if loop == "corner" else bool(rough[q2] < pthr)
                    ev["ahead"].add((loop, "same" if w2 // 64 == w // 64 else "later", taken, "lo" if q2 < q else "hi"))
            v[q2] = 0

    for ring in range(p["vertical_scan"]):
        rs, re_ = int(pr["row_start"][ring]), int(pr["row_end"][ring])
        t = int((re_ - rs) / 6)  # truncating, like the reference's int division
        for s in range(6):
            b0, b1 = rs + s * t, rs + (s + 1) * t
            if b0 >= b1:
                continue
            ev = events[(ring, s)] = _new_events()
            ev["t"] = t
            order = np.arange(b0, b1)[np.argsort(rough[b0:b1], kind="stable")]
            walk = [int(q) for q in order] + [b1]
            pos = {q: e for e, q in enumerate(walk)}
            rsort = rough[order]
            eq = rsort[1:] == rsort[:-1]
            ev["ties_corner"], ev["ties_planar"] = int((eq & (rsort[1:] > cthr)).sum()), int((eq & (rsort[1:] < pthr)).sum())
            ev["eq_corner_thr"], ev["eq_planar_thr"] = int((rough[b0:b1 + 1] == cthr).sum()), int((rough[b0:b1 + 1] == pthr).sum())
            if rough[b1] > cthr and not v[b1]:
                ev["b1_candidate_invalid"] = True
            large = 0
            for e in range(t, -1, -1):
                q = walk[e]
                if rough[q] > cthr and v[q]:
                    large += 1
                    if large > 20:
                        ev["cap_hit"] = True
                        break
                    is_corner[q] = 1
                    corner_idx.append(q)
                    ev["corners"] += 1
                    if q == b1:
                        ev["b1_corner"] = True
                    suppress(q, e, "corner", ev, pos, t)
            for e in range(0, t + 1):
                q = walk[e]
                if v[q] and rough[q] < pthr:
                    if q == b1:
                        ev["b1_planar_accept"] = True
                    suppress(q, e, "planar", ev, pos, t)
                if not is_corner[q]:
                    planar_idx.append(q)
                    if q == b1:
                        ev["b1_planar_emitted"] = True
                    if q == b0 and s > 0 and events.get((ring, s - 1), {}).get("b1_planar_emitted"):
                        ev["b0_planar_again"] = True
    return dict(valid_post=v, is_corner=is_corner, corner_idx=np.array(corner_idx, I32).reshape(-1),
                planar_idx=np.array(planar_idx, I32).reshape(-1)), events


def model(raw, p):
    """Every array the front-end returns (the names of FeatureFrontEnd.get), the flag events and the selection events"""
    pr = project_model(raw, p)
    rough, valid_pre, fev = flags_model(pr["depth"], pr["col"])
    sel, events = select_model(pr, p, rough, valid_pre)
    out = dict(pr, roughness=rough, valid_pre=valid_pre, **sel)
    out["corner"], out["planar"] = pr["ordered"][sel["corner_idx"]], pr["ordered"][sel["planar_idx"]]
    return out, fev, events


def merged(events, key):
    """union of a set-valued event over all sectors"""
    out = set()
    for ev in events.values():
        out |= ev[key]
    return out


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
class Frame(NamedTuple):
    raw: np.ndarray
    params: dict    # the arguments of OracleFeatures
    info: dict      # what the property tests need


def _params(rows, cols, h_res=None, min_distance=4.0, max_distance=100.0, corner_thres=1.0, planar_thres=0.1):
    return dict(vertical_scan=rows, horizontal_scan=cols, horizontal_resolution=h_res_for(cols) if h_res is None else float(h_res),
                min_distance=float(min_distance), max_distance=float(max_distance), corner_thres=float(corner_thres),
                planar_thres=float(planar_thres))


def image_frame(rings, cols, rows=None, dtype=DT_A, shuffle=None, info=None, **kw):
    """rings: {ring: (columns, depths)}.  The cloud is emitted in (ring, column) order, or permuted with the seed `shuffle`."""
    rows = (max(rings) + 1 if rings else 1) if rows is None else rows
    p = _params(rows, cols, **kw)
    cells = [(r, int(c), F32(d)) for r in sorted(rings) for c, d in zip(*rings[r])]
    for r, (c, d) in rings.items():
        assert len(c) == len(d) and (np.diff(c) > 0).all() and (len(c) == 0 or (c[0] >= 0 and c[-1] < cols)), (r, len(c), len(d))
    raw = raw_from_image(cells, cols, p["horizontal_resolution"], dtype) if cells else np.zeros(0, dtype)
    if shuffle is not None:
        raw = raw[np.random.default_rng(shuffle).permutation(len(raw))]
    return Frame(_ro(raw), p, dict(info or {}, cells=len(cells)))


def flat(n, d=D0):
    return np.full(n, d, F32)


def spike(d, i, k):
    """raise d[i] by k grid units"""
    d[i] = F32(d[i] + F32(k) * U)


def columns(n, gaps=None, start=0):
    """n ascending columns from `start`, step 1 except gaps[i] = the step from position i - 1 to position i"""
    step = np.ones(n, np.int64)
    step[0] = start
    for i, g in (gaps or {}).items():
        step[i] = g
    return np.cumsum(step)


def _cap(cols=1800, rows=None):
    """ring 0 and ring 2 (ring 1 empty, so the second ring's base is not zero), t = 256: sectors with 19, 20, 21, 40, 0, 0 spikes of distinct
    height six apart, every one a valid candidate above the threshold"""
    t = 256
    n = 11 + 6 * t
    rings = {}
    want = {}
    for ring, shift in ((0, 0), (2, 3)):
        d = flat(n)
        for s, m in enumerate((19, 20, 21, 40, 0, 0)):
            # heights 28..76 units, the lowest first in position so that position order and roughness order differ
            hs = np.random.default_rng(10 * ring + s).permutation(np.arange(28, 28 + m))
            for j in range(m):
                spike(d, 5 + s * t + 6 + shift + 6 * j, int(hs[j]))
            want[(ring, s)] = m
        rings[ring] = (columns(n), d)
    return image_frame(rings, cols, rows=rows, info=dict(candidates=want))


def _boundary():
    """t = 16, planar_thres 2^-5.  Ring 1 (11 + 6 t + 5 cells: the last sector's b1 is followed by the unsectored remainder), its six b1:
    the sector's largest roughness and valid; above the threshold and invalid (a 0.5 m spike: both flag rules); flat (below planar_thres, a
    column step of 11 in front of it, or the planar walk's earlier elements would clear it before its turn); a spike's neighbour (neither
    corner nor planar candidate); a valid spike lower than another of its sector; a valid spike in the last sector.  Ring 0 (11 + 6 t cells):
    the last b1 is row_end itself."""
    t = 16
    rings = {}
    for ring, extra in ((0, 0), (1, 5)):
        n = 11 + 6 * t + extra
        d = flat(n)
        b1 = [5 + (s + 1) * t for s in range(6)]
        spike(d, b1[0], 76)
        spike(d, b1[0] - 8, 40)
        spike(d, b1[1], 128)
        spike(d, b1[1] + 7, 50)
        spike(d, b1[3] + 2, 64)
        spike(d, b1[4], 40)
        spike(d, b1[4] - 7, 70)
        spike(d, b1[5], 60)
        rings[ring] = (columns(n, {b1[2]: 11}), d)
    return image_frame(rings, 900, planar_thres=2.0 ** -5, info=dict(t=t))


GAP_KINDS = [(kind, k, g) for kind in ("f", "b", "fb") for k in range(1, 6) for g in (10, 11)]


def _gaps():
    """t = 100, five groups per sector: A (70 units) at q, B (50) at q + k and / or C (40) at q - k, the column step of 10 or 11 right in
    front of B / behind C: at 11 the suppression of A stops there and B / C is accepted later, at 10 it is cleared.  planar_thres 2^-5, so
    the spikes' neighbours are neither kind of candidate and keep their flag unless a suppression reaches them."""
    t = 100
    n = 11 + 6 * t
    d = flat(n)
    gaps = {}
    where = {}
    for m, (kind, k, g) in enumerate(GAP_KINDS):
        q = 5 + (m // 5) * t + 10 + 20 * (m % 5)
        spike(d, q, 70)
        if "f" in kind:
            spike(d, q + k, 50)
            gaps[q + k] = g
        if "b" in kind:
            spike(d, q - k, 40)
            gaps[q - k + 1] = g
        where[(kind, k, g)] = q
    c = columns(n, gaps)
    rings = {1: (c, d)}
    # rings 2..4, for the planar walk: blocks set apart by column steps of 20, each a flat run, a 20-unit zigzag of 1..6 cells (roughness
    # between the thresholds: never accepted, so their flags show which suppressions reached them), a flat run; one column step of 10 or 11
    # somewhere around the zigzag.  Every block comes twice, once with either step, so the pair differs in that decision alone.
    rng = np.random.default_rng(5)
    blocks = 0
    for ring in (2, 3, 4):
        dd, gg = [F32(20.0)] * 8, {}
        while len(dd) < 1100:
            L, w, R = int(rng.integers(6, 13)), int(rng.integers(1, 7)), int(rng.integers(6, 13))
            at = int(rng.integers(L - 3, L + w + 4))
            for g in (10, 11):
                gg[len(dd)] = 20
                gg[len(dd) + at] = g
                dd += [D0] * L + [F32(D0 + F32(20) * U) if k % 2 == 0 else D0 for k in range(w)] + [D0] * R
                blocks += 1
        gg[len(dd)] = 20
        dd += [D0] * 8
        rings[ring] = (columns(len(dd), gg), np.array(dd, F32))
    return image_frame(rings, 4096, rows=5, planar_thres=2.0 ** -5, info=dict(where=where, blocks=blocks))


CHUNK_LENGTHS = {"chunks_a": (1, 2, 62, 63, 64, 65), "chunks_b": (127, 128, 129, 255, 256, 257), "chunks_c": (512, 680)}
CHUNK_COLS = {"chunks_a": 512, "chunks_b": 1800, "chunks_c": 4096}


def _chunk_ring(t, extra):
    """One ring of sector length t: depths and column steps.  Per sector, from its start: a filler that occupies the top of the corner walk
    behind b1 without being accepted, so the first real candidate sits F + 1 lanes in: either F spikes of 0.5 m six apart (roughness 25, every
    one invalid together with its ten neighbours) or, where the sector is too short for 60 of those, a 1 m zigzag (every cell invalid,
    roughness about 36); then groups A (high) with lower spikes B at +2 / +4 and C at -3 that A's suppression clears while they are still ahead
    in the walk; the rest flat, where the planar walk accepts every sixth element and clears the five behind it, across chunk edges too.
    t = 63, 64, 65: sector 0 is a 0.25 m zigzag, a plateau of valid candidates, the walk accepts every sixth down to its last chunk, and a
    column step of 11 behind b0 keeps b0 for the walk's last lane.  t = 128, 257: sector 5 is such a plateau too: the cap breaks the walk in
    its second chunk."""
    n = 11 + 6 * t + extra
    d = flat(n)
    gaps = {}
    if t < 8:
        if t == 2:
            spike(d, 5 + 1, 60)   # (in sector 0: its planar walk clears whatever lies within five cells before a later sector's turn)
        return d, gaps
    for s in range(6):
        b0 = 5 + s * t
        if (t in (63, 64, 65) and s == 0) or (t in (128, 257) and s == 5):
            d[max(b0 - 6, 0):b0 + t + 6:2] = F32(20.25)   # (past both ends: every cell of the sector sees the full pattern)
            gaps[b0 + 1] = 11
            continue
        if t < 100:
            f = ((0, 1, 2, 3, 4, 5), (5, 4, 3, 2, 1, 0), (0, 2, 4, 6, 1, 3), (1, 0, 3, 2, 5, 4))[t % 4][s]
            used = 6 + 6 * f
        elif t < 500:
            f = 0
            z = 0 if s == 0 else 52 + (t + 3 * s) % 14       # 52 .. 65 cells of zigzag
            d[b0 + 8:b0 + 8 + z:2] = F32(21.0)
            used = 8 + z + (6 if z else 0)
        else:
            f = (0, 61, 62, 63, 60, 3)[s]
            used = 6 + 6 * f
        for j in range(f):
            spike(d, b0 + 6 + 6 * j, 128)
        q = b0 + used + 8
        h = 76
        while q + 12 < b0 + t - 6 and h > 40:
            spike(d, q, h)
            spike(d, q + 2 + 2 * (h % 2), h - 14)
            spike(d, q - 3, h - 20)
            q += 17 + (h % 5)
            h -= 3
    return d, gaps


def _chunks(name):
    rings = {}
    for r, t in enumerate(CHUNK_LENGTHS[name]):
        d, gaps = _chunk_ring(t, 5 if (r % 2 or t == 680) else 0)
        rings[r] = (columns(len(d), gaps), d)
    return image_frame(rings, CHUNK_COLS[name], shuffle=7, info=dict(lengths=CHUNK_LENGTHS[name]))


def _ties():
    """ring 0: 20 m with a +0.25 m spike at every eighth column, a full 1800-column ring; ring 1: a 0.25 m zigzag, every element of every
    sector at roughness 2.25 and valid (a plateau above the corner threshold); ring 2: flat (a plateau below the planar threshold) with equal
    spikes six apart in two sectors, 49 tied candidates for 20 places"""
    n = 1800
    a = flat(n)
    a[::8] = F32(20.25)
    b = flat(n)
    b[1::2] = F32(20.25)
    c = flat(n)
    t = (n - 11) // 6
    for s in (1, 4):
        for j in range(49):
            spike(c, 5 + s * t + 3 + 6 * j, 64)
    return image_frame({0: (columns(n), a), 1: (columns(n), b), 2: (columns(n), c)}, 1800, info=dict(t=t))


TH_CORNER, TH_PLANAR = 1.5625, 2.0 ** -10   # (10 * 32 U)^2 and (8 U)^2: exact on the depth grid


def _thresholds(nxt):
    """Isolated groups of 11 cells (column steps of 11 on either side keep every outside suppression out).  Group kinds: a 32-unit spike,
    roughness exactly 1.5625; an 8-unit bump, roughness 0.09765625 with ten neighbours at exactly 2^-10.  With the thresholds AT those values
    nothing is selected and the groups keep their flags; with corner_thres one float below and planar_thres one float above, the spike is a
    corner and the neighbours are accepted as planar and clear the group."""
    groups = 12
    n = 11 + 6 * 22 + 5
    d = flat(n)
    gaps = {}
    centres = []
    for g in range(groups):
        q = 12 + 11 * g
        centres.append((q, "corner" if g % 2 == 0 else "planar"))
        spike(d, q, 32 if g % 2 == 0 else 8)
        gaps[q - 5] = 11
        gaps[q + 6] = 11
    corner, planar = (nextf(TH_CORNER, 0.0), nextf(TH_PLANAR, 1.0)) if nxt else (F32(TH_CORNER), F32(TH_PLANAR))
    return image_frame({0: (columns(n, gaps), d)}, 900, corner_thres=float(corner), planar_thres=float(planar), info=dict(centres=centres))


SHORT_COUNTS = (0, 1, 5, 6, 10, 11, 12, 16, 17, 18)


def _short_ring(n, seed):
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, F32)
    d = flat(n)
    if n >= 12:
        spike(d, 5 + (seed % max(n - 11, 1)), 60)
    return columns(n, start=seed % 7), d


def _short_rings(order):
    """rings of 0, 1, 5, 6, 10, 11, 12, 16, 17 and 18 cells (row_end < row_start, t = 0 and the first t = 1) around full 257-cell rings:
    'a': full ring first, 'b': full ring last, 'c': full rings in between"""
    full = lambda k: (columns(257), np.where(np.arange(257) % 9 == k, F32(20.25), D0).astype(F32))
    rings = {}
    shorts = [_short_ring(n, 3 * k + 1) for k, n in enumerate(SHORT_COUNTS)]
    if order == "a":
        seq = [full(2)] + shorts
    elif order == "b":
        seq = shorts[::-1] + [full(4)]
    else:
        seq = shorts[:4] + [full(1)] + shorts[4:7] + [full(6)] + shorts[7:]
    for r, (c, d) in enumerate(seq):
        if len(c):
            rings[r] = (c, d)
    return image_frame(rings, 257, rows=len(seq), info=dict(counts=[len(c) for c, _ in seq]))


def _tiny(total, cols=257):
    """11 (no extraction) or 12 (the smallest cloud the extractor runs on) ordered points over four rings, one of them empty"""
    counts = (3, 0, 4, total - 7)
    rings = {r: (columns(n, start=5 * r), flat(n)) for r, n in enumerate(counts) if n}
    return image_frame(rings, cols, rows=4, info=dict(counts=list(counts)))


def _flags():
    """feat_valid_rough_kernel's comparisons, min_distance 2^-4 so that depths below 0.5 m (float spacing 2^-25) can carry a difference of
    exactly float32(0.3).  Ring 0, flat segments of 16 cells; between segment m and m + 1 the depth steps by the probe's difference, down
    (rule a) or up (rule b): float32(0.3) exactly (marks: it is above the double 0.3), the float below (no mark), under a column step of 1, 9
    (marks) and 10 (does not); in front of them a step whose mark reaches into the first five cells of the cloud.  Ring 1 at 25 m, isolated by column steps of 10: both neighbours 0.5 m = 0.02 * 25 away (no mark: the
    comparison is strict), one float further (mark), one of them one float nearer (no mark); then the same without the isolation, where rules a
    and c zero the same flags.  Ring 2 starts five columns before ring 1 ends, 0.5 m nearer: a mark across the ring boundary; its last step
    sits seven cells before the end of the cloud and marks into the last six."""
    f03 = F32(0.3)
    lo, hi = F32(0.125), F32(F32(0.125) + f03)
    assert F32(hi - lo) == f03 and float(f03) > 0.3 and float(nextf(f03, 0.0)) < 0.3
    probes = [("a", hi, 1, True), ("a", nextf(hi, 0.0), 1, False), ("b", hi, 1, True), ("b", nextf(hi, 0.0), 1, False),
              ("a", hi, 9, True), ("a", hi, 10, False), ("b", hi, 9, True), ("b", hi, 10, False)]
    d0, gaps0, info = [hi] * 8 + [lo] * 12, {}, []   # a step down between cells 7 and 8: rule a marks cells 2 .. 7, into the first five
    for m, (rule, top, step, marks) in enumerate(probes):
        first, second = (top, lo) if rule == "a" else (lo, top)
        j = len(d0) + 15                      # the last cell of the first half: the step is between j and j + 1
        d0 += [first] * 16 + [second] * 16
        if step > 1:
            gaps0[j + 1] = step
        info.append((rule, j, step, marks))
    d0 = np.array(d0, F32)
    # ring 1: probes of rule c around 25 m
    up, dn = F32(25.5), F32(24.5)
    trip = [(up, dn, False), (nextf(up, 100.0), nextf(dn, 0.0), True), (nextf(up, 100.0), nextf(dn, 100.0), False), (nextf(up, 0.0), nextf(dn, 0.0), False),
            (up, up, False), (nextf(up, 100.0), nextf(up, 100.0), True)]
    d1, gaps1, cinfo = [], {}, []
    for isolated in (True, False):
        for (l, r, marks) in trip:
            j = len(d1) + 8
            d1 += [F32(25.0)] * 8 + [F32(25.0)] + [F32(25.0)] * 8
            d1[j - 1], d1[j + 1] = l, r
            if isolated:
                for g in (j - 1, j, j + 1, j + 2):
                    gaps1[g] = 10
            cinfo.append((j, isolated, marks))
    d1 = np.array(d1, F32)
    c1 = columns(len(d1), gaps1, start=3)
    # ring 2: begins within ten columns of ring 1's last column, 0.5 m nearer; ends with a step up seven cells before the end
    d2 = np.array([F32(24.5)] * 27 + [F32(25.0)] * 6, F32)
    c2 = columns(len(d2), start=int(c1[-1]) - 5)
    rings = {0: (columns(len(d0), gaps0), d0), 1: (c1, d1), 2: (c2, d2)}
    return image_frame(rings, 1800, min_distance=2.0 ** -4, info=dict(probes=info, cprobes=cinfo, n0=len(d0), n1=len(d1), n2=len(d2)))


# ---- projection frames ----------------------------------------------------------------------------------------------------------------------
def _gates():
    """depth exactly min_distance and max_distance (kept), one float outside each (dropped), one inside each"""
    lo, hi = F32(4.0), F32(100.0)
    ds = [lo, nextf(lo, 0.0), nextf(lo, 100.0), hi, nextf(hi, 1000.0), nextf(hi, 0.0)]
    cells = [(0, 10 + 3 * k, d) for k, d in enumerate(ds)] + [(0, 100 + k, D0) for k in range(12)]
    p = _params(1, 257)
    return Frame(_ro(raw_from_image(cells, 257, p["horizontal_resolution"])), p, dict(kept=[True, False, True, True, False, True]))


def _every_column(cols, rows=2):
    """every column at its centre, in ring 0 ascending and in the last ring descending (rows = 1: one ring)"""
    rings = {0: (columns(cols), flat(cols))}
    if rows > 1:
        rings[rows - 1] = (columns(cols), np.where(np.arange(cols) % 7 == 3, F32(20.25), D0).astype(F32))
    return image_frame(rings, cols, rows=rows, shuffle=cols, info=dict(cols=cols))


def _edges():
    """azimuths one part in 10^6 either side of every cell edge of 257 columns, x < 0 with y = +-0.0, x = y = 0 with z != 0, rings equal to
    `rows` and 65535 (dropped).  Compared with the oracle only: which side of an edge a point falls on is the polynomial's business."""
    cols, rows = 257, 3
    p = _params(rows, cols)
    h = p["horizontal_resolution"]
    az = ((np.arange(cols) - cols // 2 + 0.5) * h)[:, None] * np.array([1 - 1e-6, 1 + 1e-6])[None, :]
    az = az.reshape(-1)
    raw = np.zeros(len(az) + 8, DT_A)
    raw["x"][:len(az)], raw["y"][:len(az)] = (20 * np.cos(az)).astype(F32), (20 * np.sin(az)).astype(F32)
    raw["ring"][:len(az)] = np.arange(len(az)) % 2
    k = len(az)
    raw["x"][k:k + 2], raw["y"][k:k + 2], raw["ring"][k:k + 2] = -10.0, (0.0, -0.0), 2
    raw["z"][k + 2:k + 4], raw["ring"][k + 2:k + 4] = (10.0, -10.0), (2, 1)
    raw["x"][k + 4:k + 8], raw["y"][k + 4:k + 8], raw["ring"][k + 4:k + 8] = 10.0, (1.0, 2.0, 3.0, 4.0), (rows, 65535, rows + 1, 2)
    raw["intensity"] = np.arange(len(raw))
    return Frame(_ro(raw), p, dict(dropped_rings=3))


def _h_res(kind):
    """an h_res that does not match the column count: 'fine' (a quarter of 2 pi / cols: columns fall below 0 and stay >= cols after the single
    wrap), 'coarse' (four times: only the middle columns are used)"""
    cols, rows = 256, 2
    h = h_res_for(cols) * (0.25 if kind == "fine" else 4.0)
    p = _params(rows, cols, h_res=h)
    az = (np.arange(1024) + 0.25) * (2 * np.pi / 1024) - np.pi
    raw = np.zeros(len(az), DT_A)
    raw["x"], raw["y"], raw["z"] = (20 * np.cos(az)).astype(F32), (20 * np.sin(az)).astype(F32), 1.0
    raw["ring"] = np.arange(len(az)) % 2
    raw["intensity"] = np.arange(len(raw))
    q = (fast_atan2_f32(raw["y"], raw["x"]) / F32(h)).astype(F64)
    c = np.trunc(q + np.copysign(0.5, q)).astype(np.int64) + cols // 2
    return Frame(_ro(raw), p, dict(below=int((c < 0).sum()), beyond=int((c >= 2 * cols).sum()), wrapped=int(((c >= cols) & (c < 2 * cols)).sum())))


def _returns(dtype=DT_A):
    """2 to 9 returns per cell, differing in intensity and z; the stream is laid out so that the first (winning) return of a cell and its
    later returns lie in different 256-thread blocks, winners not in stream order of the cells.  Occupied cells alone at columns 63, 64, 255,
    256, 257 and cols - 1 in ring 2 (the edges of the compaction's ballots)."""
    cols, rows = 900, 128
    p = _params(rows, cols)
    cells = []
    ncell = 300
    for m in range(9):  # return m of cell k sits at stream index 300 m + perm_m(k): for most cells no later return shares the winner's block of 256
        perm = np.random.default_rng(40 + m).permutation(ncell)
        for k in perm:
            if m < 2 + k % 8:
                ring = (0, 1, 127)[k % 3]
                cells.append((ring, 3 * (k // 3) + 7, D0 + F32(k % 5) * U, float(1000 * m + k), m % len(SHRINKS)))
            else:
                cells.append((126, 100 + int(k), D0, float(-k), 0))  # a filler keeps the stream positions
    cells += [(2, c, D0) for c in (63, 64, 255, 256, 257, cols - 1)]
    raw = raw_from_image(cells, cols, p["horizontal_resolution"], dtype)
    return Frame(_ro(raw), p, dict(ncell=ncell))


FRAMES = {
    "cap": _cap, "boundary": _boundary, "gaps": _gaps,
    "chunks_a": lambda: _chunks("chunks_a"), "chunks_b": lambda: _chunks("chunks_b"), "chunks_c": lambda: _chunks("chunks_c"),
    "ties": _ties, "thresholds_eq": lambda: _thresholds(False), "thresholds_next": lambda: _thresholds(True),
    "short_rings_a": lambda: _short_rings("a"), "short_rings_b": lambda: _short_rings("b"), "short_rings_c": lambda: _short_rings("c"),
    "tiny11": lambda: _tiny(11), "tiny12": lambda: _tiny(12), "flags": _flags,
    "gates": _gates, "columns64": lambda: _every_column(64), "columns257": lambda: _every_column(257), "columns900": lambda: _every_column(900),
    "columns1800": lambda: _every_column(1800), "columns4096_one_row": lambda: _every_column(4096, rows=1), "edges": _edges,
    "h_res_fine": lambda: _h_res("fine"), "h_res_coarse": lambda: _h_res("coarse"), "returns": _returns, "returns_layout_b": lambda: _returns(DT_B),
}
# one handle, frame after frame (same rows, columns and thresholds): a fully occupied 4096-column frame, 11 points, nothing, then `cap`
REUSE = {"reuse_full": lambda: _every_column(4096, rows=4), "reuse_tiny11": lambda: _tiny(11, cols=4096),
         "reuse_empty": lambda: image_frame({}, 4096, rows=4), "reuse_cap": lambda: _cap(cols=4096, rows=4)}
REUSE_ORDER = ("reuse_full", "reuse_tiny11", "reuse_empty", "reuse_cap")
# frames with fewer than 12 ordered points: the compiled reference reads outside its vectors there (feature_extractor.cpp:50)
NOT_FOR_REFERENCE = {"tiny11": "11 ordered points: the reference's ExtractFeatures indexes N - 6 .. N - 1 and i - 5 .. i + 6 unguarded"}
# refpin's seeded random frames the device runs as well (tests/test_feature_cases.py checks what they cover)
FUZZ_SEEDS = (3, 4, 5, 6, 8, 9, 10, 11)


@functools.lru_cache(maxsize=None)
def frame(name: str) -> Frame:
    return (FRAMES.get(name) or REUSE[name])()


@functools.lru_cache(maxsize=None)
def modelled(name: str):
    f = frame(name)
    return model(f.raw, f.params)


@functools.lru_cache(maxsize=None)
def oracle_arrays(name: str, sort_mode: int = 0):
    """the oracle's arrays for a frame, ties in index order: what the device reproduces"""
    from oracle import oracle as O
    f = frame(name)
    o = O.OracleFeatures(**f.params)
    o.set_sort_mode(sort_mode)
    n = o.Project(f.raw)
    ran = o.ExtractFeatures()
    out = {k: _ro(o.get(k)) for k in O.FEAT_ARRAYS}
    out["n_ordered"], out["extracted"], out["tie_pairs"] = n, ran, o.tie_pairs()
    o.close()
    return out
