"""Restatement of the check of a pose against a filter's map (include/tbnav_icp.h, MAP CHECK, items V1-V10), written from the header
alone, in Python integers.  Input: the map's classes (Classes: from the log-odds [ix][iy] and the occupancy, or from the filter's own
exported map and the occupancy), the map's xmin / ymin / resolution (icp_search_map_restatement.Geom), the source cloud with its beam
indices (icp_restatement.cloud) and the cloud-frame point of a zero range (origin_of).  The point transform is the one
icp_align_map_restatement uses for A5 (item 3 from the float-rounded pose of item 2); D is found as V5 is written, over every
occupied cell of the box, not by rows outwards as the kernel does; the ray's offsets are G17's closed form per step
(nav_gain_restatement.ray_steps), not a carried remainder.  The kernel reproduces every field with ==.

`plant` names a deliberate error (tests/test_icp_verify_map_cases.py shows that each changes at least one case): "bresenham" (a
carried-error Bresenham in place of the closed form), "no_corner" (no corner rule), "through_le" (b + k <= n), "chebyshev" (a
Chebyshev D), "transposed" (the map transposed), "count_end" (the end cell counted in the path counts), "free_strict"
(l < free_cut), "no_trs" (a sensor cell that ignores Trs)."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import numpy as np

from icp_restatement import F32
from icp_search_map_restatement import Geom, cell_of
from nav_frontier_restatement import export_value
from nav_gain_restatement import ray_steps

BEST_PARTICLE = -1
MAX_HALF, MAX_SLACK = 128, 8
NONE, OUTSIDE, HIT, THROUGH, MISSING, UNSEEN, UNDECIDED = range(7)       # tbnav_icp_verify_class
C_UNKNOWN, C_FREE, C_OCCUPIED, C_OTHER = range(4)                         # V7's sensor_class
BEAM_FIELDS = ("cls", "ei", "ej", "n", "b", "D", "free_cells", "unknown_cells")
INFO_FIELDS = ("points", "outside", "walked", "hit", "through", "missing", "unseen", "undecided", "free_cells", "unknown_cells",
               "sensor_cell", "sensor_class", "accepted")
PLANTS = ("bresenham", "no_corner", "through_le", "chebyshev", "transposed", "count_end", "free_strict", "no_trs")


@dataclass(frozen=True)
class Params:
    """tbnav_icp_verify_map_params (V1a)"""
    half_cells: int = 96
    slack_cells: int = 2
    max_through_q10: int = 102
    max_missing_q10: int = 102
    min_hit_q10: int = 512
    reserved: int = 0

    def with_(self, **kw):
        return replace(self, **kw)


def valid(p: Params) -> bool:
    q10 = lambda v: 0 <= v <= 1024
    return (8 <= p.half_cells <= MAX_HALF and 0 <= p.slack_cells <= MAX_SLACK and q10(p.max_through_q10) and q10(p.max_missing_q10)
            and q10(p.min_hit_q10) and p.reserved == 0)


def free_cut() -> float:
    """the largest log-odds GridMapper::gridMap exports as 0 (probability <= 0.35): G10's free_cut, by bisection"""
    prob = lambda l: 1 - (1 / (1 + math.exp(l)))
    lo, hi = -3.0, 0.0
    while math.nextafter(lo, hi) < hi:
        mid = 0.5 * (lo + hi)
        if prob(mid) > 0.35:
            hi = mid
        else:
            lo = mid
    assert export_value(lo) == 0 and export_value(hi) != 0
    return lo


class Classes:
    """V2: the class of every cell, int8 [ix][iy]"""

    def __init__(self, cls):
        self.cls = np.ascontiguousarray(cls, dtype=np.int8)

    @staticmethod
    def from_log_odds(lo, occ, plant=None):
        """from the log-odds [ix][iy] and the occupancy bits [ix][iy] (OCCUPIED wins)"""
        lo = np.asarray(lo, dtype=np.float64)
        cut = free_cut()
        def one(l):
            v = export_value(l)
            if v == -1:
                return C_UNKNOWN
            if plant == "free_strict":
                return C_FREE if l < cut else C_OTHER
            return C_FREE if v == 0 else C_OTHER
        vals = {float(v): one(float(v)) for v in np.unique(lo)}
        cls = np.vectorize(lambda v: vals[float(v)], otypes=[np.int8])(lo)
        cls[np.asarray(occ).astype(bool)] = C_OCCUPIED
        return Classes(cls)

    @staticmethod
    def from_export(exported, occ, side):
        """from the filter's own exported map (int8 [G], the grid TRANSPOSED: -1 UNKNOWN, 0 FREE) and the occupancy bits [ix][iy]"""
        m = np.asarray(exported, dtype=np.int8).reshape(side, side).T
        cls = np.where(m == -1, C_UNKNOWN, np.where(m == 0, C_FREE, C_OTHER)).astype(np.int8)
        cls[np.asarray(occ).astype(bool)] = C_OCCUPIED
        return Classes(cls)


def origin_of(Trs=(0.0, 0.0, 0.0)):
    """the cloud-frame point a zero range would give: Trs's translation as item 1 forms it"""
    return F32(float(Trs[1])), F32(float(Trs[2]))


@dataclass
class Result:
    info: dict              # V7, INFO_FIELDS
    beams: dict             # V9, BEAM_FIELDS -> int32 [n_beams]


def _bresenham(di, dj):
    """the planted walk: the error term carried from step to step"""
    ai, aj, si, sj = abs(di), abs(dj), (di > 0) - (di < 0), (dj > 0) - (dj < 0)
    n = max(ai, aj)
    out, i, j = [], 0, 0
    if ai >= aj:
        err = 2 * aj - ai
        for _ in range(n):
            if err > 0:
                j += sj; err -= 2 * ai
            err += 2 * aj
            i += si
            out.append((i, j))
    else:
        err = 2 * ai - aj
        for _ in range(n):
            if err > 0:
                i += si; err -= 2 * aj
            err += 2 * ai
            j += sj
            out.append((i, j))
    return out


def pose_floats(T):
    """item 2: the float-rounded pose held in fp64 -> (c, s, x, y)"""
    with np.errstate(over="ignore"):
        return float(F32(math.cos(T[0]))), float(F32(math.sin(T[0]))), float(F32(T[1])), float(F32(T[2]))


def transform(c, s, x, y, px, py):
    """item 3 / A5: the doubles of the float point a"""
    with np.errstate(invalid="ignore", over="ignore"):
        ax = np.float32(((c * float(px)) + ((-s) * float(py))) + x)
        ay = np.float32(((s * float(px)) + (c * float(py))) + y)
    return float(ax), float(ay)


def sensor_cell(geom: Geom, T, origin=(0.0, 0.0), plant=None):
    """V3's s, or None: TBNAV_ERR_OUT_OF_WORLD"""
    T = tuple(float(v) for v in T)
    if not all(math.isfinite(v) for v in T):
        return None
    c, s, x, y = pose_floats(T)
    o = (0.0, 0.0) if plant == "no_trs" else origin
    ax, ay = transform(c, s, x, y, o[0], o[1])
    return cell_of(geom, ax, ay)


def verify(classes: Classes, geom: Geom, src, src_beam, n_beams, T, p: Params = Params(), origin=(0.0, 0.0), plant=None) -> Result:
    """tbnav_icp_verify_map_beams for one pair; None: the pose is TBNAV_ERR_OUT_OF_WORLD"""
    assert valid(p)
    cls = classes.cls.T if plant == "transposed" else classes.cls
    assert cls.shape == (geom.side, geom.side)
    sc = sensor_cell(geom, T, origin, plant)
    if sc is None:
        return None
    si, sj = sc
    H, k, side = p.half_cells, p.slack_cells, geom.side
    inv = 1.0 / geom.resolution
    c, s, x, y = pose_floats(tuple(float(v) for v in T))
    inside = lambda i, j: si - H <= i < si + H and sj - H <= j < sj + H and 0 <= i < side and 0 <= j < side
    occupied = lambda i, j: cls[i, j] == C_OCCUPIED
    beams = {f: np.zeros(n_beams, dtype=np.int32) for f in BEAM_FIELDS}
    count = {HIT: 0, THROUGH: 0, MISSING: 0, UNSEEN: 0, UNDECIDED: 0}
    points = outside = free_cells = unknown_cells = 0
    src = np.asarray(src, dtype=np.float32).reshape(-1, 2)
    for q in range(src.shape[0]):
        i = int(src_beam[q])
        points += 1
        ax, ay = transform(c, s, x, y, src[q, 0], src[q, 1])
        with np.errstate(invalid="ignore", over="ignore"):
            fi, fj = np.floor((np.float64(ax) - geom.xmin) * inv), np.floor((np.float64(ay) - geom.ymin) * inv)
        if not (fi >= max(si - H, 0) and fi < min(si + H, side) and fj >= max(sj - H, 0) and fj < min(sj + H, side)):
            outside += 1
            beams["cls"][i] = OUTSIDE
            continue
        ei, ej = int(fi), int(fj)
        di, dj = ei - si, ej - sj
        n = max(abs(di), abs(dj))
        steps = _bresenham(di, dj) if plant == "bresenham" else (ray_steps(di, dj) if n else [])
        b, pi, pj = n + 1, si, sj
        for t, (oi, oj) in enumerate(steps, start=1):
            ci, cj = si + oi, sj + oj
            blocked = occupied(ci, cj)
            if plant != "no_corner" and ci != pi and cj != pj and occupied(pi, cj) and occupied(ci, pj):
                blocked = True
            if blocked:
                b = t
                break
            pi, pj = ci, cj
        last = min(b, n) - 1 + (1 if plant == "count_end" and b > n else 0)
        nf = sum(1 for oi, oj in steps[:last] if cls[si + oi, sj + oj] == C_FREE)
        nu = sum(1 for oi, oj in steps[:last] if cls[si + oi, sj + oj] == C_UNKNOWN)
        through = (b + k <= n) if plant == "through_le" else (b + k < n)
        D = -1
        if through:
            kind = THROUGH
        else:
            best = None
            for mi in range(ei - k, ei + k + 1):
                for mj in range(ej - k, ej + k + 1):
                    if inside(mi, mj) and occupied(mi, mj):
                        d = (mi - ei) ** 2 + (mj - ej) ** 2
                        if plant == "chebyshev":
                            d = max(abs(mi - ei), abs(mj - ej)) ** 2
                        if best is None or d < best:
                            best = d
            if best is not None:
                D = best
            if best is not None and D <= k * k:
                kind = HIT
            else:
                kind = {C_FREE: MISSING, C_UNKNOWN: UNSEEN, C_OTHER: UNDECIDED, C_OCCUPIED: HIT}[int(cls[ei, ej])]
        count[kind] += 1
        free_cells += nf
        unknown_cells += nu
        for f, v in zip(BEAM_FIELDS, (kind, ei, ej, n, b if b <= n else -1, D, nf, nu)):
            beams[f][i] = v
    walked = points - outside
    accepted = int(walked >= 1 and count[THROUGH] * 1024 <= p.max_through_q10 * walked and count[MISSING] * 1024 <= p.max_missing_q10 * walked
                   and count[HIT] * 1024 >= p.min_hit_q10 * walked)
    info = dict(points=points, outside=outside, walked=walked, hit=count[HIT], through=count[THROUGH], missing=count[MISSING],
                unseen=count[UNSEEN], undecided=count[UNDECIDED], free_cells=free_cells, unknown_cells=unknown_cells, sensor_cell=(si, sj),
                sensor_class=int(cls[si, sj]), accepted=accepted)
    assert count[HIT] + count[THROUGH] + count[MISSING] + count[UNSEEN] + count[UNDECIDED] == walked
    return Result(info, beams)
