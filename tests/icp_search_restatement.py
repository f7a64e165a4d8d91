"""numpy restatement of the device ICP's correlative search (include/tbnav_icp.h, CORRELATIVE SEARCH, items S1-S8): an addition
with no counterpart in the reference, so the header's section is its whole specification and this file spells it out.

Integer arithmetic is Python's / numpy's int64; fp64 is Python floats or numpy float64 element by element (IEEE doubles, no
contraction), with every product and sum parenthesised as the header writes it; exp / cos / sin are math's, that is glibc's.
The clouds are icp_restatement.cloud (contract item 1).  The kernels reproduce all of it exactly: there is no tolerance.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import numpy as np

import icp_restatement as R

MAX_SIDE, MAX_STAMP, MAX_LIN, MAX_ANG = 208, 8, 16, 90


@dataclass(frozen=True)
class Params:
    """tbnav_icp_search_params with tbnav_icp_default_search_params' values"""
    resolution: float = 0.05
    half_extent: float = 4.0
    sigma: float = 0.05
    ang_step: float = math.pi / 180.0
    min_quality: float = 0.5
    stamp_cells: int = 3
    lin_cells: int = 6
    ang_steps: int = 20
    slack_q10: int = 0

    def with_(self, **kw):
        return replace(self, **kw)


def side(p: Params) -> int:
    return 2 * math.ceil(p.half_extent / p.resolution)


def valid(p: Params) -> bool:
    """S1's limits"""
    fin = all(math.isfinite(v) for v in (p.resolution, p.half_extent, p.sigma, p.ang_step, p.min_quality))
    if not fin or not (p.resolution > 0 and p.half_extent > 0 and p.sigma > 0):
        return False
    if not (1 <= p.stamp_cells <= MAX_STAMP and 0 <= p.lin_cells <= MAX_LIN and 0 <= p.ang_steps <= MAX_ANG and 0 <= p.slack_q10 <= 1023):
        return False
    cells = math.ceil(p.half_extent / p.resolution)
    return 1 <= cells <= MAX_SIDE and side(p) + 2 * p.lin_cells <= MAX_SIDE


def stamp(p: Params) -> np.ndarray:
    """S3: uint8 [2k+1][2k+1], indexed [oy + k][ox + k]"""
    k = p.stamp_cells
    st = np.zeros((2 * k + 1, 2 * k + 1), dtype=np.uint8)
    for oy in range(-k, k + 1):
        for ox in range(-k, k + 1):
            d2 = float(ox * ox + oy * oy) * (p.resolution * p.resolution)
            st[oy + k, ox + k] = math.floor(255.0 * math.exp(-(d2 / (2.0 * (p.sigma * p.sigma)))) + 0.5)
    return st


def _cells(v: np.ndarray, p: Params):
    """floor((v + E) * inv) per element: (int64 cells, mask of the elements that have one at all).  A cell that is not a number,
    or further than 65536 cells out, is outside every table and every window: it is dropped here, where it could not be an int."""
    inv = 1.0 / p.resolution
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((v + p.half_extent) * inv)
        ok = (f >= -65536.0) & (f <= 65536.0)
    return np.where(ok, f, 0.0).astype(np.int64), ok


def table_of_cloud(pts: np.ndarray, p: Params) -> np.ndarray:
    """S4: uint8 [n][n], indexed [iy][ix], from a float32 cloud [m][2]"""
    n, k = side(p), p.stamp_cells
    st = stamp(p)
    tab = np.zeros((n, n), dtype=np.uint8)
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    cx, okx = _cells(pts[:, 0].astype(np.float64), p)
    cy, oky = _cells(pts[:, 1].astype(np.float64), p)
    for ix, iy, ok in zip(cx.tolist(), cy.tolist(), (okx & oky).tolist()):
        if not ok:
            continue
        x0, x1, y0, y1 = max(ix - k, 0), min(ix + k + 1, n), max(iy - k, 0), min(iy + k + 1, n)
        if x0 >= x1 or y0 >= y1:
            continue
        part = st[y0 - (iy - k):y1 - (iy - k), x0 - (ix - k):x1 - (ix - k)]
        tab[y0:y1, x0:x1] = np.maximum(tab[y0:y1, x0:x1], part)
    return tab


def table(scan, laser: R.Laser, p: Params = Params(), Trs=(0.0, 0.0, 0.0)) -> np.ndarray:
    pts, _ = R.cloud(scan, laser, Trs)
    return table_of_cloud(pts, p)


def scores_of_clouds(tgt, src, T_init, p: Params) -> np.ndarray:
    """S5: the score volume, uint32 [na][nl][nl]"""
    n, wl, wa = side(p), p.lin_cells, p.ang_steps
    na, nl = 2 * wa + 1, 2 * wl + 1
    tab = table_of_cloud(tgt, p)
    # the table with 2*wl zero cells round it: every window of a base cell in [-wl, n - 1 + wl] is a slice of it, and what lies
    # outside the table adds 0
    big = np.zeros((n + 4 * wl, n + 4 * wl), dtype=np.int64)
    big[2 * wl:2 * wl + n, 2 * wl:2 * wl + n] = tab
    src = np.asarray(src, dtype=np.float32).reshape(-1, 2)
    sx, sy = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64)
    th0, x0, y0 = float(T_init[0]), float(T_init[1]), float(T_init[2])
    out = np.zeros((na, nl, nl), dtype=np.int64)
    d = np.arange(nl)
    for ia in range(na):
        th = th0 + float(ia - wa) * p.ang_step
        c, s = math.cos(th), math.sin(th)
        with np.errstate(invalid="ignore", over="ignore"):
            ax = (((c * sx) - (s * sy)) + x0)
            ay = (((s * sx) + (c * sy)) + y0)
        bx, okx = _cells(ax, p)
        by, oky = _cells(ay, p)
        keep = okx & oky & (bx >= -wl) & (bx <= n - 1 + wl) & (by >= -wl) & (by <= n - 1 + wl)   # all others read no table cell
        bx, by = bx[keep], by[keep]
        if bx.size:
            rows = (by + wl)[:, None, None] + d[None, :, None]     # by + (iy - wl), shifted by the border 2*wl
            cols = (bx + wl)[:, None, None] + d[None, None, :]
            out[ia] = big[rows, cols].sum(axis=0)
    assert out.max(initial=0) < 2 ** 32
    return out.astype(np.uint32)


@dataclass
class Info:
    """tbnav_icp_search_info"""
    T: tuple
    quality: float
    score: int
    points: int
    candidates: int
    ia: int
    iy: int
    ix: int
    at_edge: int
    accepted: int
    searched: int = 1


def select(scores: np.ndarray, p: Params):
    """S6 -> (ia, iy, ix, score of the chosen candidate, candidates)"""
    wl, wa = p.lin_cells, p.ang_steps
    na, nl = 2 * wa + 1, 2 * wl + 1
    sc = scores.astype(np.int64)
    best = int(sc.max())
    thr = best - ((best * p.slack_q10) >> 10)
    ia, iy, ix = np.meshgrid(np.arange(na), np.arange(nl), np.arange(nl), indexing="ij")
    D = (ia - wa) ** 2 + (iy - wl) ** 2 + (ix - wl) ** 2
    lin = (ia * nl + iy) * nl + ix
    mask = sc >= thr
    rank = np.where(mask, D * (1 << 20) + lin, np.iinfo(np.int64).max)   # D first, then the linear index (< 2^20)
    j = int(np.argmin(rank))
    a, y, x = np.unravel_index(j, sc.shape)
    return int(a), int(y), int(x), int(sc[a, y, x]), int(mask.sum())


def search_clouds(tgt, src, T_init, p: Params, scores=None) -> Info:
    """S6, S7 on explicit clouds"""
    wl, wa = p.lin_cells, p.ang_steps
    na, nl = 2 * wa + 1, 2 * wl + 1
    if scores is None:
        scores = scores_of_clouds(tgt, src, T_init, p)
    ia, iy, ix, score, cand = select(scores, p)
    th0, x0, y0 = float(T_init[0]), float(T_init[1]), float(T_init[2])
    T = (th0 + float(ia - wa) * p.ang_step, x0 + float(ix - wl) * p.resolution, y0 + float(iy - wl) * p.resolution)
    points = int(np.asarray(src).reshape(-1, 2).shape[0])
    quality = float(score) / (255.0 * float(points)) if points else 0.0
    at_edge = int((wa > 0 and ia in (0, na - 1)) or (wl > 0 and (iy in (0, nl - 1) or ix in (0, nl - 1))))
    accepted = int(quality >= p.min_quality and points > 0 and np.asarray(tgt).reshape(-1, 2).shape[0] > 0)
    return Info(T, quality, score, points, cand, ia, iy, ix, at_edge, accepted)


def scores(target_scan, source_scan, laser: R.Laser, T_init, p: Params = Params(), Trs=(0.0, 0.0, 0.0)) -> np.ndarray:
    tgt, _ = R.cloud(target_scan, laser, Trs)
    src, _ = R.cloud(source_scan, laser, Trs)
    return scores_of_clouds(tgt, src, T_init, p)


def search(target_scan, source_scan, laser: R.Laser, T_init, p: Params = Params(), Trs=(0.0, 0.0, 0.0), scores=None) -> Info:
    """tbnav_icp_search"""
    tgt, _ = R.cloud(target_scan, laser, Trs)
    src, _ = R.cloud(source_scan, laser, Trs)
    return search_clouds(tgt, src, T_init, p, scores)


def match(target_scan, source_scan, laser: R.Laser, T_init, p: Params = Params(), Trs=(0.0, 0.0, 0.0), icp=R.match, info=None, **kw):
    """S8: the search (or its record info, when the caller has it already), then the ICP (icp = icp_restatement.match or
    icp_line_restatement.match) from T when accepted and from T_init unchanged otherwise -> (the ICP's Result, Info)"""
    if info is None:
        info = search(target_scan, source_scan, laser, T_init, p, Trs)
    start = info.T if info.accepted else tuple(float(v) for v in T_init)
    return icp(target_scan, source_scan, laser, start, Trs=Trs, **kw), info
