"""numpy restatement of the correlative search against a filter's map (include/tbnav_icp.h, MAP SEARCH, items M1-M9), written from
the header alone.  Input: the occupancy as a bool array [ix][iy] with the map's xmin / ymin / resolution, and the source cloud
(float32 [m][2], icp_restatement.cloud).  The table is M4 as it is written — every occupied cell stamps S3's stamp by a maximum — and
not the nearest-cell form the kernel uses; S5 is spelt out here with E' in E's place; S6, S7, F1-F6 and W1-W8 are
icp_search_restatement's, icp_search_shape_restatement's and icp_search_wide_restatement's own code on this file's score volumes.
Everything is integer or IEEE fp64 element by element with the header's parentheses: the kernels reproduce it exactly.

`plant` names a deliberate error (tests/test_icp_search_map_cases.py shows that each changes at least one case): "disc" (the stamp cut
to a disc of radius k), "transposed", "origin" (cx - h2 off by one), "E" (S1's E kept), "outside" (cells outside the map occupied),
"chebyshev" (the value taken at the nearest cell by Chebyshev distance)."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

import icp_search_restatement as S
import icp_search_shape_restatement as F
import icp_search_wide_restatement as W

BEST_PARTICLE = -1


@dataclass(frozen=True)
class Geom:
    """the filter's grid (tbnav_rbpf_params): a square map of side cells"""
    xmin: float
    ymin: float
    resolution: float
    side: int


@dataclass(frozen=True)
class Frame:
    """M3"""
    cx: int
    cy: int
    h2: int
    ox: float       # the table's origin o
    oy: float
    E: float        # E'
    local: tuple    # the local guess (theta0, x0 - o.x, y0 - o.y)


def cell_of(geom: Geom, x: float, y: float):
    """M2 / G1 -> (ci, cj), or None outside the map or for a position that is not finite"""
    if not (math.isfinite(x) and math.isfinite(y)):
        return None
    inv = 1.0 / geom.resolution
    fi, fj = math.floor((x - geom.xmin) * inv), math.floor((y - geom.ymin) * inv)
    if not (0 <= fi < geom.side and 0 <= fj < geom.side):
        return None
    return int(fi), int(fj)


def frame(geom: Geom, T_init, p: S.Params, plant=None) -> Frame:
    """M3; None: TBNAV_ERR_OUT_OF_WORLD"""
    th0, x0, y0 = float(T_init[0]), float(T_init[1]), float(T_init[2])
    c = cell_of(geom, x0, y0)
    if c is None or not math.isfinite(th0):
        return None
    cx, cy = c
    h2 = S.side(p) // 2
    ox, oy = geom.xmin + float(cx) * geom.resolution, geom.ymin + float(cy) * geom.resolution
    E = p.half_extent if plant == "E" else float(h2) * geom.resolution
    return Frame(cx, cy, h2, ox, oy, E, (th0, (x0 - ox), (y0 - oy)))


def stamp_by_d2(p: S.Params) -> np.ndarray:
    """S3's stamp as a function of d2 = ox^2 + oy^2, 0 .. 2k^2 (entries no offset pair reaches hold what the formula gives)"""
    k = p.stamp_cells
    out = np.zeros(2 * k * k + 1, dtype=np.uint8)
    for c in range(out.size):
        d2 = float(c) * (p.resolution * p.resolution)
        out[c] = math.floor(255.0 * math.exp(-(d2 / (2.0 * (p.sigma * p.sigma)))) + 0.5)
    return out


def stamp_is_a_non_increasing_function_of_d2(p: S.Params) -> bool:
    """what the kernel's nearest-cell form stands on: S3's stamp equals stamp_by_d2 at every offset, and that never rises"""
    k, st, v = p.stamp_cells, S.stamp(p), stamp_by_d2(p)
    same = all(st[oy + k, ox + k] == v[ox * ox + oy * oy] for oy in range(-k, k + 1) for ox in range(-k, k + 1))
    return same and bool(np.all(np.diff(v.astype(np.int64)) <= 0))


def table(occ, geom: Geom, T_init, p: S.Params, plant=None):
    """M4 -> (uint8 [n][n] indexed [iy][ix], tgt_points)"""
    occ = np.asarray(occ).astype(bool)
    assert occ.shape == (geom.side, geom.side) and p.resolution == geom.resolution
    fr = frame(geom, T_init, p, plant)
    n, k = S.side(p), p.stamp_cells
    st = S.stamp(p).copy()
    if plant == "disc":
        for oy in range(-k, k + 1):
            for ox in range(-k, k + 1):
                if ox * ox + oy * oy > k * k:
                    st[oy + k, ox + k] = 0
    bx, by = fr.cx - fr.h2 + (1 if plant == "origin" else 0), fr.cy - fr.h2       # the map cell of table cell [0][0]
    # the map's cells round the window, k further on every side: win[iy + k][ix + k] = occupied(bx + ix, by + iy)
    win = np.full((n + 2 * k, n + 2 * k), plant == "outside", dtype=bool)
    for jy in range(n + 2 * k):
        my = by + jy - k
        if not 0 <= my < geom.side:
            continue
        for jx in range(n + 2 * k):
            mx = bx + jx - k
            if 0 <= mx < geom.side:
                win[jy, jx] = occ[mx, my]
    tab = np.zeros((n, n), dtype=np.uint8)
    if plant == "chebyshev":
        v = stamp_by_d2(p)
        ys, xs = np.nonzero(win)
        for iy in range(n):
            for ix in range(n):
                dy, dx = ys - (iy + k), xs - (ix + k)
                near = (np.abs(dy) <= k) & (np.abs(dx) <= k)
                if near.any():
                    ch = np.maximum(np.abs(dy[near]), np.abs(dx[near]))
                    j = int(np.argmin(ch))                       # the first of the nearest by Chebyshev distance, in row order
                    tab[iy, ix] = v[int(dy[near][j]) ** 2 + int(dx[near][j]) ** 2]
    else:
        for jy, jx in zip(*np.nonzero(win)):
            iy, ix = int(jy) - k, int(jx) - k                    # table coordinates of the occupied cell, -k .. n - 1 + k
            x0, x1, y0, y1 = max(ix - k, 0), min(ix + k + 1, n), max(iy - k, 0), min(iy + k + 1, n)
            if x0 < x1 and y0 < y1:
                part = st[y0 - (iy - k):y1 - (iy - k), x0 - (ix - k):x1 - (ix - k)]
                tab[y0:y1, x0:x1] = np.maximum(tab[y0:y1, x0:x1], part)
    tgt_points = int(win[k:k + n, k:k + n].sum())
    if plant == "transposed":
        tab = np.ascontiguousarray(tab.T)
    return tab, tgt_points


def _cells(v: np.ndarray, E: float, inv: float):
    """S5's floor((v + E) * inv) per element, as icp_search_restatement._cells with E given"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((v + E) * inv)
        ok = (f >= -65536.0) & (f <= 65536.0)
    return np.where(ok, f, 0.0).astype(np.int64), ok


def scores_on_table(tab: np.ndarray, src, fr: Frame, p: S.Params) -> np.ndarray:
    """S5 on a given table with the local guess and E := E' (M5): uint32 [na][nl][nl]"""
    n, wl, wa = S.side(p), p.lin_cells, p.ang_steps
    na, nl = 2 * wa + 1, 2 * wl + 1
    inv = 1.0 / p.resolution
    big = np.zeros((n + 4 * wl, n + 4 * wl), dtype=np.int64)
    big[2 * wl:2 * wl + n, 2 * wl:2 * wl + n] = tab
    src = np.asarray(src, dtype=np.float32).reshape(-1, 2)
    sx, sy = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64)
    th0, x0, y0 = fr.local
    out = np.zeros((na, nl, nl), dtype=np.int64)
    d = np.arange(nl)
    for ia in range(na):
        th = th0 + float(ia - wa) * p.ang_step
        c, s = math.cos(th), math.sin(th)
        with np.errstate(invalid="ignore", over="ignore"):
            ax = (((c * sx) - (s * sy)) + x0)
            ay = (((s * sx) + (c * sy)) + y0)
        bx, okx = _cells(ax, fr.E, inv)
        by, oky = _cells(ay, fr.E, inv)
        keep = okx & oky & (bx >= -wl) & (bx <= n - 1 + wl) & (by >= -wl) & (by <= n - 1 + wl)
        bx, by = bx[keep], by[keep]
        if bx.size:
            rows = (by + wl)[:, None, None] + d[None, :, None]
            cols = (bx + wl)[:, None, None] + d[None, None, :]
            out[ia] = big[rows, cols].sum(axis=0)
    assert out.max(initial=0) < 2 ** 32
    return out.astype(np.uint32)


def slow_list_points(src, fr: Frame, p: S.Params) -> int:
    """how many (point, angle) base cells lie outside the table while their window reaches into it (the kernels' bounds-tested list)"""
    n, wl, wa = S.side(p), p.lin_cells, p.ang_steps
    src = np.asarray(src, dtype=np.float32).reshape(-1, 2)
    sx, sy = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64)
    th0, x0, y0 = fr.local
    cnt = 0
    for ia in range(2 * wa + 1):
        th = th0 + float(ia - wa) * p.ang_step
        c, s = math.cos(th), math.sin(th)
        bx, okx = _cells((((c * sx) - (s * sy)) + x0), fr.E, 1.0 / p.resolution)
        by, oky = _cells((((s * sx) + (c * sy)) + y0), fr.E, 1.0 / p.resolution)
        inside = (bx >= 0) & (bx < n) & (by >= 0) & (by < n)
        reach = (bx >= -wl) & (bx < n + wl) & (by >= -wl) & (by < n + wl)
        cnt += int((okx & oky & reach & ~inside).sum())
    return cnt


@dataclass
class Result:
    """one map search: what tbnav_icp_search_map returns and leaves in the handle, and the hooks' arrays"""
    table: np.ndarray
    tgt_points: int
    scores: object          # the first stage's volume (None with when = ALWAYS)
    wide_scores: object     # the wide stage's (None where it did not run)
    outcome: W.Outcome      # info (world T), first, ran, shape


def search(occ, geom: Geom, src, T_init, p: S.Params = S.Params(), wp: W.WideParams = None, shape_params: F.ShapeParams = None,
           plant=None) -> Result:
    """tbnav_icp_search_map for one pair (M1-M6); None: the guess is TBNAV_ERR_OUT_OF_WORLD"""
    fr = frame(geom, T_init, p, plant)
    if fr is None:
        return None
    tab, tgt_points = table(occ, geom, T_init, p, plant)
    tgt = np.zeros((tgt_points, 2), dtype=np.float32)          # S7 asks only whether there is a target point: M5's tgt_points > 0
    T_world = tuple(float(v) for v in T_init)
    if wp is None:
        sc = scores_on_table(tab, src, fr, p)
        info, shape = W._stage(tgt, src, T_world, p, shape_params, sc)
        return Result(tab, tgt_points, sc, None, W.Outcome(info, None, 0, shape))      # (no wide record: first = None)
    sc = None if wp.when == W.ALWAYS else scores_on_table(tab, src, fr, p)
    first = None if sc is None else S.search_clouds(tgt, src, T_world, p, scores=sc)
    wide = scores_on_table(tab, src, fr, W.window(p, wp)) if sc is None or W.runs(first, wp.when) else None
    out = W.search_clouds(tgt, src, T_world, p, wp, shape_params, first_scores=sc, wide_scores=wide)
    return Result(tab, tgt_points, sc, wide if out.ran else None, out)
