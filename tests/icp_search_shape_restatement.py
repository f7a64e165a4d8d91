"""numpy restatement of the shape of the score volume (include/tbnav_icp.h, CORRELATIVE SEARCH, items F1-F6) on top of
icp_search_restatement: an addition with no counterpart in the reference, so the header's items are its whole specification and
this file spells them out.

F2 / F3 are Python ints (exact, no order); F4 / F5 are Python floats (IEEE doubles, no contraction), every product and sum
parenthesised as the header writes it, sqrt is math's, that is glibc's.  The kernel reproduces the integers exactly and the
host the doubles: there is no tolerance.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import numpy as np

import icp_restatement as R
import icp_search_restatement as S


@dataclass(frozen=True)
class ShapeParams:
    """tbnav_icp_search_shape_params with tbnav_icp_default_search_shape_params' values"""
    drop_q10: int = 256
    flat_cells2: float = 2.0

    def with_(self, **kw):
        return replace(self, **kw)


def valid(sp: ShapeParams) -> bool:
    """F1's limits"""
    return 0 <= sp.drop_q10 <= 1023 and math.isfinite(sp.flat_cells2) and sp.flat_cells2 > 0.0


@dataclass
class Shape:
    """tbnav_icp_search_shape"""
    S0: int = 0
    Sx: int = 0
    Sy: int = 0
    Sxx: int = 0
    Sxy: int = 0
    Syy: int = 0
    l1: float = 0.0
    l2: float = 0.0
    ex: float = 0.0
    ey: float = 0.0
    T_raw: tuple = (0.0, 0.0, 0.0)
    cells: int = 0
    kind: int = 0
    computed: int = 0
    dx: float = 0.0     # d' of F5, in cells (not part of the C record)
    dy: float = 0.0


def sums(slice_, best: int, wl: int, drop_q10: int):
    """F2, F3 on the chosen angle's slice [nl][nl] -> (S0, Sx, Sy, Sxx, Sxy, Syy, cells)"""
    floor = best - ((best * drop_q10) >> 10)
    S0 = Sx = Sy = Sxx = Sxy = Syy = cells = 0
    rows = np.asarray(slice_).astype(np.int64).tolist()
    for iy, row in enumerate(rows):
        dy = iy - wl
        for ix, sc in enumerate(row):
            if sc <= floor:
                continue
            w, dx = sc - floor, ix - wl
            cells += 1
            S0 += w
            Sx += w * dx
            Sy += w * dy
            Sxx += w * dx * dx
            Sxy += w * dx * dy
            Syy += w * dy * dy
    return S0, Sx, Sy, Sxx, Sxy, Syy, cells


def moments(S0, Sx, Sy, Sxx, Sxy, Syy):
    """F4 -> (l1, l2, ex, ey); S0 > 0"""
    S0, Sx, Sy, Sxx, Sxy, Syy = (float(v) for v in (S0, Sx, Sy, Sxx, Sxy, Syy))
    mx, my = Sx / S0, Sy / S0
    a = (Sxx / S0) - (mx * mx)
    b = (Sxy / S0) - (mx * my)
    c = (Syy / S0) - (my * my)
    hd = 0.5 * (a - c)
    h = math.sqrt((hd * hd) + (b * b))
    l1 = (0.5 * (a + c)) + h
    l2 = (0.5 * (a + c)) - h
    vx, vy = (hd + h, b) if hd >= 0 else (b, h - hd)
    n = math.sqrt((vx * vx) + (vy * vy))
    ex, ey = (vx / n, vy / n) if n > 0 else (1.0, 0.0)
    return l1, l2, ex, ey


def shape(scores, info: S.Info, params: S.Params, shape_params: ShapeParams = ShapeParams()) -> Shape:
    """F2-F6 from the score volume [na][nl][nl] and S7's record.  Beside the record's fields the Shape carries d' of F5 (dx, dy,
    in cells: what search() below adds to the guess); for kind 0 it is S7's offset unchanged."""
    wl = params.lin_cells
    S0, Sx, Sy, Sxx, Sxy, Syy, cells = sums(np.asarray(scores)[info.ia], int(info.score), wl, shape_params.drop_q10)
    out = Shape(S0, Sx, Sy, Sxx, Sxy, Syy, T_raw=tuple(info.T), cells=cells, computed=1)
    d = (float(info.ix - wl), float(info.iy - wl))
    out.dx, out.dy = d
    if S0 == 0:
        return out
    out.l1, out.l2, out.ex, out.ey = moments(S0, Sx, Sy, Sxx, Sxy, Syy)
    flat = shape_params.flat_cells2
    if not out.l1 > flat:
        return out
    if out.l2 > flat:
        out.kind = 2
        out.dx, out.dy = 0.0, 0.0
    else:
        out.kind = 1
        p = (d[0] * out.ex) + (d[1] * out.ey)
        out.dx, out.dy = d[0] - (p * out.ex), d[1] - (p * out.ey)
    return out


def shaped(info: S.Info, sh: Shape, T_init, params: S.Params) -> S.Info:
    """F5's record: info with the shaped T (kind 0: info itself, bit for bit)"""
    if sh.kind == 0:
        return info
    x0, y0 = float(T_init[1]), float(T_init[2])
    return replace(info, T=(info.T[0], x0 + (sh.dx * params.resolution), y0 + (sh.dy * params.resolution)))


def search(target_scan, source_scan, laser: R.Laser, T_init, p: S.Params = S.Params(), sp: ShapeParams = ShapeParams(),
           Trs=(0.0, 0.0, 0.0), scores=None):
    """tbnav_icp_search_with_shape -> (the shaped Info, Shape)"""
    if scores is None:
        scores = S.scores(target_scan, source_scan, laser, T_init, p, Trs)
    info = S.search(target_scan, source_scan, laser, T_init, p, Trs, scores=scores)
    sh = shape(scores, info, p, sp)
    return shaped(info, sh, T_init, p), sh


def match(target_scan, source_scan, laser: R.Laser, T_init, p: S.Params = S.Params(), sp: ShapeParams = ShapeParams(),
          Trs=(0.0, 0.0, 0.0), icp=R.match, found=None, **kw):
    """S8 with the shape on: the search, the shape (or found = search(...)'s pair, when the caller has it already), then the ICP
    from the shaped T when accepted and from T_init unchanged otherwise -> (the ICP's Result, Info, Shape)"""
    info, sh = found if found is not None else search(target_scan, source_scan, laser, T_init, p, sp, Trs)
    start = info.T if info.accepted else tuple(float(v) for v in T_init)
    return icp(target_scan, source_scan, laser, start, Trs=Trs, **kw), info, sh
