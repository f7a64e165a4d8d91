"""numpy restatement of the alignment of a scan to a filter's map (include/tbnav_icp.h, MAP ALIGNMENT, items A1-A11), written from the
header alone.  Input: the occupancy as a bool array [ix][iy] with the map's xmin / ymin / resolution (icp_search_map_restatement.Geom)
and the source cloud with its beam indices (icp_restatement.cloud).  The nearest cell is found as A5 is written: every occupied cell
of the box, sorted by (D, mi, mj), not by rows outwards as the kernel does.  Everything is integer or IEEE fp64 with the header's
parentheses (Python floats, math.sqrt): the kernel reproduces it bit for bit.

`plant` names a deliberate error (tests/test_icp_align_map_cases.py shows that each changes at least one case): "no_half" (the centre
without + 0.5), "tie_high" (ties to the highest index), "early_stop" (a search by rows outwards that stops at dr^2 >= best),
"chebyshev" (the nearest by Chebyshev distance), "transposed" (the map transposed), "w_plus" / "w_minus" (w +- 1), "centre" (the
nearest cell's centre in place of the centroid)."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import numpy as np

from icp_line_restatement import MIN_COND
from icp_restatement import (ABS_MSE, DBL_MAX, DEGENERATE, F32, ITERATIONS, NO_CORRESPONDENCES, REL_MSE, TRANSFORM, _tree_sum)
from icp_search_map_restatement import Geom, cell_of

BEST_PARTICLE = -1
MAX_HALF = 256


@dataclass(frozen=True)
class Params:
    """tbnav_icp_align_map_params (A1a)"""
    half_cells: int = 128
    gate_cells: int = 10
    feature_cells: int = 2
    max_flatness: float = 0.25
    reserved: int = 0

    def with_(self, **kw):
        return replace(self, **kw)


def valid(p: Params) -> bool:
    return (8 <= p.half_cells <= MAX_HALF and 1 <= p.gate_cells <= 16 and 1 <= p.feature_cells <= 4 and math.isfinite(p.max_flatness)
            and 0.0 <= p.max_flatness < 1.0 and p.reserved == 0)


@dataclass
class Pairing:
    """tbnav_icp_align_map_pairs: per beam"""
    has_home: np.ndarray
    hi: np.ndarray
    hj: np.ndarray
    mi: np.ndarray
    mj: np.ndarray
    D: np.ndarray
    has_normal: np.ndarray
    kept: np.ndarray
    bx: np.ndarray
    by: np.ndarray
    nx: np.ndarray
    ny: np.ndarray


@dataclass
class Result:
    ok: bool
    T: tuple
    iterations: int
    correspondences: int
    mse: float
    criterion: int
    pairing: Pairing        # iteration 1's


class Window:
    """A3: the occupied cells that exist, and A4 / A5 on them (cached per cell: the window does not move)"""

    def __init__(self, occ, geom: Geom, T_init, p: Params, plant=None):
        occ = np.asarray(occ).astype(bool)
        assert occ.shape == (geom.side, geom.side)
        if plant == "transposed":
            occ = occ.T
        self.geom, self.p, self.plant = geom, p, plant
        self.cx, self.cy = cell_of(geom, float(T_init[1]), float(T_init[2]))
        H = p.half_cells
        self.x0, self.y0 = self.cx - H, self.cy - H
        self.ex = np.zeros((2 * H, 2 * H), dtype=bool)         # [mi - x0][mj - y0]
        lo_i, hi_i = max(self.x0, 0), min(self.x0 + 2 * H, geom.side)
        lo_j, hi_j = max(self.y0, 0), min(self.y0 + 2 * H, geom.side)
        if lo_i < hi_i and lo_j < hi_j:
            self.ex[lo_i - self.x0:hi_i - self.x0, lo_j - self.y0:hi_j - self.y0] = occ[lo_i:hi_i, lo_j:hi_j]
        self.w = p.feature_cells + (1 if plant == "w_plus" else -1 if plant == "w_minus" else 0)
        self._near, self._feat = {}, {}

    def inside(self, i, j):
        return self.x0 <= i < self.x0 + 2 * self.p.half_cells and self.y0 <= j < self.y0 + 2 * self.p.half_cells

    def nearest(self, hi, hj):
        """A5's target cell of home (hi, hj) -> (mi, mj, D) or None"""
        key = (hi, hj)
        if key not in self._near:
            self._near[key] = self._nearest(hi, hj)
        return self._near[key]

    def _nearest(self, hi, hj):
        G, n2 = self.p.gate_cells, 2 * self.p.half_cells
        r, c = hi - self.x0, hj - self.y0
        r0, r1, c0, c1 = max(r - G, 0), min(r + G + 1, n2), max(c - G, 0), min(c + G + 1, n2)
        cells = np.argwhere(self.ex[r0:r1, c0:c1])
        if cells.shape[0] == 0:
            return None
        mi, mj = cells[:, 0] + r0 + self.x0, cells[:, 1] + c0 + self.y0
        di, dj = mi - hi, mj - hj
        D = di * di + dj * dj
        if self.plant == "early_stop":
            best = None
            for dr in range(G + 1):
                if best is not None and dr * dr >= best[0]:
                    break
                for row in ([hi] if dr == 0 else [hi - dr, hi + dr]):
                    sel = mi == row
                    for q in np.nonzero(sel)[0]:
                        cand = (int(D[q]), int(mi[q]), int(mj[q]))
                        if best is None or cand < best:
                            best = cand
            return best[1], best[2], best[0]
        first = np.maximum(np.abs(di), np.abs(dj)) if self.plant == "chebyshev" else D
        if self.plant == "tie_high":
            order = np.lexsort((-mj, -mi, first))
        else:
            order = np.lexsort((mj, mi, first))
        q = int(order[0])
        return int(mi[q]), int(mj[q]), int(D[q])

    def feature(self, mi, mj):
        """A4 -> (bx, by, has, nx, ny): doubles, bool, float32s"""
        key = (mi, mj)
        if key not in self._feat:
            self._feat[key] = self._feature(mi, mj)
        return self._feat[key]

    def _feature(self, mi, mj):
        g, w, n2 = self.geom, self.w, 2 * self.p.half_cells
        n = sx = sy = sxx = sxy = syy = 0
        for di in range(-w, w + 1):
            for dj in range(-w, w + 1):
                r, c = mi + di - self.x0, mj + dj - self.y0
                if 0 <= r < n2 and 0 <= c < n2 and self.ex[r, c]:
                    n += 1; sx += di; sy += dj; sxx += di * di; sxy += di * dj; syy += dj * dj
        a, c, b = n * sxx - sx * sx, n * syy - sy * sy, n * sxy - sx * sy
        half = 0.0 if self.plant == "no_half" else 0.5
        if self.plant == "centre":
            bx = g.xmin + (float(mi) + half) * g.resolution
            by = g.ymin + (float(mj) + half) * g.resolution
        else:
            bx = g.xmin + ((float(mi) + half) + (float(sx) / float(n))) * g.resolution
            by = g.ymin + ((float(mj) + half) + (float(sy) / float(n))) * g.resolution
        hd = 0.5 * float(a - c)
        dd = math.sqrt((hd * hd) + (float(b) * float(b)))
        lmin = (0.5 * float(a + c)) - dd
        lmax = (0.5 * float(a + c)) + dd
        if not (n >= 3 and lmax > 0.0 and lmin <= self.p.max_flatness * lmax):
            return bx, by, False, F32(0.0), F32(0.0)
        if b != 0:
            vx, vy = float(b), lmin - float(a)
        elif a >= c:
            vx, vy = 0.0, 1.0
        else:
            vx, vy = 1.0, 0.0
        l = math.sqrt((vx * vx) + (vy * vy))
        return bx, by, True, F32(vx / l), F32(vy / l)


def align(occ, geom: Geom, src, src_beam, n_beams, T_init, p: Params = Params(), max_iter=100, transform_eps=1e-8, fitness_eps=1e-6, B=256,
          plant=None) -> Result:
    """tbnav_icp_align_map for one pair; None: the guess is TBNAV_ERR_OUT_OF_WORLD"""
    assert valid(p)
    T_init = tuple(float(v) for v in T_init)
    if not all(math.isfinite(v) for v in T_init) or cell_of(geom, T_init[1], T_init[2]) is None:
        return None
    win = Window(occ, geom, T_init, p, plant)
    src = np.asarray(src, dtype=np.float32).reshape(-1, 2)
    src_beam = np.asarray(src_beam, dtype=np.int64)
    m = src.shape[0]
    inv = 1.0 / geom.resolution
    G2 = p.gate_cells * p.gate_cells
    c0, s0 = float(F32(math.cos(T_init[0]))), float(F32(math.sin(T_init[0])))
    R = [[c0, -s0], [s0, c0]]
    t = [float(F32(T_init[1])), float(F32(T_init[2]))]
    prev = DBL_MAX
    sx, sy = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64)
    thread, rnd = src_beam % B, src_beam // B
    rounds = (n_beams + B - 1) // B
    pairing = None
    k = 0
    while True:
        k += 1
        with np.errstate(invalid="ignore", over="ignore"):
            ax = (((R[0][0] * sx) + (R[0][1] * sy)) + t[0]).astype(np.float32).astype(np.float64)
            ay = (((R[1][0] * sx) + (R[1][1] * sy)) + t[1]).astype(np.float32).astype(np.float64)
            fi = np.floor((ax - geom.xmin) * inv)
            fj = np.floor((ay - geom.ymin) * inv)
        keep = np.zeros(m, dtype=bool)
        bx, by, nx, ny = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m)
        if k == 1:
            z = lambda v=0: np.full(n_beams, v, dtype=np.int32)
            pairing = Pairing(z(), z(), z(), z(-1), z(-1), z(-1), z(), z(), np.zeros(n_beams), np.zeros(n_beams),
                              np.zeros(n_beams, dtype=np.float32), np.zeros(n_beams, dtype=np.float32))
        for q in range(m):
            if not (fi[q] >= win.x0 and fi[q] < win.x0 + 2 * p.half_cells and fj[q] >= win.y0 and fj[q] < win.y0 + 2 * p.half_cells):
                continue
            hi, hj = int(fi[q]), int(fj[q])
            tgt = win.nearest(hi, hj)
            i = int(src_beam[q])
            if k == 1:
                pairing.has_home[i], pairing.hi[i], pairing.hj[i] = 1, hi, hj
            if tgt is None:
                continue
            mi, mj, D = tgt
            fbx, fby, has, fnx, fny = win.feature(mi, mj)
            if k == 1:
                pairing.mi[i], pairing.mj[i], pairing.D[i], pairing.has_normal[i] = mi, mj, D, int(has)
                pairing.bx[i], pairing.by[i], pairing.nx[i], pairing.ny[i] = fbx, fby, fnx, fny
            if D <= G2 and has:
                keep[q] = True
                bx[q], by[q], nx[q], ny[q] = fbx, fby, float(fnx), float(fny)
                if k == 1:
                    pairing.kept[i] = 1
        n = int(keep.sum())
        if n < 3:
            return Result(False, T_init, k, n, 0.0, NO_CORRESPONDENCES, pairing)
        axk, ayk = np.where(keep, ax, 0.0), np.where(keep, ay, 0.0)
        ex, ey = axk - bx, ayk - by
        r = (nx * ex) + (ny * ey)
        jj = (axk * ny) - (ayk * nx)
        vals = [jj * jj, jj * nx, jj * ny, nx * nx, nx * ny, ny * ny, jj * r, nx * r, ny * r, r * r]
        tot = []
        for v in vals:
            partial = np.zeros(B)
            for q in range(rounds):   # each thread adds its q-th beam (if kept) in increasing beam order
                sel = keep & (rnd == q)
                partial[thread[sel]] = partial[thread[sel]] + v[sel]
            tot.append(_tree_sum(partial))
        H00, H01, H02, H11, H12, H22, g0, g1, g2, Sr = tot
        mse = Sr / float(n)
        tr = H11 + H22
        det = (H11 * H22) - (H12 * H12)
        if not det > MIN_COND * (tr * tr):
            return Result(False, T_init, k, n, mse, DEGENERATE, pairing)
        v1 = ((H22 * H01) - (H12 * H02)) / det
        v2 = ((H11 * H02) - (H12 * H01)) / det
        dth = H00 - ((H01 * v1) + (H02 * v2))
        if not dth > MIN_COND * H00:
            return Result(False, T_init, k, n, mse, DEGENERATE, pairing)
        th = -(g0 - ((v1 * g1) + (v2 * g2))) / dth
        w1 = g1 + (H01 * th)
        w2 = g2 + (H02 * th)
        tix = -((H22 * w1) - (H12 * w2)) / det
        tiy = -((H11 * w2) - (H12 * w1)) / det
        u = 0.5 * th
        qq = 1.0 + (u * u)
        c = (1.0 - (u * u)) / qq
        s = th / qq
        R = [[(c * R[0][0]) - (s * R[1][0]), (c * R[0][1]) - (s * R[1][1])],
             [(s * R[0][0]) + (c * R[1][0]), (s * R[0][1]) + (c * R[1][1])]]
        t = [((c * t[0]) - (s * t[1])) + tix, ((s * t[0]) + (c * t[1])) + tiy]
        crit = None
        if k >= max_iter:
            crit = ITERATIONS
        elif c >= 1.0 - transform_eps and ((tix * tix) + (tiy * tiy)) <= transform_eps:
            crit = TRANSFORM
        else:
            dm = abs(mse - prev)
            if dm < 1e-12:
                crit = ABS_MSE
            elif (dm / prev if prev != 0.0 else math.inf) < fitness_eps:      # (dm > 0 here: IEEE's dm / 0 is +inf)
                crit = REL_MSE
        if crit is not None:
            return Result(True, (math.atan2(R[1][0], R[0][0]), t[0], t[1]), k, n, mse, crit, pairing)
        prev = mse
