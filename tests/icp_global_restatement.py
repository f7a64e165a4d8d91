"""numpy restatement of the global search (include/tbnav_icp.h, GLOBAL SEARCH, items L1-L10), written from the header alone.  Input: the
occupancy as a bool array [ci][cj] with the map's xmin / ymin / resolution, and the source cloud (float32 [m][2],
icp_restatement.cloud).  It is EXHAUSTIVE: every candidate of the region is scored, nothing is pruned; the bound volume is there to
be compared and to show that a bound never falls below a score.  lik is L2 as it is written (every occupied cell stamps S3's stamp by
a maximum), not the nearest-cell form the kernel uses.  Everything is integer, or IEEE fp64 element by element with the header's
parentheses: the kernels reproduce it exactly.

`plant` names a deliberate error (tests/test_icp_global_cases.py shows that each changes at least one case): "centred" (the pool's
window centred on the cell instead of forward of it), "nohalf" (floor(x * inv) without the half), "transposed" (the map), "tie_high"
(ties going to the highest index), "outside" (cells outside the map counted as occupied), "per_cell" (the offsets taken per cell,
from the world position of the cell's centre, instead of once per heading)."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import numpy as np

import icp_search_restatement as S

BEST_PARTICLE = -1
MAX_SIDE, MAX_ANG, MAX_BLOCKS, MAX_HOOK_SCORES = 2048, 720, 1 << 26, 1 << 24


@dataclass(frozen=True)
class Geom:
    """the filter's grid (tbnav_rbpf_params): a square map of side cells"""
    xmin: float
    ymin: float
    resolution: float
    side: int


@dataclass(frozen=True)
class Params:
    """tbnav_icp_global_params (L1)"""
    ang_count: int = 360
    ang_step: float = math.pi / 180.0
    pool_log2: int = 3
    region: tuple = (-1, -1, -1, -1)
    min_quality: float = 0.5
    reserved: int = 0

    def with_(self, **kw):
        return replace(self, **kw)


def valid(gp: Params, side: int) -> bool:
    """L1's INVALID_ARG rules for the parameters"""
    if not (1 <= gp.ang_count <= MAX_ANG and math.isfinite(gp.ang_step) and math.isfinite(gp.min_quality)):
        return False
    if not (1 <= gp.pool_log2 <= 5 and gp.reserved == 0):
        return False
    r = gp.region
    if tuple(r) == (-1, -1, -1, -1):
        return True
    return 0 <= r[0] <= r[2] < side and 0 <= r[1] <= r[3] < side


def region(gp: Params, side: int):
    """-> (tx0, ty0, w, h)"""
    if tuple(gp.region) == (-1, -1, -1, -1):
        return 0, 0, side, side
    tx0, ty0, tx1, ty1 = gp.region
    return tx0, ty0, tx1 - tx0 + 1, ty1 - ty0 + 1


def block_grid(gp: Params, side: int):
    """L5 -> (s, nbx, nby, blocks)"""
    s = 1 << gp.pool_log2
    _, _, w, h = region(gp, side)
    nbx, nby = -(-w // s), -(-h // s)
    return s, nbx, nby, gp.ang_count * nbx * nby


def lik_map(occ, sp: S.Params, plant=None) -> np.ndarray:
    """L2 -> uint8 [side][side] indexed [ci][cj]"""
    occ = np.asarray(occ).astype(bool)
    side, k = occ.shape[0], sp.stamp_cells
    assert occ.shape == (side, side)
    st = S.stamp(sp)                                   # [oy + k][ox + k]
    big = np.full((side + 2 * k, side + 2 * k), plant == "outside", dtype=bool)
    big[k:k + side, k:k + side] = occ
    out = np.zeros((side, side), dtype=np.uint8)
    for dy in range(-k, k + 1):
        for dx in range(-k, k + 1):
            # the occupied cell (mi, mj) = (ci + dx, cj + dy) stamps stamp[mj - cj + k][mi - ci + k] onto (ci, cj)
            there = big[k + dx:k + dx + side, k + dy:k + dy + side]
            out = np.maximum(out, np.where(there, st[dy + k, dx + k], 0).astype(np.uint8))
    if plant == "transposed":
        out = np.ascontiguousarray(out.T)
    return out


def pool_map(lik: np.ndarray, s: int, plant=None) -> np.ndarray:
    """L5's pool for i, j in -(s - 1) .. side - 1 -> uint8 [side + s - 1][side + s - 1] indexed [i + s - 1][j + s - 1]"""
    side, e = lik.shape[0], s - 1
    lo = s // 2 if plant == "centred" else 0                              # the window is i - lo .. i - lo + s - 1
    big = np.zeros((side + 3 * s, side + 3 * s), dtype=np.uint8)          # lik(i, j) at [i + 2s][j + 2s]
    big[2 * s:2 * s + side, 2 * s:2 * s + side] = lik
    out = np.zeros((side + e, side + e), dtype=np.uint8)
    for a in range(s):
        for b in range(s):
            r0, c0 = 2 * s - e + a - lo, 2 * s - e + b - lo
            out = np.maximum(out, big[r0:r0 + side + e, c0:c0 + side + e])
    return out


def offsets(src, ia: int, gp: Params, resolution: float, plant=None):
    """L3 -> (ox, oy, ok): int64 per valid source point, ok False where the guard drops the point at this heading"""
    src = np.asarray(src, dtype=np.float32).reshape(-1, 2)
    sx, sy = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64)
    th = float(ia) * gp.ang_step
    c, s = math.cos(th), math.sin(th)
    inv = 1.0 / resolution
    half = 0.0 if plant == "nohalf" else 0.5
    with np.errstate(invalid="ignore", over="ignore"):
        vx = ((((c * sx) - (s * sy))) * inv) + half
        vy = ((((s * sx) + (c * sy))) * inv) + half
        ok = (vx >= -65536.0) & (vx <= 65536.0) & (vy >= -65536.0) & (vy <= 65536.0)
    ox = np.floor(np.where(ok, vx, 0.0)).astype(np.int64)
    oy = np.floor(np.where(ok, vy, 0.0)).astype(np.int64)
    return ox, oy, ok


def _gather_sum(big: np.ndarray, m: int, ox, oy, x0: int, y0: int, nx: int, ny: int, step: int) -> np.ndarray:
    """sum over the points of field(x0 + a * step + ox, y0 + b * step + oy) for a < nx, b < ny; big holds the field with a zero
    margin of m cells, field(i, j) at [i + m][j + m]; a point that reads outside big for every (a, b) adds nothing"""
    out = np.zeros((nx, ny), dtype=np.int64)
    pairs, counts = np.unique(np.stack([ox, oy], axis=1), axis=0, return_counts=True) if len(ox) else (np.zeros((0, 2), np.int64), [])
    n = big.shape[0]
    for (dx, dy), cnt in zip(pairs, counts):
        xs = x0 + int(dx) + m + step * np.arange(nx)
        ys = y0 + int(dy) + m + step * np.arange(ny)
        okx, oky = (xs >= 0) & (xs < n), (ys >= 0) & (ys < n)
        if okx.any() and oky.any():
            out[np.ix_(okx, oky)] += int(cnt) * big[np.ix_(xs[okx], ys[oky])].astype(np.int64)
    return out


def _scores_per_cell(lik, src, ia, gp, geom: Geom):
    """the plant "per_cell": every point's cell from the world position of the cell's centre"""
    tx0, ty0, w, h = region(gp, geom.side)
    src = np.asarray(src, dtype=np.float32).reshape(-1, 2)
    sx, sy = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64)
    th = float(ia) * gp.ang_step
    c, s = math.cos(th), math.sin(th)
    inv = 1.0 / geom.resolution
    rx, ry = ((c * sx) - (s * sy)), ((s * sx) + (c * sy))
    out = np.zeros((w, h), dtype=np.int64)
    for a in range(w):
        wx = (geom.xmin + ((float(tx0 + a) + 0.5) * geom.resolution)) + rx
        ci = np.floor((wx - geom.xmin) * inv)
        for b in range(h):
            wy = (geom.ymin + ((float(ty0 + b) + 0.5) * geom.resolution)) + ry
            cj = np.floor((wy - geom.ymin) * inv)
            ok = (ci >= 0) & (ci < geom.side) & (cj >= 0) & (cj < geom.side)
            out[a, b] = int(lik[ci[ok].astype(np.int64), cj[ok].astype(np.int64)].astype(np.int64).sum())
    return out


def score_volume(lik: np.ndarray, src, gp: Params, geom: Geom, plant=None) -> np.ndarray:
    """L3: every candidate's score -> uint32 [NA][w][h] indexed [ia][tx - tx0][ty - ty0]"""
    side = geom.side
    tx0, ty0, w, h = region(gp, side)
    big = np.zeros((3 * side, 3 * side), dtype=np.uint8)
    big[side:2 * side, side:2 * side] = lik
    out = np.zeros((gp.ang_count, w, h), dtype=np.int64)
    for ia in range(gp.ang_count):
        if plant == "per_cell":
            out[ia] = _scores_per_cell(lik, src, ia, gp, geom)
            continue
        ox, oy, ok = offsets(src, ia, gp, geom.resolution, plant)
        out[ia] = _gather_sum(big, side, ox[ok], oy[ok], tx0, ty0, w, h, 1)
    assert out.max(initial=0) < 2 ** 32
    return out.astype(np.uint32)


def bound_volume(pool: np.ndarray, src, gp: Params, geom: Geom, plant=None) -> np.ndarray:
    """L5 -> uint32 [NA][nbx][nby]; pool is pool_map's array"""
    side = geom.side
    s, nbx, nby, _ = block_grid(gp, side)
    tx0, ty0, _, _ = region(gp, side)
    m = side + 2 * s
    big = np.zeros((3 * side + 4 * s, 3 * side + 4 * s), dtype=np.uint8)          # pool(i, j) at [i + m][j + m]
    big[m - (s - 1):m + side, m - (s - 1):m + side] = pool
    out = np.zeros((gp.ang_count, nbx, nby), dtype=np.int64)
    for ia in range(gp.ang_count):
        ox, oy, ok = offsets(src, ia, gp, geom.resolution, plant)
        out[ia] = _gather_sum(big, m, ox[ok], oy[ok], tx0, ty0, nbx, nby, s)
    return out.astype(np.uint32)


def block_maxima(scores: np.ndarray, s: int) -> np.ndarray:
    """the exact maximum of every block -> [NA][nbx][nby]"""
    na, w, h = scores.shape
    nbx, nby = -(-w // s), -(-h // s)
    pad = np.zeros((na, nbx * s, nby * s), dtype=scores.dtype)
    pad[:, :w, :h] = scores
    return pad.reshape(na, nbx, s, nby, s).max(axis=(2, 4))


@dataclass
class Info:
    """tbnav_icp_global_info (L7) but for refined_blocks and rounds, which are the implementation's"""
    searched: int
    accepted: int
    T: tuple
    ia: int
    tx: int
    ty: int
    score: int
    points: int
    occupied: int
    quality: float
    blocks: int


@dataclass
class Result:
    lik: np.ndarray
    pool: np.ndarray
    occupied: int
    bounds: np.ndarray
    scores: np.ndarray
    info: Info
    survivors: int          # the blocks whose bound reaches the best score: what any exact search has to refine (L6)


def localize(occ, geom: Geom, src, sp: S.Params = S.Params(), gp: Params = Params(), plant=None) -> Result:
    """tbnav_icp_localize_map and its hooks' arrays"""
    occ = np.asarray(occ).astype(bool)
    assert occ.shape == (geom.side, geom.side) and sp.resolution == geom.resolution and valid(gp, geom.side)
    src = np.asarray(src, dtype=np.float32).reshape(-1, 2)
    s, _, _, blocks = block_grid(gp, geom.side)
    lik = lik_map(occ, sp, plant)
    pool = pool_map(lik, s, plant)
    scores = score_volume(lik, src, gp, geom, plant)
    bounds = bound_volume(pool, src, gp, geom, plant)
    tx0, ty0, w, h = region(gp, geom.side)
    flat = scores.reshape(-1)
    best = int(flat.max())
    at = np.flatnonzero(flat == best)
    lin = int(at[-1] if plant == "tie_high" else at[0])          # [ia][tx][ty] order is L4's linear index order
    ia, rest = divmod(lin, w * h)
    a, b = divmod(rest, h)
    tx, ty = tx0 + a, ty0 + b
    points, occupied = int(src.shape[0]), int(occ.sum())
    quality = float(best) / (255.0 * float(points)) if points > 0 else 0.0
    accepted = int(quality >= gp.min_quality and points > 0 and occupied > 0)
    T = (float(ia) * gp.ang_step, geom.xmin + (float(tx) + 0.5) * geom.resolution, geom.ymin + (float(ty) + 0.5) * geom.resolution)
    info = Info(1, accepted, T, ia, tx, ty, best, points, occupied, quality, blocks)
    return Result(lik, pool, occupied, bounds, scores, info, int((bounds >= best).sum()))
