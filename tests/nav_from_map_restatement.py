"""TEST INFRASTRUCTURE — restatement of the cost grid taken from a filter particle's occupancy (include/tbnav_nav.h, G7-G8) in numpy.

G7's tables are the host route's own formulas (nav_restatement.nav_cost_from_distance, mppi_field_restatement.cost_field_from_distance)
evaluated at d(c) = sqrt(c) * resolution; G8's c(cell) is a brute-force minimum over the window.  Nothing in the product imports this
file.
"""
from __future__ import annotations

import math

import numpy as np

from mppi_field_restatement import cost_field_from_distance
from nav_restatement import nav_cost_from_distance

MAX_REACH, MAX_OCC_DIST = 32, 10.0
NONE = np.iinfo(np.int64).max      # c of a cell with nothing occupied in its window


# ---- G7 ---------------------------------------------------------------------------------------------------------------------
def check_args(resolution, r_robot, r_inflate, k):
    """None, or the status name the header gives: "INVALID_ARG" / "UNSUPPORTED"."""
    v = (resolution, r_robot, r_inflate, k)
    if not all(math.isfinite(x) for x in v) or not resolution > 0.0 or not (0.0 <= r_robot < r_inflate <= MAX_OCC_DIST) or not (0.0 <= k <= 63.0):
        return "INVALID_ARG"
    return "UNSUPPORTED" if math.ceil(r_inflate / resolution) + 1 > MAX_REACH else None


def reach(resolution, r_inflate):
    return int(math.ceil(r_inflate / resolution)) + 1


def tables(resolution, r_robot, r_inflate, k):
    """(cost uint8, field float32, R): the entries c = 0 .. R*R followed by the open value (that of d = 10.0)."""
    assert check_args(resolution, r_robot, r_inflate, k) is None
    R = reach(resolution, r_inflate)
    d = np.append(np.sqrt(np.arange(R * R + 1).astype(np.float64)) * resolution, MAX_OCC_DIST)
    return nav_cost_from_distance(d, r_robot, r_inflate, k), cost_field_from_distance(d, r_robot, r_inflate), R


# ---- G8 ---------------------------------------------------------------------------------------------------------------------
def nearest_c(occ, R):
    """int64 [nx][ny]: the minimum of di^2 + dj^2 over occupied cells with |di|, |dj| <= R; NONE where there is none.  Brute force:
    every offset of the window in turn."""
    occ = np.asarray(occ).astype(bool)
    nx, ny = occ.shape
    best = np.full((nx, ny), NONE, dtype=np.int64)
    for di in range(-R, R + 1):
        xa, xb = max(0, -di), min(nx, nx - di)          # cells ix in xa .. xb - 1 have ix + di inside
        if xa >= xb:
            continue
        for dj in range(-R, R + 1):
            ya, yb = max(0, -dj), min(ny, ny - dj)
            if ya >= yb:
                continue
            hit = occ[xa + di:xb + di, ya + dj:yb + dj]
            view = best[xa:xb, ya:yb]
            np.minimum(view, np.where(hit, di * di + dj * dj, NONE), out=view)
    return best


def lookup(c, table, R):
    """table[c] where c <= R*R, the open value (the table's last entry) elsewhere."""
    inside = c <= R * R
    return np.where(inside, table[np.where(inside, c, 0)], table[-1])


def cost_from_occ(occ, resolution, r_robot, r_inflate, k, c=None):
    cost, _, R = tables(resolution, r_robot, r_inflate, k)
    return lookup(nearest_c(occ, R) if c is None else c, cost, R)


def field_from_occ(occ, resolution, r_robot, r_inflate, c=None):
    _, field, R = tables(resolution, r_robot, r_inflate, 0.0)
    return lookup(nearest_c(occ, R) if c is None else c, field, R)


def first_row_c(occ, R):
    """A WRONG merge, for the cases to tell apart: the rows at distance 0, 1, 1, 2, 2 .. are taken in turn and the first that holds an
    occupied cell within R columns decides, instead of the minimum over all rows."""
    occ = np.asarray(occ).astype(bool)
    nx, ny = occ.shape
    out = np.full((nx, ny), NONE, dtype=np.int64)
    cols = np.arange(ny)
    for ix in range(nx):
        for iy in range(ny):
            for dr in range(R + 1):
                found = None
                for r in ((ix,) if dr == 0 else (ix - dr, ix + dr)):
                    if 0 <= r < nx:
                        dc = np.abs(cols[occ[r]] - iy)
                        dc = dc[dc <= R]
                        if dc.size and (found is None or int(dc.min()) < found):
                            found = int(dc.min())
                if found is not None:
                    out[ix, iy] = dr * dr + found * found
                    break
    return out
