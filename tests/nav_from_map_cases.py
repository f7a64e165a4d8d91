"""The case table of the cost grid taken from a filter particle's occupancy (include/tbnav_nav.h G7-G8, csrc/nav_from_map.hip).  Plain
data with fixed seeds: map sizes, parameter sets, occupancy patterns, and the probe cells of the reach pattern.
tests/test_nav_from_map_cases.py proves the table on the CPU, tests/test_nav_from_map_gpu.py runs it.

Sizes are the smallest at which the kernel's tiling can go wrong: 64 (2 x 2 tiles of 32: every tile has neighbours outside the map), 96
(3 x 3: one tile with all eight neighbours), 80 (a ragged last tile of 16), and 24 cells of 0.5 m (tests/edt_cases.py's r20: one ragged
tile, another resolution).
"""
import zlib
from collections import namedtuple

import numpy as np

import edt_cases as ec

Size = namedtuple("Size", "id half res xsize radius")     # radius: the filter's own, ceil(10 / res)
SIZES = (Size("s64", 1.6, 0.05, 64, 200), Size("s96", 2.4, 0.05, 96, 200), Size("s80", 2.0, 0.05, 80, 200),
         Size("r20", ec.SIZE["r20"].half, ec.SIZE["r20"].res, ec.SIZE["r20"].xsize, ec.SIZE["r20"].radius))
SIZE = {s.id: s for s in SIZES}

# (r_robot, r_inflate, k).  At 0.05 m: R = 10 but for "R32" (ceil(1.55 / 0.05) + 1 = 32, the largest reach there is)
PARAMS_5CM = dict(base=(0.10, 0.45, 8.0), r_robot_0=(0.0, 0.45, 8.0), k_0=(0.10, 0.45, 0.0), k_63=(0.10, 0.45, 63.0), R32=(0.10, 1.55, 8.0))
# at 0.5 m: R = 2, R = 10 and R = 21 (nearly the whole 24-cell map)
PARAMS_50CM = dict(base=(0.10, 0.45, 8.0), r_robot_0_k_63=(0.0, 4.2, 63.0), wide=(0.6, 9.9, 8.0))
# tbnav_nav_inflation_tables alone: (resolution, r_robot, r_inflate, k)
TABLE_PARAMS = ((0.05, 0.10, 0.45, 8.0), (0.05, 0.0, 1.55, 63.0), (0.0625, 0.2, 0.3, 0.0), (2.5, 1.0, 9.9, 8.0),
                (0.05, 0.10, float(np.nextafter(0.45, 1.0)), 8.0))


def params(size):
    return PARAMS_50CM if size.id == "r20" else PARAMS_5CM


def _occ(size, cells=()):
    occ = np.zeros((size.xsize, size.xsize), dtype=np.uint8)
    for i, j in cells:
        occ[i, j] = 1
    return occ


# the one obstacle of the reach pattern: on the map's last row, so that cells R + 1 rows away exist for R = 32 on 64 cells
def reach_obstacle(size):
    return size.xsize - 1, size.xsize // 2


def patterns(size):
    """name -> occupancy [xsize][xsize] u8 (x the slow index), in a fixed order."""
    xs = size.xsize
    last = xs - 1
    rng = np.random.default_rng(zlib.crc32(size.id.encode()))
    out = {"empty": _occ(size),
           "corners": _occ(size, ((0, 0), (0, last), (last, 0), (last, last)))}
    if xs > 32:
        # either side of the seam between tiles in both axes, and the four cells round the corner four tiles share
        out["seam_rows"] = _occ(size, ((31, 7), (32, 20)))
        out["seam_cols"] = _occ(size, ((9, 31), (22, 32)))
        for n, c in enumerate(((31, 31), (31, 32), (32, 31), (32, 32))):
            out[f"four_corner_{n}"] = _occ(size, (c,))
        # one occupied tile among untouched ones (tile (1, 1), or what of it the map holds)
        one = _occ(size)
        hi = min(64, xs)
        one[32:hi, 32:hi] = rng.random((hi - 32, hi - 32)) < 0.05
        out["one_tile"] = one
    row, col = _occ(size), _occ(size)
    row[xs // 2 + 1, :] = 1
    col[:, xs // 2 + 1] = 1
    out["full_row"], out["full_col"] = row, col
    out["full_map"] = np.ones((xs, xs), dtype=np.uint8)
    out["random"] = (rng.random((xs, xs)) < 0.004).astype(np.uint8)
    if not out["random"].any():
        out["random"][int(rng.integers(xs)), int(rng.integers(xs))] = 1
    # two cells at equal distance from TIE_TARGET = (10, 10) in different rows: (7, 14) and (15, 10), both at 25; and for
    # MERGE_TARGET = (20, 14) a cell in its own row, (20, 23) at 81, that is farther than one two rows away, (22, 15) at 5 (a merge
    # that lets the first row with a bit decide gives 81 there)
    out["ties"] = _occ(size, ((7, 14), (15, 10), (20, 23), (22, 15)))
    out["reach"] = _occ(size, (reach_obstacle(size),))
    return out


TIE_TARGET, TIE_C, MERGE_TARGET, MERGE_C, MERGE_WRONG_C = (10, 10), 25, (20, 14), 5, 81


def reach_probes(size, R):
    """[(cell, c)] round the reach pattern's obstacle: at exactly R and R + 1 cells along the axis, one column beside the first
    (c = R*R + 1: inside the window, past the table), and the two diagonal offsets whose c lies closest to R*R from either side."""
    ox, oy = reach_obstacle(size)
    diag = [(a * a + b * b, a, b) for a in range(2, R + 1) for b in range(2, R + 1) if a <= ox and b <= oy]
    inside = max((t for t in diag if t[0] <= R * R), default=None)
    outside = min((t for t in diag if t[0] > R * R), default=None)
    probes = [((ox - R, oy), R * R), ((ox - R - 1, oy), (R + 1) * (R + 1)), ((ox - R, oy - 1), R * R + 1)]
    probes += [((ox - t[1], oy - t[2]), t[0]) for t in (inside, outside) if t is not None]
    return [(cell, c) for cell, c in probes if cell[0] >= 0 and cell[1] >= 0]


# ---- scenario U's walls as cells --------------------------------------------------------------------------------------------
U_FILTER = dict(xmin=-1.0, xmax=3.0, ymin=-2.0, ymax=2.0, resolution=0.05)      # nav_restatement.U_GRID as the filter's map
U_WALL_HALF = 0.03       # a cell is wall when its centre lies within this of a segment: the walls run along cell borders, so two cells thick


def scenario_u_occupancy():
    """nav_restatement.U_WALLS rasterised on U's 80 x 80 grid, u8 [80][80]."""
    import nav_restatement as nr
    return (nr.scenario_u_distance() <= U_WALL_HALF).astype(np.uint8)
