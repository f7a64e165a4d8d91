"""The case table of the frontiers ranked by information gain (include/tbnav_nav.h G17-G20, csrc/nav_gain.hip).  Plain data: log-odds
grids drawn from nav_frontier_cases' five values, cost grids, thresholds and ranges; and the ranked plan of the exploration loop.
tests/test_nav_gain_cases.py proves on the CPU that each case reaches what it names, tests/test_nav_gain_gpu.py runs the table.

Sizes are nav_from_map_cases.SIZES: 64 (2 x 2 tiles), 96 (3 x 3), 80 (a ragged last tile), 24 cells of 0.5 m (one ragged tile).  Every
viewpoint is a seed of the find, so a case places FREE cells beside UNKNOWN ones where it wants to look from (min_cells is 1 but where
the case is about the threshold).

The nook and the doorway (s96, cost 1 off the walls, R = 16, min_cells 8): a FREE room [20..60]^2 inside OCCUPIED walls; a 10-cell gap
in the wall ix = 19 (iy 24 .. 33) that leads into a walled pocket of 50 unknown cells; a 16-cell gap in the wall ix = 61 (iy 44 .. 59)
that leads into open unknown space; the robot at (25, 28).  tests/nav_gain_restatement.py gives: 26 frontier cells, all seeds; the
pocket's ten gains all 50; the doorway's 348, 377, 386, 393 x 4, 398 x 2 and back, gain_max 398 first at (61, 51).  The path from
(25, 28) ends
    weight 0:    at (19, 28) in the pocket, d = start = 0, 7 cells;
    weight 1:    at (19, 28) in the pocket, d = start = 348 — not 0: the case that needs G20's stop rule;
    weight 2:    at (61, 47) in the doorway, d = start = 10 (its gain is 393), 37 cells;
    weight 8:    at (61, 51) in the doorway, d = start = 0, 37 cells;
    weight 4096: at (61, 51) in the doorway.
The plan flips between the adjacent weights 1 and 2.

The exploration loop with the ranked plan (EXPLORE_GAIN_RANGE = 40 cells, EXPLORE_GAIN_WEIGHT = 1; nav_frontier_cases.explore over the
oracle's GridMapper and the restatements).  Asserted: that it ends with no seed left within EXPLORE_MAX_ITER.  Recorded, with no claim
that ranked is the better plan — nobody has measured that:
    start (-2.0, 1.5): nearest 24 iterations, 9 marks, 5 unknown cells left inside; ranked 16 iterations, 1 mark, 5 unknown cells left;
    start ( 0.0, 0.0): nearest 18 iterations, 0 marks, 2 unknown cells left inside; ranked 14 iterations, 0 marks, 7 unknown cells left.
"""
from collections import namedtuple

import numpy as np

import nav_frontier_cases as fcs

SIZES, SIZE = fcs.SIZES, fcs.SIZE
U, F, F2, O, K = fcs.U, fcs.F, fcs.F2, fcs.O, fcs.K

Case = namedtuple("Case", "lo cost discs min_cells R")     # nav_frontier_cases.Case and the range in cells
RANGES = (1, 2, 3, 8, 31, 32, 33, 48, 128)                 # 32 and 33 take different instantiations of nav_frontier_gain
WEIGHTS = (0, 1, 2, 4096)
R_SMALL = 8


def _case(xs, fill, cells=(), R=R_SMALL, cost=None, min_cells=1):
    lo = np.full((xs, xs), fill, dtype=np.float64)
    for (x0, x1, y0, y1), v in cells:       # inclusive ranges, later ones over earlier ones
        lo[x0:x1 + 1, y0:y1 + 1] = v
    return Case(lo, fcs.base_cost(xs) if cost is None else cost, (), min_cells, R)


def _one(x, y, v):
    return ((x, x, y, y), v)


def diag_wall_lo(xs):
    """OCCUPIED where ix - iy == 5, from one side of the map to the other: a wall that is only 8-connected.  Known and neither on the
    viewpoint's side, UNKNOWN behind; the viewpoint (8, 8) is a seed by the one unknown cell (8, 7) beside it."""
    X, Y = np.meshgrid(np.arange(xs), np.arange(xs), indexing="ij")
    lo = np.where(X - Y > 5, U, np.where(X - Y == 5, O, K))      # (an odd offset: the diagonal steps from (8, 8) jump it)
    lo[8, 8], lo[8, 7] = F, U
    return lo


def seam_cells(xs):
    """FREE cells in an unknown map: iy = 0, 31, 32 and last, ix = 31 and 32 (one ragged tile: the map's sides)."""
    last = xs - 1
    if xs > 32:
        return ((31, 0), (32, 31), (31, 32), (32, last), (0, 31), (last, 32))
    return ((5, 0), (5, last), (0, 5), (last, 5))


def ranges_lo(xs):
    """A FREE block of 4 x 4 across the corner four tiles share (in the middle of the one ragged tile), twelve of its cells seeds, in an
    unknown map with a wall, a known patch and single occupied cells round it."""
    lo = np.full((xs, xs), U, dtype=np.float64)
    a = 30 if xs > 32 else 10
    lo[a:a + 4, a:a + 4] = F
    lo[a + 10, max(0, a - 10):min(xs, a + 21)] = O
    lo[a - 9:a - 4, a + 4:min(xs, a + 14)] = K
    for dx, dy in ((-3, -2), (2, 7), (-6, 1), (5, -5), (1, -8)):
        lo[a + dx, a + dy] = O
    return lo


# ---- the nook and the doorway -----------------------------------------------------------------------------------------------
NOOK_SIZE, NOOK_START, NOOK_R, NOOK_MIN_CELLS = "s96", (25, 28), 16, 8
NOOK_POCKET_GAP, NOOK_DOOR_GAP = (24, 33), (44, 59)         # iy ranges, inclusive, in the walls ix = 19 and ix = 61
NOOK_ENDS = {0: (19, 28), 1: (19, 28), 2: (61, 47), 8: (61, 51), 4096: (61, 51)}      # weight -> the path's last cell (the restatement's)
NOOK_FLIP = (1, 2)


def nook():
    lo = np.full((96, 96), U, dtype=np.float64)
    lo[19:62, 19:62] = O
    lo[20:61, 20:61] = F
    p0, p1 = NOOK_POCKET_GAP
    lo[13:19, p0 - 1:p1 + 2] = O             # the pocket's walls ...
    lo[14:19, p0:p1 + 1] = U                 # ... round its 5 x 10 unknown cells
    lo[19, p0:p1 + 1] = F                    # the gap in the wall ix = 19
    d0, d1 = NOOK_DOOR_GAP
    lo[61, d0:d1 + 1] = F                    # the gap in the wall ix = 61
    return Case(lo, np.where(lo == O, 0, 1).astype(np.uint8), (), NOOK_MIN_CELLS, NOOK_R)


def in_pocket_gap(cell):
    return cell[0] == 19 and NOOK_POCKET_GAP[0] <= cell[1] <= NOOK_POCKET_GAP[1]


def in_door_gap(cell):
    return cell[0] == 61 and NOOK_DOOR_GAP[0] <= cell[1] <= NOOK_DOOR_GAP[1]


def cases(size):
    """name -> Case, in a fixed order."""
    xs = size.xsize
    last = xs - 1
    out = {}
    # distinct count: a FREE strip in front of an open unknown half-plane; the rays of a viewpoint overlap near it
    out["open_half"] = _case(xs, U, [((0, 9, 0, last), F)])
    # a wall one cell thick, two unknown rows in front of it, unknown behind
    out["wall"] = _case(xs, U, [((0, 9, 0, last), F), ((12, 12, 0, last), O)])
    out["diag_wall"] = Case(diag_wall_lo(xs), fcs.base_cost(xs), (), 1, R_SMALL)
    # one occupied cell beside the first diagonal step, unknown cells along that diagonal
    out["corner_graze"] = _case(xs, K, [_one(10, 10, F), _one(9, 10, U), _one(11, 10, O), _one(11, 11, U), _one(12, 12, U), _one(13, 13, U)])
    # FREE and known-neither cells between the viewpoint and three unknown ones
    out["pass_through"] = _case(xs, K, [_one(10, 10, F), _one(9, 10, U), _one(10, 11, F), _one(10, 12, K), _one(10, 13, F2), _one(10, 14, K),
                                        ((10, 10, 15, 17), U)])
    if xs > 32:
        # the unknown half is in tiles nobody has written (id 0)
        out["id0_half"] = _case(xs, U, [((0, 31, 0, last), F)])
    # viewpoints in the map's corners: most rays end at the map's side (on s80 and r20 in a ragged tile)
    out["corners"] = _case(xs, U, [_one(0, 0, F), _one(last, last, F)])
    out["corners_R128"] = _case(xs, U, [_one(0, 0, F), _one(last, last, F)], R=128)
    out["seams"] = _case(xs, U, [_one(x, y, F) for x, y in seam_cells(xs)], R=33)
    # unknown cells at bit offsets 0 and 31 only, seen from either side of the word seam
    cols = [c for c in (0, 31, 32, 63) if c < xs] + [last]
    out["seam_bits"] = _case(xs, K, [((0, last, c, c), U) for c in cols] + [_one(5, 1, F), _one(min(31, last - 2), last - 1, F)] +
                             ([_one(32, 30, F), _one(31, 33, F)] if xs > 32 else []), R=32)
    for R in RANGES:
        out[f"ranges_R{R}"] = Case(ranges_lo(xs), fcs.base_cost(xs), (), 1, R)
    # the ray to (8, 1) steps aside at s = 4, not at s = 8; (7, 2) and (5, 3) are entered by the rounded steps only
    out["rounding"] = _case(xs, K, [_one(10, 10, F), _one(9, 10, U), _one(17, 12, U), _one(15, 13, U)])
    # clusters of min_cells - 1 and min_cells cells
    out["min_cells_edge"] = _case(xs, U, [((5, 5, 2, 8), F), ((9, 9, 2, 9), F2)], min_cells=fcs.MIN_CELLS)
    # two viewpoints that see two cells each, one that sees one
    out["tie"] = _case(xs, K, [_one(4, 10, F), ((2, 3, 10, 10), U), _one(12, 10, F), ((10, 11, 10, 10), U), _one(20, 10, F), _one(19, 10, U)], R=3)
    out["no_seed"] = _case(xs, F)
    if size.id == NOOK_SIZE:
        out["nook"] = nook()
    return out


# the planted errors (switches of nav_gain_restatement.seen) and the case each must change
PLANTED = (("leaky", "diag_wall"), ("either", "corner_graze"), ("per_ray", "open_half"), ("trunc", "rounding"), ("count_occ", "wall"))


# ---- the exploration loop with the ranked plan ------------------------------------------------------------------------------
EXPLORE_GAIN_RANGE, EXPLORE_GAIN_WEIGHT = 40, 1
