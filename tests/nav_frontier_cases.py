"""The case table of the exploration frontiers (include/tbnav_nav.h G10-G16, csrc/nav_frontier.hip).  Plain data: map sizes, log-odds
grids drawn from five values, cost grids, visited discs and thresholds; and the exploration loop both legs run.
tests/test_nav_frontier_cases.py proves on the CPU that each case reaches what it names, tests/test_nav_frontier_gpu.py runs the table.

Sizes are nav_from_map_cases.SIZES: 64 (2 x 2 tiles), 96 (3 x 3), 80 (a ragged last tile), 24 cells of 0.5 m (one ragged tile).

The exploration loop (explore): SURVEY 8-d's room on a +-4 m map of 0.05 m cells, theta = 0, room_scan's noise from default_rng(7),
inflation (0.10, 0.45, 8.0), min_cells 8; the robot jumps 12 cells along the path per iteration and marks a disc of 10 cells where the
path has at most 3 cells.  With the cost grid formed by nav_from_map_restatement (the first probe of the definition used scipy's EDT and
gave 23 iterations / 9 marks / 0 unknown cells and 13 / 0 / 1), the oracle's GridMapper and nav_frontier_restatement give:
    start (-2.0, 1.5): 24 iterations, 9 marks, 5 unknown cells of the 10716 more than 0.15 m inside the walls at the end;
    start ( 0.0, 0.0): 18 iterations, 0 marks, 2 unknown cells.
"""
from collections import namedtuple

import numpy as np

import nav_from_map_cases as fc

SIZES, SIZE = fc.SIZES, fc.SIZE

L_FREE, L_OCC = float(np.log(0.35 / (1 - 0.35))), float(np.log(0.9 / (1 - 0.9)))
U, F, F2, O, K = 0.0, L_FREE, 2 * L_FREE, L_OCC, L_OCC + L_FREE      # unknown, free, free twice seen, occupied, known and neither (0.829)
VALUES = (U, F, F2, O, K)

Case = namedtuple("Case", "lo cost discs min_cells")     # lo f64 [xs][xs] (x slow), cost u8 [xs][xs], discs ((ix, iy, r), ...)
MIN_CELLS = 8


def base_cost(xs):
    """Passable everywhere, 1 .. 5 in a fixed pattern: the solves' costs-to-go are not plain distances."""
    X, Y = np.meshgrid(np.arange(xs), np.arange(xs), indexing="ij")
    return (1 + (X * 7 + Y * 3) % 5).astype(np.uint8)


def _case(xs, fill, cells=(), cost=None, discs=(), min_cells=MIN_CELLS):
    lo = np.full((xs, xs), fill, dtype=np.float64)
    for (x0, x1, y0, y1), v in cells:       # inclusive ranges
        lo[x0:x1 + 1, y0:y1 + 1] = v
    return Case(lo, base_cost(xs) if cost is None else cost, tuple(discs), min_cells)


def diag_start(xs):
    """Where the diagonal chain of eight cells starts: through the corner four tiles share, (31, 31)-(32, 32), where there is one."""
    return 28 if xs > 32 else 8


def serpentine_rows(xs):
    return min(xs, 32) - 1       # rows 0, 2, .. of one tile, joined at alternate ends: one chain one cell wide


def cases(size):
    """name -> Case, in a fixed order."""
    xs = size.xsize
    last = xs - 1
    out = {"all_unknown": _case(xs, U), "all_free": _case(xs, F)}
    if xs > 32:
        # a free half-plane ending on row / column 31 and 32: the unknown neighbour is in the next tile, which nobody has written
        out["half_row31"] = _case(xs, U, [((0, 31, 0, last), F)])
        out["half_row32"] = _case(xs, U, [((0, 32, 0, last), F)])
        out["half_col31"] = _case(xs, U, [((0, last, 0, 31), F2)])
        out["half_col32"] = _case(xs, U, [((0, last, 0, 32), F2)])
        # ... and once with that tile written: an occupied cell in it, far from the border
        out["half_row31_touched"] = _case(xs, U, [((0, 31, 0, last), F), ((40, 40, 5, 5), O), ((40, 40, 40, 40), O)])
        out["half_col31_touched"] = _case(xs, U, [((0, last, 0, 31), F), ((5, 5, 40, 40), K), ((40, 40, 40, 40), K)])
    # free cells on the map's edge, everything else known: outside the grid is not unknown
    out["edge_free"] = _case(xs, K, [((0, 0, 5, 9), F), ((last, last, 3, 12), F), ((4, 11, 0, 0), F), ((2, 9, last, last), F)])
    k0 = diag_start(xs)
    out["diag_chain"] = _case(xs, U, [((k, k, k, k), F) for k in range(k0, k0 + 8)])
    out["two_runs"] = _case(xs, U, [((10, 10, 5, 14), F), ((12, 12, 5, 14), F)])
    rows = serpentine_rows(xs)
    width = min(xs, 32) - 1
    serp = [((r, r, 0, width), F) for r in range(0, rows, 2)]
    serp += [((r, r, width, width) if (r // 2) % 2 == 0 else (r, r, 0, 0), F) for r in range(1, rows - 1, 2)]
    out["serpentine"] = _case(xs, U, serp)
    blocked = base_cost(xs)
    blocked[10, 12] = 0
    out["blocked_split"] = _case(xs, U, [((10, 10, 4, 20), F)], cost=blocked)
    out["visited_part"] = _case(xs, U, [((20, 20, 4, 20), F)], discs=((20, 18, 3),))
    out["min_cells_edge"] = _case(xs, U, [((5, 5, 2, 8), F), ((9, 9, 2, 9), F2)])
    out["known_neither"] = _case(xs, K, [((10, 14, 10, 14), F), ((3, 3, 3, 6), O)])
    # an unknown cell seen only across a corner is no reason; one seen across an edge is
    out["diagonal_unknown"] = _case(xs, K, [((10, 10, 10, 10), U), ((11, 11, 11, 11), F), ((20, 20, 20, 20), F), ((20, 20, 21, 21), U)], min_cells=1)
    return out


# the planted errors (switches of nav_frontier_restatement.find) and the case each must change
PLANTED = (("look8", "diagonal_unknown"), ("conn4", "diag_chain"), ("outside_unknown", "edge_free"), ("strict", "min_cells_edge"),
           ("keep_blocked", "blocked_split"))


def visited_mask(xs, discs):
    import nav_frontier_restatement as ff
    v = np.zeros((xs, xs), dtype=bool)
    for ix, iy, r in discs:
        v |= ff.disc(xs, xs, ix, iy, r)
    return v


# ---- the exploration loop ---------------------------------------------------------------------------------------------------
EXPLORE_MAP = dict(half=4.0, res=0.05, xsize=160)
EXPLORE_INFLATION = (0.10, 0.45, 8.0)
EXPLORE_STARTS = ((-2.0, 1.5), (0.0, 0.0))
EXPLORE_JUMP, EXPLORE_MARK_RADIUS, EXPLORE_SHORT_PATH, EXPLORE_MAX_ITER, EXPLORE_SEED = 12, 10, 3, 60, 7
EXPLORE_INSIDE, EXPLORE_MAX_UNKNOWN = 0.15, 0.01


def explore_cell_centre(cell):
    m = EXPLORE_MAP
    return -m["half"] + (cell[0] + 0.5) * m["res"], -m["half"] + (cell[1] + 0.5) * m["res"]


def explore(start, integrate, plan, mark):
    """The loop.  integrate(scan, pose): the scan goes into the map at pose (theta, x, y); plan(cell) -> None where no seed is left, else
    the path int32 [n][2] from the robot's cell to the nearest seed; mark(cell): a disc of EXPLORE_MARK_RADIUS joins the visited mask.
    Returns dict(cells=[the robot's cell at every iteration], marks=[iterations that marked], done=ended by "no seed")."""
    import nav_restatement as nr
    import oracle_api as orc
    import rbpf_cases as rc
    m = EXPLORE_MAP
    rng = np.random.default_rng(EXPLORE_SEED)
    x, y = start
    cells, marks = [], []
    for it in range(EXPLORE_MAX_ITER):
        integrate(orc.room_scan((0.0, x, y), walls=rc.ROOM_SURVEY, rng=rng), (0.0, x, y))
        cell = nr.cell_of(m["xsize"], m["xsize"], -m["half"], -m["half"], m["res"], x, y)
        cells.append(cell)
        path = plan(cell)
        if path is None:
            return dict(cells=cells, marks=marks, done=True)
        if len(path) <= EXPLORE_SHORT_PATH:
            mark(cell)
            marks.append(it)
        else:
            x, y = explore_cell_centre(tuple(int(v) for v in path[min(EXPLORE_JUMP, len(path) - 1)]))
    return dict(cells=cells, marks=marks, done=False)


def explore_unknown_inside(exported):
    """(unknown cells, cells) among those whose centre lies more than EXPLORE_INSIDE inside the room's walls."""
    import rbpf_cases as rc
    m = EXPLORE_MAP
    xs = m["xsize"]
    c = -m["half"] + (np.arange(xs) + 0.5) * m["res"]
    X, Y = np.meshgrid(c, c, indexing="ij")
    x0, x1, y0, y1 = rc.ROOM_SURVEY
    inside = (X > x0 + EXPLORE_INSIDE) & (X < x1 - EXPLORE_INSIDE) & (Y > y0 + EXPLORE_INSIDE) & (Y < y1 - EXPLORE_INSIDE)
    grid = np.asarray(exported, dtype=np.int8).reshape(xs, xs).T
    return int(((grid == -1) & inside).sum()), int(inside.sum())
