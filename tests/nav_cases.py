"""The goal field's case table (include/tbnav_nav.h): the smallest shapes at which csrc/nav.hip can go wrong — sides that are no
multiple of its 32-cell tile, goals on tile-corner cells, walls through a tile corner, rounds far beyond the tiles per side — each
with the restatement's answer computed once per process (tests/nav_restatement.py) and shared by the CPU and the GPU tests.
"""
from __future__ import annotations

import functools

import numpy as np

import nav_restatement as nr

GEOM = dict(xmin=-1.0, ymin=-2.0, resolution=0.05)   # every case's geometry but scenario U's own


def _drawn(nx, ny, seed, blocked=0.2):
    """Costs 1 .. 64 drawn uniformly, a fraction `blocked` of the cells set to 0."""
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 65, (nx, ny)).astype(np.uint8)
    c[rng.random((nx, ny)) < blocked] = 0
    return c


def _with_goal(cost, goal):
    """The goal cell clamped into the grid and made passable (a drawn grid may have blocked it)."""
    g = (min(goal[0], cost.shape[0] - 1), min(goal[1], cost.shape[1] - 1))
    if cost[g] == 0:
        cost = cost.copy(); cost[g] = 1
    return cost, g


def _diagonal_wall(gap):
    """40 x 40 at cost 1 with the single 8-connected wall ix + iy = 63 from (24, 39) to (39, 24): it passes through (31, 32) and
    (32, 31), so the forbidden move (31, 31) -> (32, 32) crosses a tile corner.  gap: one wall cell, (36, 27), left open."""
    c = np.ones((40, 40), dtype=np.uint8)
    for i in range(24, 40):
        c[i, 63 - i] = 0
    if gap:
        c[36, 27] = 1
    return c


def _enclosed():
    """20 x 20 at cost 3 with the goal inside a closed box of walls: everything outside the box is unreached."""
    c = np.full((20, 20), 3, dtype=np.uint8)
    c[6, 6:15] = 0; c[14, 6:15] = 0; c[6:15, 6] = 0; c[6:15, 14] = 0
    return c


SERPENTINE_N = 96
# corridors on the even rows, walls on the odd ones with a gap at alternating ends: 48 corridors of 95 moves and 47 gaps of 2, all
# straight (every diagonal move at a gap has a blocked cell beside it), at 10 * 64 each
SERPENTINE_LONGEST = (48 * 95 + 47 * 2) * 10 * 64


def _serpentine(n=SERPENTINE_N, cost=64):
    c = np.full((n, n), cost, dtype=np.uint8)
    for k in range(n // 2):
        c[2 * k + 1, :] = 0
        if 2 * k + 1 < n - 1:
            c[2 * k + 1, n - 1 if k % 2 == 0 else 0] = cost
    return c


# the same inside ONE tile at cost 3: 16 corridors of 31 moves and 15 gaps of 2, so the farthest of the 527 passable cells is 526
# straight moves away — more than a visit's sweeps can carry a front, which advances one cell per sweep along a corridor (a row's
# 32 cells are lanes of one wave): the tile runs into its sweep bound and wakes itself
SERPENTINE_IN_TILE_LONGEST = (16 * 31 + 15 * 2) * 10 * 3


def _room(n=400, seed=5, discs=12):
    """An n x n room of 0.05 m cells: nav_cost_from_distance (r_robot 0.10, r_inflate 0.45, k 8) of the analytic distance to the
    room's walls and to `discs` drawn discs."""
    res = GEOM["resolution"]
    X, Y = nr.cell_centres(n, n, 0.0, 0.0, res)
    side = n * res
    dist = np.minimum(np.minimum(X, side - X), np.minimum(Y, side - Y))
    rng = np.random.default_rng(seed)
    for _ in range(discs):
        cx, cy = rng.uniform(0.15, 0.85, 2) * side
        r = rng.uniform(0.02, 0.06) * side
        dist = np.minimum(dist, np.maximum(np.hypot(X - cx, Y - cy) - r, 0.0))
    return nr.nav_cost_from_distance(dist, 0.10, 0.45, 8.0)


def _first_free(cost, near):
    """The passable cell nearest to `near` (squared cell distance, ties to the lowest index)."""
    ix, iy = np.nonzero(cost)
    k = int(np.argmin((ix - near[0]) ** 2 + (iy - near[1]) ** 2))
    return int(ix[k]), int(iy[k])


def _build():
    cases = {}

    def add(name, cost, goal, starts=()):
        assert name not in cases and cost[goal] != 0
        cases[name] = dict(name=name, cost=np.ascontiguousarray(cost, dtype=np.uint8), goal=(int(goal[0]), int(goal[1])), starts=tuple(starts))

    for g in ((0, 0), (0, 1), (1, 0), (1, 1)):
        add(f"free_2x2_goal_{g[0]}{g[1]}", np.ones((2, 2), dtype=np.uint8), g)
    add("drawn_7x5", _drawn(7, 5, seed=75, blocked=0.0), (5, 1))     # non-square: swapped strides show
    for nx, ny in ((31, 33), (32, 32), (33, 31), (64, 65)):
        for goal in ((31, 31), (32, 32)):                           # tile-corner cells (clamped into the smaller grids)
            cost, g = _with_goal(_drawn(nx, ny, seed=100 * nx + ny), goal)
            if f"drawn_{nx}x{ny}_goal_{g[0]}_{g[1]}" not in cases:
                add(f"drawn_{nx}x{ny}_goal_{g[0]}_{g[1]}", cost, g)
    add("diagonal_wall_closed", _diagonal_wall(gap=False), (20, 20), starts=[(39, 0), (0, 39), (31, 31)])
    add("diagonal_wall_gap", _diagonal_wall(gap=True), (20, 20), starts=[(39, 0), (32, 32), (39, 39)])
    add("enclosed_goal", _enclosed(), (10, 10))
    add("serpentine_96", _serpentine(), (0, 0))
    add("serpentine_in_tile_32", _serpentine(32, 3), (0, 0))
    add("empty_400", np.ones((400, 400), dtype=np.uint8), (0, 0), starts=[(399, 100), (123, 399)])
    room = _room()
    add("room_400", room, _first_free(room, (350, 380)))
    rng = np.random.default_rng(2024)
    for i in range(30):
        nx, ny = (int(v) for v in rng.integers(2, 101, 2))
        cost = _drawn(nx, ny, seed=9000 + i, blocked=float(rng.choice([0.0, 0.1, 0.2, 0.3])))
        cost, g = _with_goal(cost, (int(rng.integers(0, nx)), int(rng.integers(0, ny))))
        add(f"seeded_{i:02d}_{nx}x{ny}", cost, g)
    return cases


CASES = _build()
NAMES = list(CASES)
SMALL = [n for n in NAMES if max(CASES[n]["cost"].shape) <= 100]     # what the numpy Bellman-Ford sweep is run on
WALL_CASES = ["diagonal_wall_closed", "diagonal_wall_gap"]
PATH_TIE_CASES = ["empty_400", "diagonal_wall_closed", "diagonal_wall_gap"]    # cases whose walks meet ties (G6's order decides)


def _sequence():
    """Two solves and a set_cost in a row on one 64 x 65 handle: (cost, or None to keep the grid; goal)."""
    a = CASES["drawn_64x65_goal_31_31"]["cost"]
    b, goal_b = _with_goal(_drawn(64, 65, seed=4242, blocked=0.3), (32, 32))
    return [(a, (31, 31)), (None, _first_free(a, (63, 64))), (b, goal_b)]


SEQUENCE = _sequence()


@functools.lru_cache(maxsize=None)
def _expected_of(cost_bytes, shape, goal):
    return nr.cost_to_go(np.frombuffer(cost_bytes, dtype=np.uint8).reshape(shape), goal)


def expected_for(cost, goal):
    """The restatement's cost-to-go of (cost, goal), computed once per process; treat it as read-only."""
    cost = np.ascontiguousarray(cost, dtype=np.uint8)
    d = _expected_of(cost.tobytes(), cost.shape, (int(goal[0]), int(goal[1])))
    d.setflags(write=False)
    return d


def expected(name):
    return expected_for(CASES[name]["cost"], CASES[name]["goal"])


def starts(name):
    """The walks a case is asked for: from the farthest reached cell, from the reached cells with the lowest and the highest index,
    from the goal (a path of one cell), and from the cells the table names (where ties or a wall are met)."""
    d = expected(name)
    flat = d.ravel().astype(np.int64)
    reached = np.nonzero(flat != nr.UNREACHED)[0]
    picks = [int(reached[np.argmax(flat[reached])]), int(reached[0]), int(reached[-1]), int(np.nonzero(flat == 0)[0][0])]
    ny = d.shape[1]
    out = []
    for cell in [(p // ny, p % ny) for p in picks] + list(CASES[name]["starts"]):
        if cell not in out and d[cell] != nr.UNREACHED:
            out.append(cell)
    return out


def refusing_start(name):
    """A blocked or unreached cell of the case (G6: TBNAV_ERR_UNSUPPORTED), or None."""
    d = expected(name)
    bad = np.nonzero(d.ravel() == nr.UNREACHED)[0]
    return (int(bad[0]) // d.shape[1], int(bad[0]) % d.shape[1]) if len(bad) else None
