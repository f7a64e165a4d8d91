"""CPU tests of the goal field's restatement (tests/nav_restatement.py) and case table (tests/nav_cases.py): the Dijkstra against
a plain numpy Bellman-Ford sweep, each case reaching what it names, and scenario U meeting its conditions — which is what makes
them conditions for the device leg (tests/test_nav_gpu.py) and not hopes."""
import numpy as np
import pytest

import mppi_field_restatement as fr
import nav_cases as nc
import nav_restatement as nr

BIG = np.int64(1) << 40


def _shift(padded, dx, dy, nx, ny):
    """a[ix + dx][iy + dy] for every (ix, iy), from the array padded by one cell."""
    return padded[1 + dx:1 + dx + nx, 1 + dy:1 + dy + ny]


def bellman_ford(cost, goal, corner_rule=True):
    """G3-G4 as whole-array sweeps to the fixed point: written apart from the Dijkstra (no heap, no per-cell rule function)."""
    c = np.asarray(cost).astype(np.int64)
    nx, ny = c.shape
    cp = np.pad(c, 1)                       # outside the grid: blocked
    free = c != 0
    d = np.full((nx, ny), BIG); d[goal] = 0
    while True:
        dp = np.pad(d, 1, constant_values=BIG)
        new = d
        for dx, dy, w in nr.MOVES:
            cb, db = _shift(cp, dx, dy, nx, ny), _shift(dp, dx, dy, nx, ny)
            ok = free & (cb != 0) & (db < BIG)
            if corner_rule and dx != 0 and dy != 0:
                ok = ok & (_shift(cp, 0, dy, nx, ny) != 0) & (_shift(cp, dx, 0, nx, ny) != 0)
            new = np.minimum(new, np.where(ok, db + w * cb, BIG))
        if np.array_equal(new, d):
            return np.where(d == BIG, nr.UNREACHED, d).astype(np.uint32)
        d = new


@pytest.mark.parametrize("name", nc.SMALL)
def test_dijkstra_equals_the_bellman_ford_sweep(name):
    case = nc.CASES[name]
    assert np.array_equal(nc.expected(name), bellman_ford(case["cost"], case["goal"]))


def test_the_table_holds_what_the_issue_names():
    shapes = {nc.CASES[n]["cost"].shape for n in nc.NAMES}
    assert {(2, 2), (7, 5), (31, 33), (32, 32), (33, 31), (64, 65), (40, 40), (96, 96), (400, 400)} <= shapes
    assert sum(n.startswith("seeded_") for n in nc.NAMES) == 30
    assert all(2 <= s <= 100 for n in nc.NAMES if n.startswith("seeded_") for s in nc.CASES[n]["cost"].shape)
    goals = {nc.CASES[n]["goal"] for n in nc.NAMES if n.startswith("drawn_")}
    assert (31, 31) in goals and (32, 32) in goals
    for n in nc.NAMES:
        c = nc.CASES[n]["cost"]
        assert c.dtype == np.uint8 and c.max() <= nr.MAX_COST and c[nc.CASES[n]["goal"]] != 0
    for n in ("drawn_31x33_goal_30_31", "drawn_64x65_goal_32_32"):
        frac = float((nc.CASES[n]["cost"] == 0).mean())
        assert 0.1 < frac < 0.3, frac


@pytest.mark.parametrize("name", nc.WALL_CASES)
def test_the_corner_rule_changes_the_answer_on_the_wall_cases(name):
    """Without G3's rule for diagonal moves the single 8-connected wall leaks: the far side is reached where it must not be (closed
    wall), or reached more cheaply than through the gap."""
    case = nc.CASES[name]
    with_rule, without = nc.expected(name), nr.cost_to_go(case["cost"], case["goal"], corner_rule=False)
    assert np.array_equal(without, bellman_ford(case["cost"], case["goal"], corner_rule=False))
    far = (39, 39)
    assert case["cost"][31, 32] == 0 and case["cost"][32, 31] == 0 and case["cost"][31, 31] != 0 and case["cost"][32, 32] != 0
    assert without[far] != nr.UNREACHED and without[32, 32] == without[31, 31] + 14      # the leak: straight through the tile corner
    if name == "diagonal_wall_closed":
        assert with_rule[far] == nr.UNREACHED and with_rule[32, 32] == nr.UNREACHED
        ix, iy = np.indices(with_rule.shape)
        assert np.array_equal(with_rule == nr.UNREACHED, ix + iy >= 63)               # the wall and all of the far side
    else:
        assert nr.UNREACHED > with_rule[far] > without[far]
        assert int((with_rule == nr.UNREACHED).sum()) == 15                           # the wall's cells but the gap


def test_the_enclosed_goal_reaches_the_inside_of_its_box_only():
    d = nc.expected("enclosed_goal")
    reached = d != nr.UNREACHED
    assert reached[7:14, 7:14].all() and int(reached.sum()) == 49


def test_the_serpentines_longest_distance_is_its_closed_form():
    d = nc.expected("serpentine_96")
    reached = d[d != nr.UNREACHED]
    assert int(reached.max()) == nc.SERPENTINE_LONGEST == int(d[94, 0])
    assert len(reached) == 48 * 96 + 47
    d = nc.expected("serpentine_in_tile_32")
    reached = d[d != nr.UNREACHED]
    assert int(reached.max()) == nc.SERPENTINE_IN_TILE_LONGEST == 15780 == int(d[30, 0])
    assert len(reached) == 16 * 32 + 15 == int((nc.CASES["serpentine_in_tile_32"]["cost"] != 0).sum())


@pytest.mark.parametrize("name", nc.PATH_TIE_CASES)
def test_ties_occur_on_the_path_cases_so_the_order_matters(name):
    case, d = nc.CASES[name], nc.expected(name)
    ties = differ = 0
    for s in nc.starts(name):
        p, t = nr.path(case["cost"], d, s)
        q, _ = nr.path(case["cost"], d, s, last_wins=True)
        assert tuple(p[0]) == s and tuple(p[-1]) == case["goal"] and tuple(q[-1]) == case["goal"]
        step = np.abs(np.diff(p, axis=0))
        assert step.max(initial=0) <= 1 and (np.diff(d[p[:, 0], p[:, 1]].astype(np.int64)) < 0).all()    # neighbours, d falls strictly
        ties += t
        differ += not np.array_equal(p, q)
    assert ties > 0 and differ > 0


def test_path_refuses_blocked_and_unreached_starts():
    for name in ("diagonal_wall_closed", "enclosed_goal"):
        case, d = nc.CASES[name], nc.expected(name)
        with pytest.raises(ValueError):
            nr.path(case["cost"], d, nc.refusing_start(name))
    case, d = nc.CASES["diagonal_wall_closed"], nc.expected("diagonal_wall_closed")
    assert case["cost"][39, 39] != 0
    with pytest.raises(ValueError):
        nr.path(case["cost"], d, (39, 39))     # passable, but behind the wall


def test_cell_of_and_field_restated():
    g = nc.GEOM
    assert nr.cell_of(7, 5, **g, x=-1.0, y=-2.0) == (0, 0)
    assert nr.cell_of(7, 5, **g, x=-0.6501, y=-1.7501) == (6, 4)
    for x, y in ((-1.0001, -2.0), (-1.0, -2.0001), (-0.65, -2.0), (-1.0, -1.75), (np.nan, -2.0), (-1.0, np.inf)):
        assert nr.cell_of(7, 5, **g, x=x, y=y) is None
    d = np.array([[0, 10, 14], [1999, 2000, nr.UNREACHED]], dtype=np.uint32)
    v = nr.field(d, 0.05, 10.0)
    assert v.dtype == np.float32 and np.array_equal(v, np.array([[0.0, 0.05, 14 * 0.05 / 10.0], [1999 * 0.05 / 10.0, 10.0, 10.0]], dtype=np.float32))


# ---- scenario U ---------------------------------------------------------------------------------------------------------------
def _restated_controller(prm, field):
    T = nr.mppi_steps(prm["horizon"], prm["dt"])
    state = dict(u=np.zeros((2, T)))

    def tick(x, noise):
        r = fr.mppi_new_controls_field(prm, state["u"], (0.0, 0.0), nr.U_WAYPOINT, x, noise, field=field)
        state["u"] = r["u"]
        return r["out"]
    return tick


def test_scenario_u_course():
    cost, dist = nr.scenario_u_cost(), nr.scenario_u_distance()
    assert cost.shape == (80, 80) and cost[nr.U_GOAL_CELL] == 1 and cost[nr.cell_of(**nr.U_GRID, x=0.0, y=0.0)] == 1
    X, Y = nr.cell_centres(**nr.U_GRID)
    assert (X[nr.U_GOAL_CELL], Y[nr.U_GOAL_CELL]) == pytest.approx(nr.U_WAYPOINT[:2], abs=1e-12)
    assert np.array_equal(cost == 0, dist <= nr.U_R_ROBOT) and int(cost.max()) == 9
    d = nr.cost_to_go(cost, nr.U_GOAL_CELL)
    start = nr.cell_of(**nr.U_GRID, x=0.0, y=0.0)
    straight = 10 * (nr.U_GOAL_CELL[0] - start[0])
    assert d[start] != nr.UNREACHED and d[start] > 1.3 * straight          # the way round the cup is a real detour
    inside = nr.cell_of(**nr.U_GRID, x=0.7, y=0.0)
    assert d[inside] > d[start]                                             # the pocket is uphill: the field pulls out of it


def test_scenario_u_with_the_goal_field_the_robot_goes_round_the_cup():
    ticks, least, x = nr.scenario_u_run(_restated_controller(nr.U_PRM, nr.scenario_u_goal_field()), seed=3)
    print("scenario U with the goal field: ticks", ticks, "least distance to the walls", least, "end", x)
    assert ticks is not None and ticks <= nr.U_MAX_TICKS and least >= nr.U_R_ROBOT


def test_scenario_u_with_the_inflation_field_the_robot_stays_in_the_cup():
    ticks, least, x = nr.scenario_u_run(_restated_controller(nr.U_PRM_INFLATION, nr.scenario_u_inflation_field()), seed=3, prm=nr.U_PRM_INFLATION)
    print("scenario U with scenario S's inflation field: ticks", ticks, "least distance to the walls", least, "end", x)
    assert ticks is None and x[0] < 0.9
