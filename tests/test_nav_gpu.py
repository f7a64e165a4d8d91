"""GPU tests of the goal field (include/tbnav_nav.h, csrc/nav.hip) against its restatement (tests/nav_restatement.py) over the
case table (tests/nav_cases.py): the cost-to-go, the field's float bits and the paths with ==, the solver's structure, the
rejections, the hand-over to the MPPI handle bit for bit against tbnav_mppi_set_cost_field, and scenario U through the library."""
import ctypes as C

import numpy as np
import pytest

import nav_cases as nc
import nav_restatement as nr
from cases import WAYPOINTS, make_mppi, mppi_cfg

pytestmark = pytest.mark.gpu

CAPS = (10.0, 0.73)      # scenario U's, and one that caps most cells of most grids


def _nav(gpu_pkg, cost, geom=None):
    from rtn_amd.nav import GoalField
    g = dict(nc.GEOM if geom is None else geom)
    nav = GoalField(cost.shape[0], cost.shape[1], g["xmin"], g["ymin"], g["resolution"])
    nav.setCost(cost)
    return nav


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_solution(gpu_pkg, nav, cost, goal, starts, refusing):
    """d, the field's bits for both caps, every walk and the refusal, all with ==."""
    want = nc.expected_for(cost, goal)
    got = nav.costToGo()
    assert got.dtype == np.uint32 and np.array_equal(got, want), int((got != want).sum())
    for cap in CAPS:
        assert np.array_equal(_bits(nav.field(cap)), _bits(nr.field(want, nav.resolution, cap))), cap
    for s in starts:
        p, _ = nr.path(cost, want, s)
        assert np.array_equal(nav.path(*s), p), s
    if refusing is not None:
        with pytest.raises(gpu_pkg.capi.TbnavError) as ei:
            nav.path(*refusing)
        assert ei.value.status == gpu_pkg.capi.ERR_UNSUPPORTED


# ---- 1: every case -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nc.NAMES)
def test_case_equals_the_restatement(gpu_pkg, name):
    case = nc.CASES[name]
    nav = _nav(gpu_pkg, case["cost"])
    nav.solve(*case["goal"])
    info = nav.lastSolve()
    print(name, case["cost"].shape, "goal", case["goal"], info)
    assert info["kernel"] == "nav_relax_tiles" and info["solved"] and info["goal"] == case["goal"]
    assert info["tiles"] == (-(-case["cost"].shape[0] // 32), -(-case["cost"].shape[1] // 32))
    assert 1 <= info["rounds"] <= info["launches"] and info["tile_visits"] >= info["rounds"] - 1
    _check_solution(gpu_pkg, nav, case["cost"], case["goal"], nc.starts(name), nc.refusing_start(name))
    nav.close()


# ---- 2: the solver's structure ---------------------------------------------------------------------------------------------------
def test_rounds_in_open_space_follow_the_tiles_not_the_cells(gpu_pkg):
    """In open space the front crosses at least one tile per round, so rounds <= 4 * (tiles_x + tiles_y) (the factor 4 is slack for
    the argument, not a measurement); a per-cell sweep needs 399 rounds from that corner."""
    case = nc.CASES["empty_400"]
    nav = _nav(gpu_pkg, case["cost"])
    assert nav.lastSolve()["kernel"] == "" and not nav.lastSolve()["solved"]
    nav.solve(*case["goal"])
    info = nav.lastSolve()
    tx, ty = info["tiles"]
    print("empty 400 x 400 from (0, 0): rounds", info["rounds"], "launches", info["launches"], "tile visits", info["tile_visits"], "bound", 4 * (tx + ty))
    assert (tx, ty) == (13, 13) and info["rounds"] <= 4 * (tx + ty)
    assert info["tile_visits"] >= tx * ty       # every tile was reached
    nav.close()


def test_the_serpentine_takes_rounds_far_beyond_its_tiles_per_side(gpu_pkg):
    """A path that crosses tile borders hundreds of times: the rounds are counted in border crossings, and a tile that runs into
    its sweep bound stays active (== with the restatement is asserted by the case test above)."""
    case = nc.CASES["serpentine_96"]
    nav = _nav(gpu_pkg, case["cost"])
    nav.solve(*case["goal"])
    info = nav.lastSolve()
    print("serpentine 96 x 96: rounds", info["rounds"], "launches", info["launches"], "tile visits", info["tile_visits"])
    assert info["tiles"] == (3, 3) and info["rounds"] > 3 * 3
    assert int(nav.costToGo()[94, 0]) == nc.SERPENTINE_LONGEST
    nav.close()


def test_a_serpentine_inside_one_tile_runs_into_the_sweep_bound_and_wakes_itself(gpu_pkg):
    """One tile, 16 x 31 corridor moves: a row's 32 cells are lanes of one wave that sweep in lockstep, so a sweep advances a front one
    cell along a corridor, and three visits of 128 sweeps cannot do them; a last round must change nothing.  So rounds >= 5, and
    each of the first three visits at least ends at the sweep bound, where the tile wakes itself — nobody else could (== with the
    restatement is asserted by the case test)."""
    case = nc.CASES["serpentine_in_tile_32"]
    nav = _nav(gpu_pkg, case["cost"])
    nav.solve(*case["goal"])
    info = nav.lastSolve()
    print("serpentine in one tile: rounds", info["rounds"], "launches", info["launches"], "tile visits", info["tile_visits"])
    assert info["tiles"] == (1, 1) and info["rounds"] >= 5
    assert info["tile_visits"] >= info["rounds"] - 1
    assert int(nav.costToGo()[30, 0]) == nc.SERPENTINE_IN_TILE_LONGEST
    nav.close()


def test_two_solves_and_a_set_cost_in_a_row_equal_fresh_handles(gpu_pkg):
    """Solving again resets what the last solve left: another goal, then a changed cost grid, each against a fresh handle and the
    restatement; set_cost alone leaves the last solution in place."""
    nav = _nav(gpu_pkg, nc.SEQUENCE[0][0])
    cost = nc.SEQUENCE[0][0]
    for new_cost, goal in nc.SEQUENCE:
        if new_cost is not None:
            before = None if not nav.lastSolve()["solved"] else (nav.costToGo(), nav.field(CAPS[0]), nav.path(*nav.lastSolve()["goal"]))
            nav.setCost(new_cost)
            if before is not None:      # the solution of the old grid stays until the next solve
                assert np.array_equal(nav.costToGo(), before[0]) and np.array_equal(_bits(nav.field(CAPS[0])), _bits(before[1]))
                assert np.array_equal(nav.path(*nav.lastSolve()["goal"]), before[2])
            cost = new_cost
        nav.solve(*goal)
        fresh = _nav(gpu_pkg, cost)
        fresh.solve(*goal)
        assert np.array_equal(nav.costToGo(), fresh.costToGo()) and nav.lastSolve()["goal"] == goal
        want = nc.expected_for(cost, goal)
        reached = np.argwhere(want != nr.UNREACHED)
        _check_solution(gpu_pkg, nav, cost, goal, [tuple(int(v) for v in reached[0]), tuple(int(v) for v in reached[-1])], None)
        fresh.close()
    nav.close()


# ---- 3: G1 and the rejections ------------------------------------------------------------------------------------------------------
def test_cell_of_on_the_library(gpu_pkg):
    c = gpu_pkg.capi
    nav = _nav(gpu_pkg, nc.CASES["drawn_7x5"]["cost"])
    g = nc.GEOM
    rng = np.random.default_rng(1)
    pts = [(-1.0, -2.0), (-0.6501, -1.7501), (-0.65, -2.0), (-1.0, -1.75), (-1.0001, -2.0), (-1.0, -2.0001), (np.nan, -2.0), (-1.0, np.inf), (-np.inf, 0.0),
           (1e300, -1.9)] + [tuple(v) for v in rng.uniform((-1.1, -2.1), (-0.6, -1.7), (200, 2))]
    for x, y in pts:
        want = nr.cell_of(7, 5, **g, x=x, y=y)
        if want is None:
            with pytest.raises(c.TbnavError) as ei:
                nav.cellOf(x, y)
            assert ei.value.status == c.ERR_OUT_OF_WORLD, (x, y)
        else:
            assert nav.cellOf(x, y) == want, (x, y)
    nav.close()


def test_rejections_leave_the_last_solution_in_place(gpu_pkg):
    c = gpu_pkg.capi
    L = c.lib()
    from rtn_amd.nav import GoalField
    # G1: before any device call
    for kw in (dict(nx=1), dict(ny=1), dict(nx=2049), dict(ny=2049), dict(resolution=0.0), dict(resolution=-0.05), dict(resolution=np.nan),
               dict(resolution=np.inf), dict(xmin=np.nan), dict(ymin=-np.inf)):
        p = dict(nx=7, ny=5, **nc.GEOM); p.update(kw)
        with pytest.raises(c.TbnavError) as ei:
            GoalField(p["nx"], p["ny"], p["xmin"], p["ymin"], p["resolution"])
        assert ei.value.status == c.ERR_INVALID_ARG, kw
    case = nc.CASES["diagonal_wall_closed"]
    cost, goal = case["cost"], case["goal"]
    nav = GoalField(40, 40, **nc.GEOM)
    h = nav._h
    d_buf, f_buf, n = np.zeros((40, 40), np.uint32), np.zeros((40, 40), np.float32), C.c_int32(-7)
    # nothing set, nothing solved
    assert L.tbnav_nav_solve(h, *goal) == c.ERR_INVALID_ARG
    nav.setCost(cost)
    assert L.tbnav_nav_get_cost_to_go(h, d_buf.ctypes.data) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_get_field(h, 10.0, f_buf.ctypes.data) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_path(h, 0, 0, None, 0, C.byref(n)) == c.ERR_INVALID_ARG and n.value == -7
    m = make_mppi(gpu_pkg, mppi_cfg(65, 0.1))
    assert L.tbnav_nav_apply_to_mppi(h, m._h, 10.0, 1.0) == c.ERR_INVALID_ARG and m.costField() is None
    nav.solve(*goal)

    def state():
        return nav.costToGo(), _bits(nav.field(10.0)), nav.path(0, 0), nav.lastSolve()

    def same(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]

    before = state()
    assert np.array_equal(before[0], nc.expected("diagonal_wall_closed"))
    # G2: a cost above 64 — and the grid in force stays: the same goal solves to the same answer afterwards
    bad = cost.copy(); bad[3, 4] = 65
    assert L.tbnav_nav_set_cost(h, bad.ctypes.data) == c.ERR_INVALID_ARG and L.tbnav_nav_set_cost(h, None) == c.ERR_INVALID_ARG
    assert same(state(), before)
    # G4: a goal that is blocked or outside
    for g in ((31, 32), (-1, 0), (0, -1), (40, 0), (0, 40)):
        assert L.tbnav_nav_solve(h, *g) == c.ERR_INVALID_ARG, g
        assert same(state(), before)
    # G5
    for cap in (0.0, -1.0, np.nan, np.inf):
        assert L.tbnav_nav_get_field(h, cap, f_buf.ctypes.data) == c.ERR_INVALID_ARG
        assert L.tbnav_nav_apply_to_mppi(h, m._h, cap, 1.0) == c.ERR_INVALID_ARG and m.costField() is None
    assert L.tbnav_nav_get_field(h, 10.0, None) == c.ERR_INVALID_ARG and L.tbnav_nav_get_cost_to_go(h, None) == c.ERR_INVALID_ARG
    for weight in (np.nan, np.inf):
        assert L.tbnav_nav_apply_to_mppi(h, m._h, 10.0, weight) == c.ERR_INVALID_ARG and m.costField() is None
    assert L.tbnav_nav_apply_to_mppi(h, None, 10.0, 1.0) == c.ERR_INVALID_ARG and L.tbnav_nav_apply_to_mppi_group(h, None, 10.0, 1.0) == c.ERR_INVALID_ARG
    # G6: outside, blocked, unreached, a buffer too small
    cells = np.full((64, 2), -1, np.int32)
    for s in ((-1, 0), (40, 39), (0, 40)):
        assert L.tbnav_nav_path(h, *s, cells.ctypes.data, 64, C.byref(n)) == c.ERR_INVALID_ARG and n.value == -7
    for s in ((31, 32), (39, 39)):
        assert L.tbnav_nav_path(h, *s, cells.ctypes.data, 64, C.byref(n)) == c.ERR_UNSUPPORTED and n.value == -7
    assert L.tbnav_nav_path(h, 0, 0, cells.ctypes.data, 5, C.byref(n)) == c.ERR_INVALID_ARG and n.value == len(before[2]) == 21
    assert np.array_equal(cells[:5], before[2][:5]) and (cells[5:] == -1).all()
    assert L.tbnav_nav_path(h, 0, 0, cells.ctypes.data, 21, C.byref(n)) == c.OK and np.array_equal(cells[:21], before[2])
    assert same(state(), before)
    nav.solve(*goal)
    assert np.array_equal(nav.costToGo(), before[0])
    m.close(); nav.close()


# ---- 4: the hand-over ----------------------------------------------------------------------------------------------------------------
# tests/test_mppi_field_gpu.py's parity setting: rollouts from X0 with the warm start UINIT start beside a 7 x 5 field of 0.05 m cells
# from (0.4, 0.1), cross it and leave it
X0, UINIT, XD = (0.5, 0.2, 1.0), (5.0, 6.0), WAYPOINTS[2]
FIELD_GEOM = dict(xmin=0.4, ymin=0.1, resolution=0.05)
CAP, WEIGHT = 10.0, 1e4


def _solved_7x5(gpu_pkg):
    case = nc.CASES["drawn_7x5"]
    nav = _nav(gpu_pkg, case["cost"], FIELD_GEOM)
    nav.solve(*case["goal"])
    return nav


def _controller(gpu_pkg, K):
    m = make_mppi(gpu_pkg, mppi_cfg(K, 0.5))
    m.setWaypoint(*XD)
    m.setInitialControls(*UINIT)
    return m


def _noise(seed, K, T):
    return np.random.default_rng(seed).normal(0.0, np.sqrt(0.9), (K, T, 2))


@pytest.mark.parametrize("K", [65, 256])
def test_apply_to_mppi_equals_set_cost_field_of_get_field(gpu_pkg, K):
    """Three ticks with the warm start carried: J, the returned controls and u, bit for bit."""
    nav = _solved_7x5(gpu_pkg)
    a, b, plain = (_controller(gpu_pkg, K) for _ in range(3))
    nav.applyTo(a, CAP, WEIGHT)
    values = nav.field(CAP)
    b.setCostField(values, FIELD_GEOM["xmin"], FIELD_GEOM["ymin"], FIELD_GEOM["resolution"], WEIGHT)
    assert a.costField() == b.costField() == dict(nx=7, ny=5, weight=WEIGHT, **FIELD_GEOM)
    centres = np.stack([v.ravel() for v in nr.cell_centres(7, 5, **FIELD_GEOM)], axis=1)
    assert np.array_equal(a.costFieldLookup(centres), b.costFieldLookup(centres))     # the same values on the device
    x0 = X0
    for tick in range(3):
        nz = _noise(100 * K + tick, K, a.steps)
        ga, gb = a.newControls(*x0, nz), b.newControls(*x0, nz)
        assert ga == gb and a.lastKernelNames() == b.lastKernelNames() and a.lastKernelNames()[0] == "mppi_rollout_field<1>"
        assert np.array_equal(a.costToGo(), b.costToGo()) and np.array_equal(a.getControls(), b.getControls())
        if tick == 0:
            plain.newControls(*x0, nz)
            assert (a.costToGo() > plain.costToGo()).all()      # (the field takes part in the tick: metres to go times the weight)
        x0 = (x0[0] + 0.002, x0[1] - 0.001, x0[2] + 0.003)
    # a second hand-over replaces the first: another cap and weight, again bit for bit
    nav.applyTo(a, CAPS[1], 3.0)
    b.setCostField(nav.field(CAPS[1]), FIELD_GEOM["xmin"], FIELD_GEOM["ymin"], FIELD_GEOM["resolution"], 3.0)
    nz = _noise(7, K, a.steps)
    assert a.newControls(*x0, nz) == b.newControls(*x0, nz) and np.array_equal(a.costToGo(), b.costToGo())
    for m in (a, b, plain):
        m.close()
    nav.close()


def test_apply_to_a_group_of_two_members_on_one_device(gpu_pkg):
    from rtn_amd.mppi import CartModel, LossFunc, MPPIGroup
    K = 256
    d = mppi_cfg(K, 0.5)
    nav = _solved_7x5(gpu_pkg)

    def group():
        g = MPPIGroup(CartModel(d["wheel_radius"], d["wheel_base"]), LossFunc(d["Q"], d["R"], d["P1"]), d["lam"], d["max_wheel_vel"], d["ul_var"],
                      d["ur_var"], 0.5, d["dt"], K, devices=[0, 0])
        g.setWaypoint(*XD); g.setInitialControls(*UINIT)
        return g
    a, b = group(), group()
    with pytest.raises(gpu_pkg.capi.TbnavError):
        nav.applyTo(a, np.nan, WEIGHT)
    assert all(a.member(r).costField() is None for r in range(2))        # every member or none
    nav.applyTo(a, CAP, WEIGHT)
    b.setCostField(nav.field(CAP), FIELD_GEOM["xmin"], FIELD_GEOM["ymin"], FIELD_GEOM["resolution"], WEIGHT)
    assert all(a.member(r).costField() == b.member(r).costField() == dict(nx=7, ny=5, weight=WEIGHT, **FIELD_GEOM) for r in range(2))
    x0 = X0
    for tick in range(3):
        nz = _noise(900 + tick, K, 50)
        assert a.newControls(*x0, nz) == b.newControls(*x0, nz)
        assert np.array_equal(a.getControls(), b.getControls())
        for r in range(2):
            assert a.member(r).lastKernelNames()[0] == "mppi_rollout_field<1>"
            assert np.array_equal(a.member(r).costToGo(), b.member(r).costToGo())
        x0 = (x0[0] + 0.002, x0[1] - 0.001, x0[2] + 0.003)
    a.close(); b.close(); nav.close()


def test_a_handle_whose_applied_field_is_cleared_is_a_handle_that_never_had_one(gpu_pkg):
    K = 256
    nav = _solved_7x5(gpu_pkg)
    a, b = _controller(gpu_pkg, K), _controller(gpu_pkg, K)
    T = a.steps
    nz = _noise(5, K, T)
    nav.applyTo(b, CAP, WEIGHT)
    b.newControls(*X0, nz)
    assert b.lastKernelNames()[0] == "mppi_rollout_field<1>"
    J_with_field = b.costToGo()
    warm = np.zeros((2, T)); warm[0], warm[1] = UINIT
    b.setControls(warm)
    b.clearCostField()
    assert a.costField() is None and b.costField() is None
    ga, gb = a.newControls(*X0, nz), b.newControls(*X0, nz)
    assert ga == gb and (J_with_field > a.costToGo()).all()
    assert np.array_equal(a.costToGo(), b.costToGo()) and np.array_equal(a.getControls(), b.getControls())
    assert a.lastKernelNames() == b.lastKernelNames() and not a.lastKernelNames()[0].startswith("mppi_rollout_field")
    a.close(); b.close(); nav.close()


# ---- 5: scenario U on the device ------------------------------------------------------------------------------------------------------
def test_scenario_u_on_the_device_with_the_goal_field(gpu_pkg):
    """The course of tests/nav_restatement.py through the library: cost grid from rtn_amd.nav.nav_cost_from_distance, solved on the
    device, handed over with apply_to_mppi; host noise of seed 3 through newControls.  The closed loop does not follow the
    restatement's tick for tick (a closed loop amplifies 1e-16); the conditions are the restatement's: arrival within 0.05 m in at
    most 1500 ticks and a least distance to the walls >= r_robot = 0.10 m."""
    from rtn_amd.nav import GoalField, nav_cost_from_distance
    cost = nav_cost_from_distance(nr.scenario_u_distance(), nr.U_R_ROBOT, nr.U_R_INFLATE, nr.U_K)
    assert np.array_equal(cost, nr.scenario_u_cost())
    nav = GoalField(**nr.U_GRID)
    nav.setCost(cost)
    assert nav.cellOf(*nr.U_WAYPOINT[:2]) == nr.U_GOAL_CELL
    nav.solveAt(*nr.U_WAYPOINT[:2])
    assert np.array_equal(_bits(nav.field(nr.U_CAP)), _bits(nr.scenario_u_goal_field()["values"]))
    m = make_mppi(gpu_pkg, nr.U_PRM)
    m.setWaypoint(*nr.U_WAYPOINT)
    m.setInitialControls(0.0, 0.0)
    nav.applyTo(m, nr.U_CAP, nr.U_WEIGHT)
    ticks, least, x = nr.scenario_u_run(lambda x, noise: m.newControls(x[0], x[1], x[2], noise), seed=3)
    print("scenario U on the device, goal field: ticks", ticks, "least distance to the walls", least, "end", x, nav.lastSolve())
    assert m.lastKernelNames()[0] == "mppi_rollout_field<1>"
    assert ticks is not None and ticks <= nr.U_MAX_TICKS and least >= nr.U_R_ROBOT
    m.close(); nav.close()


def test_scenario_u_on_the_device_with_the_inflation_field(gpu_pkg):
    """The same controller with scenario S's inflation field (weight 2e4, Q = [1e4, 1e4, 1]) has not arrived after 1500 ticks and
    ends inside the cup, x < 0.9."""
    f = nr.scenario_u_inflation_field()
    m = make_mppi(gpu_pkg, nr.U_PRM_INFLATION)
    m.setWaypoint(*nr.U_WAYPOINT)
    m.setInitialControls(0.0, 0.0)
    m.setCostField(f["values"], f["xmin"], f["ymin"], f["resolution"], f["weight"])
    ticks, least, x = nr.scenario_u_run(lambda x, noise: m.newControls(x[0], x[1], x[2], noise), seed=3, prm=nr.U_PRM_INFLATION)
    print("scenario U on the device, inflation field: ticks", ticks, "least distance to the walls", least, "end", x)
    assert ticks is None and x[0] < 0.9
    m.close()
