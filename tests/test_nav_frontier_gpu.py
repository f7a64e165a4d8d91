"""GPU tests of the exploration frontiers (include/tbnav_nav.h G10-G16, csrc/nav_frontier.hip) against their restatement
(tests/nav_frontier_restatement.py), all with ==: the case table (tests/nav_frontier_cases.py) through setLogOdds with the classes read
back from the filter's own export, then the tile tables, the best particle, a map drawn by scans, the rejections, the one-goal solve,
the hand-over to MPPI, and the exploration loop against the CPU leg's."""
import ctypes as C

import numpy as np
import pytest

import nav_frontier_cases as cs
import nav_frontier_check as ck
import nav_frontier_restatement as ff
import nav_from_map_restatement as fr
import nav_restatement as nr
import oracle_api as orc
import rbpf_cases as rc
from cases import WAYPOINTS, make_mppi, mppi_cfg

pytestmark = pytest.mark.gpu


def _filter(gpu_pkg, size, N, **kw):
    from rtn_amd.rbpf import ParticleFilter, default_params
    pf = ParticleFilter(default_params(N=N, k=2, map_min=-size.half, map_max=size.half, resolution=size.res), **kw)
    assert (pf.xsize, pf.ysize) == (size.xsize, size.xsize)
    return pf


def _scan(pose):
    """A scan of the small room with a sector of beams that do not return (the scanner gates them out): the map ends there."""
    scan = orc.room_scan(pose, walls=rc.ROOM_SMALL, noise_sigma=0.0)
    scan[100:200] = 4.0
    return scan


def _nav(size):
    from rtn_amd.nav import GoalField
    return GoalField(size.xsize, size.xsize, -size.half, -size.half, size.res)


# ---- 1: the case table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size_id", [s.id for s in cs.SIZES])
def test_every_case_equals_the_restatement(gpu_pkg, size_id):
    """Every case in a slot of its own that nobody has written before (an all-zero tile then stays the shared tile, id 0): the export
    equals the named classes, labels / list / counts / seeds / cost-to-go / field / path equal the restatement, the kernels are the four
    named, and the serpentine takes more than one round."""
    size = cs.SIZE[size_id]
    table = cs.cases(size)
    pf, nav = _filter(gpu_pkg, size, N=len(table) + 1), _nav(size)
    assert nav.lastFrontierKernels() == [] and not nav.lastFrontiers()["found"]
    for slot, (name, case) in enumerate(table.items()):
        pf.setLogOdds(slot, case.lo.reshape(-1))
        assert np.array_equal(pf.particleMap(slot), ff.export_map(case.lo)), name
        mask = ck.install(nav, case.cost, case.discs)
        info, front, lab, seed = ck.check_find(nav, pf, slot, case.cost, mask, case.min_cells, (size_id, name))
        if name == "serpentine":
            assert info["rounds"] > 1 and info["tile_visits"] >= info["rounds"] - 1
        if name in ("half_row31", "half_col31"):
            assert info["cells"] == size.xsize       # the unknown neighbours are all in tiles with id 0
        ck.check_solves(nav, case.cost, seed, size.res, (size_id, name))
    # the last slot was never written: unknown throughout
    info, front, _, _ = ck.check_find(nav, pf, len(table), table["all_free"].cost, ck.install(nav, table["all_free"].cost, ()), 1, "fresh")
    assert info["cells"] == 0 and info["rounds"] == 1
    nav.close(); pf.close()


# ---- 2: the tile table -----------------------------------------------------------------------------------------------------------------
def test_slots_that_share_tiles_and_then_diverge_each_give_their_own_frontiers(gpu_pkg):
    size = cs.SIZE["s96"]
    pf, nav = _filter(gpu_pkg, size, N=3), _nav(size)
    case = cs.cases(size)["two_runs"]
    pf.setLogOdds(0, case.lo.reshape(-1))
    pf.gatherLocal(np.array([-1, 0, -1], dtype=np.int32))
    pf.copyParticle(2, pf, 0)
    mask = ck.install(nav, case.cost, ())
    labs = [ck.check_find(nav, pf, p, case.cost, mask, cs.MIN_CELLS, ("shared", p))[2] for p in range(3)]
    assert np.array_equal(labs[0], labs[1]) and np.array_equal(labs[0], labs[2])
    pose = (0.3, 0.1, -0.2)
    pf.integrateScan(1, _scan(pose), pose)
    after = [ck.check_find(nav, pf, p, case.cost, mask, cs.MIN_CELLS, ("diverged", p)) for p in range(3)]
    assert np.array_equal(after[0][2], labs[0]) and np.array_equal(after[2][2], labs[0])
    assert after[1][0]["cells"] > 50 and not np.array_equal(after[1][2], labs[0])      # the scan's frontiers are in slot 1 alone
    seed1 = ck.check_find(nav, pf, 1, case.cost, mask, cs.MIN_CELLS, ("diverged", 1, "again"))[3]      # (the last find above was slot 2's)
    assert np.array_equal(seed1, after[1][3])
    ck.check_solves(nav, case.cost, seed1, size.res, "diverged")
    nav.close(); pf.close()


# ---- 3: the best particle --------------------------------------------------------------------------------------------------------------
def test_best_particle_is_the_arg_max_of_the_weights_and_the_first_of_a_tie(gpu_pkg):
    size = cs.SIZE["s64"]
    pf, nav = _filter(gpu_pkg, size, N=4), _nav(size)
    cost = cs.base_cost(64)
    mask = ck.install(nav, cost, ())
    for p in range(4):
        lo = np.zeros((64, 64))
        lo[10 + 10 * p, 5:20 + p] = cs.F
        pf.setLogOdds(p, lo.reshape(-1))
    for w, best in (([0.1, 0.4, 0.4, 0.1], 1), ([0.1, 0.2, 0.3, 0.4], 3), ([0.25, 0.25, 0.25, 0.25], 0), ([0.1, 0.2, 0.5, 0.2], 2)):
        pf.setParticles(w=np.array(w))
        info, front, _, seed = ck.check_find(nav, pf, best, cost, mask, cs.MIN_CELLS, ("best", w), particle=None)
        assert front[10 + 10 * best, 5:20 + best].all() and info["cells"] == 15 + best and pf.getRobotState()[1] == best
    nav.close(); pf.close()


# ---- 4: a map drawn by scans -----------------------------------------------------------------------------------------------------------
def test_a_map_drawn_by_real_scans(gpu_pkg):
    size = cs.SIZE["s80"]
    pf, nav = _filter(gpu_pkg, size, N=1), _nav(size)
    for pose in ((0.0, 0.0, 0.0), (0.07, 0.10, 0.05), (0.14, 0.20, 0.10)):
        pf.integrateScan(0, _scan(pose), pose)
    nav.setCostFrom(pf, 0.10, 0.45, 8.0, particle=0)
    cost = nav.cost()
    nav.markVisited(40, 60, 6)
    mask = ff.disc(80, 80, 40, 60, 6)
    for min_cells in (1, 8):
        info, front, lab, seed = ck.check_find(nav, pf, 0, cost, mask, min_cells, ("scans", min_cells))
        assert info["cells"] > 20 and seed.any()
        ck.check_solves(nav, cost, seed, size.res, ("scans", min_cells))
    nav.close(); pf.close()


# ---- 5: rejections ----------------------------------------------------------------------------------------------------------------------
def test_rejections_change_nothing(gpu_pkg):
    from rtn_amd.nav import GoalField
    c = gpu_pkg.capi
    L = c.lib()
    size = cs.SIZE["s64"]
    case = cs.cases(size)["two_runs"]
    pf, nav = _filter(gpu_pkg, size, N=2), _nav(size)
    pf.setLogOdds(0, case.lo.reshape(-1))
    info = c.NavFrontierInfo()
    buf32 = np.zeros((64, 64), dtype=np.uint32)
    n = C.c_int32(-5)
    # before a cost grid, before a find
    assert L.tbnav_nav_find_frontiers(nav._h, pf._h, 0, 8, C.byref(info)) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_solve_frontiers(nav._h) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_get_frontier_labels(nav._h, buf32.ctypes.data) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_frontier_list(nav._h, None, 0, C.byref(n)) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_solve_goals(nav._h, np.array([[3, 3]], dtype=np.int32).ctypes.data, 1) == c.ERR_INVALID_ARG
    mask = ck.install(nav, case.cost, ())
    _, front, lab, seed = ck.check_find(nav, pf, 0, case.cost, mask, 8, "first")
    nav.solve(40, 40)
    d0, info0 = nav.costToGo(), nav.lastSolve()

    def unchanged():
        return (np.array_equal(nav.frontierLabels(), lab) and np.array_equal(nav.costToGo(), d0) and nav.lastSolve() == info0 and
                np.array_equal(nav.visited(), mask.astype(np.uint8)))

    for particle, min_cells in ((0, 0), (0, -3), (2, 8), (-2, 8), (1 << 20, 8)):
        assert L.tbnav_nav_find_frontiers(nav._h, pf._h, particle, min_cells, C.byref(info)) == c.ERR_INVALID_ARG and unchanged()
    assert L.tbnav_nav_find_frontiers(nav._h, None, 0, 8, C.byref(info)) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_find_frontiers(None, pf._h, 0, 8, C.byref(info)) == c.ERR_INVALID_ARG and unchanged()
    for ix, iy, r in ((-1, 3, 2), (3, 64, 2), (64, 0, 0), (3, 3, -1), (3, 3, 65)):
        assert L.tbnav_nav_mark_visited(nav._h, ix, iy, r) == c.ERR_INVALID_ARG and unchanged()
    for cells in ([[3, 3], [64, 3]], [[3, 3], [3, -1]]):
        a = np.array(cells, dtype=np.int32)
        assert L.tbnav_nav_solve_goals(nav._h, a.ctypes.data, 2) == c.ERR_INVALID_ARG and unchanged()
    assert L.tbnav_nav_solve_goals(nav._h, np.array([[3, 3]], dtype=np.int32).ctypes.data, 0) == c.ERR_INVALID_ARG and unchanged()
    assert L.tbnav_nav_solve_goals(nav._h, None, 1) == c.ERR_INVALID_ARG
    # a buffer too small for the list: the number needed
    assert L.tbnav_nav_frontier_list(nav._h, (c.NavFrontier * 1)(), 1, C.byref(n)) == c.ERR_INVALID_ARG and n.value == 2
    # a grid that is not the filter's
    for kw in (dict(nx=96, ny=96), dict(nx=64, ny=62), dict(xmin=-1.6 + 1e-9), dict(resolution=0.0500001)):
        g = dict(nx=64, ny=64, xmin=-1.6, ymin=-1.6, resolution=0.05)
        g.update(kw)
        other = GoalField(**g)
        other.setCost(np.ones((g["nx"], g["ny"]), dtype=np.uint8))
        assert L.tbnav_nav_find_frontiers(other._h, pf._h, 0, 8, C.byref(info)) == c.ERR_INVALID_ARG, kw
        assert not other.lastFrontiers()["found"] and other.lastFrontierKernels() == []
        other.close()
    # a blocked goal among the listed: the last solution stays
    blocked = case.cost.copy()
    blocked[30, 30] = 0
    nav.setCost(blocked)
    assert L.tbnav_nav_solve_goals(nav._h, np.array([[3, 3], [30, 30]], dtype=np.int32).ctypes.data, 2) == c.ERR_INVALID_ARG and unchanged()
    # the grid was set again since the find: its seeds are no goals any more, until the next find
    assert L.tbnav_nav_solve_frontiers(nav._h) == c.ERR_INVALID_ARG and unchanged()
    nav.findFrontiers(pf, 8, particle=0)
    nav.markVisited(0, 0, 0)
    assert L.tbnav_nav_solve_frontiers(nav._h) == c.ERR_INVALID_ARG
    nav.findFrontiers(pf, 8, particle=0)
    nav.clearVisited()
    mask[:] = False
    assert L.tbnav_nav_solve_frontiers(nav._h) == c.ERR_INVALID_ARG and unchanged()
    # no seed: UNSUPPORTED, and the last solution survives
    info20 = nav.findFrontiers(pf, 20, particle=0)
    assert info20["cells"] == 20 and info20["seed_cells"] == 0 and info20["seed_clusters"] == 0
    assert L.tbnav_nav_solve_frontiers(nav._h) == c.ERR_UNSUPPORTED and nav.solveFrontiers() is False
    assert np.array_equal(nav.costToGo(), d0) and nav.lastSolve() == info0
    # and the accepted calls still work afterwards
    nav.findFrontiers(pf, 8, particle=0)
    assert nav.solveFrontiers() is True and np.array_equal(nav.costToGo() == 0, seed)
    nav.close(); pf.close()


# ---- 6: one goal ------------------------------------------------------------------------------------------------------------------------
def test_solve_goals_with_one_goal_equals_solve_bit_for_bit(gpu_pkg):
    size = cs.SIZE["s96"]
    nav = _nav(size)
    rng = np.random.default_rng(5)
    cost = cs.base_cost(96)
    cost[rng.random((96, 96)) < 0.2] = 0
    cost[31:34, 60:66] = 3
    nav.setCost(cost)
    for goal in ((32, 63), (0, 0) if cost[0, 0] else (31, 60), (33, 65)):
        nav.solve(*goal)
        d, info, f = nav.costToGo(), nav.lastSolve(), nav.field(5.0)
        nav.solve(*(31, 61))       # something else in between
        nav.solveGoals([goal])
        assert np.array_equal(nav.costToGo(), d) and nav.lastSolve() == info and np.array_equal(ck.bits(nav.field(5.0)), ck.bits(f))
        assert np.array_equal(d, nr.cost_to_go(cost, goal))
        nav.solveGoals([goal, goal, goal])      # a cell listed twice is harmless
        assert np.array_equal(nav.costToGo(), d)
    nav.close()


# ---- 7: the hand-over -------------------------------------------------------------------------------------------------------------------
def test_apply_to_after_solve_frontiers_equals_set_cost_field_of_the_host_array(gpu_pkg):
    size = cs.SIZE["s64"]
    case = cs.cases(size)["min_cells_edge"]
    pf, nav = _filter(gpu_pkg, size, N=1), _nav(size)
    pf.setLogOdds(0, case.lo.reshape(-1))
    ck.install(nav, case.cost, ())
    nav.findFrontiers(pf, case.min_cells, particle=0)
    assert nav.solveFrontiers()
    a, b = (make_mppi(gpu_pkg, mppi_cfg(64, 0.5)) for _ in range(2))
    for m in (a, b):
        m.setWaypoint(*WAYPOINTS[2])
        m.setInitialControls(5.0, 6.0)
    nav.applyTo(a, 3.0, 1e4)
    b.setCostField(nav.field(3.0), -size.half, -size.half, size.res, 1e4)
    centres = np.stack([v.ravel() for v in nr.cell_centres(64, 64, -size.half, -size.half, size.res)], axis=1)
    assert a.costField() == b.costField() and np.array_equal(a.costFieldLookup(centres), b.costFieldLookup(centres))
    nz = np.random.default_rng(40).normal(0.0, np.sqrt(0.9), (64, a.steps, 2))
    assert a.newControls(0.5, 0.2, 1.0, nz) == b.newControls(0.5, 0.2, 1.0, nz) and np.array_equal(a.costToGo(), b.costToGo())
    for h in (a, b, nav, pf):
        h.close()


# ---- 8: the exploration loop ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", cs.EXPLORE_STARTS)
def test_exploration_loop_on_the_device_visits_the_cells_of_the_cpu_loop(gpu_pkg, start):
    """tbnav_rbpf_integrate_scan at the true pose, one particle; setCostFrom, findFrontiers, solveFrontiers, path, markVisited."""
    from rtn_amd.nav import GoalField
    from rtn_amd.rbpf import ParticleFilter, default_params
    import test_nav_frontier_cases as cpu
    m = cs.EXPLORE_MAP
    pf = ParticleFilter(default_params(N=1, k=2, map_min=-m["half"], map_max=m["half"], resolution=m["res"]))
    nav = GoalField(m["xsize"], m["xsize"], -m["half"], -m["half"], m["res"])
    assert pf.xsize == m["xsize"]

    def plan(cell):
        nav.setCostFrom(pf, *cs.EXPLORE_INFLATION, particle=0)
        nav.findFrontiers(pf, cs.MIN_CELLS, particle=0)
        if not nav.solveFrontiers():
            return None
        return nav.path(*cell)

    run = cs.explore(start, lambda scan, pose: pf.integrateScan(0, scan, pose), plan,
                     lambda cell: nav.markVisited(cell[0], cell[1], cs.EXPLORE_MARK_RADIUS))
    want = cpu.explore_cpu_cached(start)
    assert run["cells"] == want["cells"] and run["marks"] == want["marks"] and run["done"] and want["done"]
    assert np.array_equal(pf.particleMap(0), want["exported"])
    nav.close(); pf.close()
