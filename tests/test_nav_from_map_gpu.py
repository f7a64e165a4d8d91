"""GPU tests of the cost grid taken from a filter particle's map on the device (include/tbnav_nav.h G7-G9, csrc/nav_from_map.hip:
nav_cost_from_occ) against its restatement (tests/nav_from_map_restatement.py) and against the host route it replaces
(occDist -> nav_cost_from_distance / cost_field_from_distance -> setCost / setCostField), all with ==, over the case table
(tests/nav_from_map_cases.py); then the tile tables, the best particle, a real scan, the solve after a device-set grid, the
rejections, a filter too large for a stored field, and scenario U from a rasterised map."""
import ctypes as C
import functools

import numpy as np
import pytest

import nav_from_map_cases as fc
import nav_from_map_restatement as fr
import nav_restatement as nr
import oracle_api as orc
import rbpf_cases as rc
from cases import WAYPOINTS, make_mppi, mppi_cfg

pytestmark = pytest.mark.gpu

L_OCC = np.log(0.9 / (1 - 0.9))
KERNEL = "nav_cost_from_occ<uint8_t>"
X0, UINIT, XD = (0.5, 0.2, 1.0), (5.0, 6.0), WAYPOINTS[2]      # tests/test_nav_gpu.py's parity setting: inside every map here
WEIGHT = 1e4


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _filter(gpu_pkg, size, N, **kw):
    from rtn_amd.rbpf import ParticleFilter, default_params
    pf = ParticleFilter(default_params(N=N, k=2, map_min=-size.half, map_max=size.half, resolution=size.res), **kw)
    assert (pf.xsize, pf.ysize) == (size.xsize, size.xsize)
    return pf


def _nav(size):
    from rtn_amd.nav import GoalField
    return GoalField(size.xsize, size.xsize, -size.half, -size.half, size.res)


def _controller(gpu_pkg, K=64):
    m = make_mppi(gpu_pkg, mppi_cfg(K, 0.5))
    m.setWaypoint(*XD)
    m.setInitialControls(*UINIT)
    return m


def _set_occ(pf, p, occ, fresh_field=True):
    """The occupancy into slot p.  fresh_field: the slot's stored distance field is first reset to "nothing within 10 m" (as
    tests/test_edt_gpu.py injects a previous field), because the filter's transform leaves cells farther than its radius from every
    occupied cell as they were — on the 24-cell map of 0.5 m cells (radius 20) the host route would otherwise carry the previous
    pattern's distances into this one's grid.  The device route reads no stored field and has no such history."""
    if fresh_field:
        pf.setOccDist(p, np.full(pf.G, fr.MAX_OCC_DIST))
    pf.setLogOdds(p, occ.reshape(-1).astype(np.float64) * L_OCC)


def _occ_of(pf, p):
    """The particle's occupied cells as the filter sees them (distance 0 to the nearest occupied cell), and the host route's metres."""
    metres = pf.occDist(p).reshape(pf.xsize, pf.xsize)
    return (metres == 0.0).astype(np.uint8), metres


@functools.lru_cache(maxsize=None)
def _c(size_id, name):
    """c(cell) of a pattern over the widest window its size's parameter sets ask for: computed once, shared, never changed."""
    size = fc.SIZE[size_id]
    c = fr.nearest_c(fc.patterns(size)[name], max(fr.reach(size.res, p[1]) for p in fc.params(size).values()))
    c.setflags(write=False)
    return c


# ---- 1: every case, both outputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size_id", [s.id for s in fc.SIZES])
def test_cost_grid_and_mppi_field_equal_the_restatement_and_the_host_route(gpu_pkg, size_id):
    """For every pattern (installed in slot 1 with setLogOdds) and parameter set: nav.cost() after setCostFrom == the restatement ==
    nav_cost_from_distance(pf.occDist(1)); the MPPI field set by setCostFieldFrom reads, at every cell centre, what setCostField of
    the host route's array reads; on the random pattern two such handles then give identical controls over three ticks."""
    from rtn_amd.mppi import cost_field_from_distance
    from rtn_amd.nav import nav_cost_from_distance
    size = fc.SIZE[size_id]
    xs = size.xsize
    pf, nav = _filter(gpu_pkg, size, N=2), _nav(size)
    a, b = _controller(gpu_pkg), _controller(gpu_pkg)
    geom = dict(xmin=-size.half, ymin=-size.half, resolution=size.res)
    centres = np.stack([v.ravel() for v in nr.cell_centres(xs, xs, **geom)], axis=1)
    assert nav.lastCostKernel() == ""
    for name, occ in fc.patterns(size).items():
        _set_occ(pf, 1, occ)
        seen, metres = _occ_of(pf, 1)
        assert np.array_equal(seen, occ), name
        for pname, (r_robot, r_inflate, k) in fc.params(size).items():
            nav.setCostFrom(pf, r_robot, r_inflate, k, particle=1)
            got = nav.cost()
            want = fr.cost_from_occ(occ, size.res, r_robot, r_inflate, k, c=_c(size_id, name))
            assert got.dtype == np.uint8 and np.array_equal(got, want), (name, pname, np.argwhere(got != want)[:8].tolist())
            assert np.array_equal(got, nav_cost_from_distance(metres, r_robot, r_inflate, k)), (name, pname)
            assert nav.lastCostKernel() == KERNEL
            if name == "reach":
                cost_tab, _, R = fr.tables(size.res, r_robot, r_inflate, k)
                for cell, c in fc.reach_probes(size, R):
                    assert got[cell] == (cost_tab[c] if c <= R * R else 1), (pname, cell, c)
            a.setCostFieldFrom(pf, r_robot, r_inflate, WEIGHT, particle=1)
            host_field = cost_field_from_distance(metres, r_robot, r_inflate)
            assert np.array_equal(_bits(host_field), _bits(fr.field_from_occ(occ, size.res, r_robot, r_inflate, c=_c(size_id, name)))), (name, pname)
            b.setCostField(host_field, geom["xmin"], geom["ymin"], geom["resolution"], WEIGHT)
            assert a.costField() == b.costField() == dict(nx=xs, ny=xs, weight=WEIGHT, **geom)
            la, lb = a.costFieldLookup(centres), b.costFieldLookup(centres)
            assert np.array_equal(la, lb), (name, pname, int((la != lb).sum()))
        if name == "random":
            x0 = X0
            for tick in range(3):
                nz = np.random.default_rng(40 + tick).normal(0.0, np.sqrt(0.9), (64, a.steps, 2))
                assert a.newControls(*x0, nz) == b.newControls(*x0, nz)
                assert a.lastKernelNames() == b.lastKernelNames() and a.lastKernelNames()[0] == "mppi_rollout_field<1>"
                assert np.array_equal(a.costToGo(), b.costToGo()) and np.array_equal(a.getControls(), b.getControls())
                x0 = (x0[0] + 0.002, x0[1] - 0.001, x0[2] + 0.003)
    # slot 0 was never written: every tile id 0
    nav.setCostFrom(pf, *fc.params(size)["base"], particle=0)
    assert (nav.cost() == 1).all()
    for h in (a, b, nav, pf):
        h.close()


# ---- 2: the tile table ----------------------------------------------------------------------------------------------------------------
def _room_scan(pose, walls=rc.ROOM_SMALL):
    return orc.room_scan(pose, walls=walls, noise_sigma=0.0)


def test_slots_that_share_tiles_and_then_diverge_each_give_their_own_grid(gpu_pkg):
    """Slot 1 becomes a copy of slot 0 by gatherLocal (tables shared, copy-on-write), slot 2 a deep copy by copyParticle; one
    integrateScan into slot 1 makes its tiles private.  Each slot's grid is that of its own map."""
    from rtn_amd.nav import nav_cost_from_distance
    size = fc.SIZE["s96"]
    pf, nav = _filter(gpu_pkg, size, N=3), _nav(size)
    occ0 = fc.patterns(size)["one_tile"]
    _set_occ(pf, 0, occ0)
    pf.gatherLocal(np.array([-1, 0, -1], dtype=np.int32))
    pf.copyParticle(2, pf, 0)
    prm = fc.PARAMS_5CM["base"]
    grids = []
    for p in range(3):
        nav.setCostFrom(pf, *prm, particle=p)
        grids.append(nav.cost())
    want0 = fr.cost_from_occ(occ0, size.res, *prm)
    assert all(np.array_equal(g, want0) for g in grids)
    pose = (0.3, 0.1, -0.2)
    pf.integrateScan(1, _room_scan(pose), pose)
    for p in range(3):
        occ, metres = _occ_of(pf, p)
        nav.setCostFrom(pf, *prm, particle=p)
        got = nav.cost()
        assert np.array_equal(got, fr.cost_from_occ(occ, size.res, *prm)) and np.array_equal(got, nav_cost_from_distance(metres, *prm)), p
        if p != 1:
            assert np.array_equal(occ, occ0) and np.array_equal(got, want0), p
        else:
            assert occ.sum() > 100 and not np.array_equal(occ, occ0) and not np.array_equal(got, want0)      # the room's walls are in slot 1 alone
    nav.close(); pf.close()


# ---- 3: the best particle -----------------------------------------------------------------------------------------------------------
def test_best_particle_is_the_arg_max_of_the_weights_and_the_first_of_a_tie(gpu_pkg):
    size = fc.SIZE["s64"]
    pf, nav, m = _filter(gpu_pkg, size, N=4), _nav(size), _controller(gpu_pkg)
    prm = fc.PARAMS_5CM["base"]
    cells = ((10, 10), (20, 40), (40, 20), (50, 50))
    own = []
    for p, cell in enumerate(cells):
        occ = np.zeros((64, 64), dtype=np.uint8)
        occ[cell] = 1
        _set_occ(pf, p, occ)
        own.append(fr.cost_from_occ(occ, size.res, *prm))
    centres = np.stack([v.ravel() for v in nr.cell_centres(64, 64, -size.half, -size.half, size.res)], axis=1)
    for w, best in (([0.1, 0.4, 0.4, 0.1], 1), ([0.1, 0.2, 0.3, 0.4], 3), ([0.25, 0.25, 0.25, 0.25], 0), ([0.1, 0.2, 0.5, 0.2], 2)):
        pf.setParticles(w=np.array(w))
        nav.setCostFrom(pf, *prm)
        assert np.array_equal(nav.cost(), own[best]), (w, best)
        assert pf.getRobotState()[1] == best
        m.setCostFieldFrom(pf, prm[0], prm[1], WEIGHT)
        by_best = m.costFieldLookup(centres)
        m.setCostFieldFrom(pf, prm[0], prm[1], WEIGHT, particle=best)
        assert np.array_equal(by_best, m.costFieldLookup(centres)) and by_best.reshape(64, 64)[cells[best]] > 0.0
    for h in (m, nav, pf):
        h.close()


# ---- 4: a map drawn by scans ----------------------------------------------------------------------------------------------------------
def test_a_map_drawn_by_real_scans(gpu_pkg):
    from rtn_amd.nav import nav_cost_from_distance
    size = fc.SIZE["s80"]
    pf, nav = _filter(gpu_pkg, size, N=1), _nav(size)
    for pose in ((0.0, 0.0, 0.0), (0.07, 0.10, 0.05), (0.14, 0.20, 0.10)):
        pf.integrateScan(0, _room_scan(pose), pose)
    occ, metres = _occ_of(pf, 0)
    assert occ.sum() > 100
    for prm in fc.PARAMS_5CM.values():
        nav.setCostFrom(pf, *prm, particle=0)
        got = nav.cost()
        assert np.array_equal(got, fr.cost_from_occ(occ, size.res, *prm)) and np.array_equal(got, nav_cost_from_distance(metres, *prm)), prm
    nav.close(); pf.close()


# ---- 5: solving over a grid set on the device --------------------------------------------------------------------------------------------
def test_solve_field_and_path_after_a_device_set_grid_then_a_host_grid_replaces_it(gpu_pkg):
    """The path is asked for BEFORE anything has fetched the grid to the host, and again after the device grid has been replaced: the
    host copy of the solved grid is fetched at the path, from what the solve used."""
    size = fc.SIZE["s64"]
    pats = fc.patterns(size)
    prm = fc.PARAMS_5CM["base"]
    pf, nav = _filter(gpu_pkg, size, N=2), _nav(size)
    _set_occ(pf, 0, pats["one_tile"])
    _set_occ(pf, 1, pats["full_col"])
    grid0, grid1 = (fr.cost_from_occ(pats[n], size.res, *prm) for n in ("one_tile", "full_col"))
    goal, start = (10, 50), (50, 3)
    assert grid0[goal] == 1 and grid0[start] == 1 and 1 < grid0.max() <= 9
    want = nr.cost_to_go(grid0, goal)
    want_path, _ = nr.path(grid0, want, start)
    nav.setCostFrom(pf, *prm, particle=0)
    nav.solve(*goal)
    assert np.array_equal(nav.path(*start), want_path)
    assert np.array_equal(nav.costToGo(), want)
    assert np.array_equal(_bits(nav.field(10.0)), _bits(nr.field(want, size.res, 10.0)))
    assert np.array_equal(nav.cost(), grid0)
    # another device grid, unsolved: the last solution stays, path included
    nav.solve(*goal)
    nav.setCostFrom(pf, *prm, particle=1)
    assert np.array_equal(nav.cost(), grid1)
    assert np.array_equal(nav.path(*start), want_path) and np.array_equal(nav.costToGo(), want)
    # ... and the next solve uses it: a full column of wall cuts the map in two
    goal1 = (60, 50)
    nav.solve(*goal1)
    want1 = nr.cost_to_go(grid1, goal1)
    assert np.array_equal(nav.costToGo(), want1) and want1[start] == nr.UNREACHED
    assert np.array_equal(nav.path(5, 58), nr.path(grid1, want1, (5, 58))[0])
    # a blocked goal of a device-set grid is refused as ever
    col = int(np.argwhere(pats["full_col"])[0][1])
    assert grid1[5, col] == 0 and gpu_pkg.capi.lib().tbnav_nav_solve(nav._h, 5, col) == gpu_pkg.capi.ERR_INVALID_ARG
    # the host route replaces the grid
    host = np.ones((64, 64), dtype=np.uint8)
    host[30, 5:60] = 0
    nav.setCost(host)
    assert np.array_equal(nav.cost(), host) and nav.lastCostKernel() == KERNEL
    nav.solve(*goal)
    want2 = nr.cost_to_go(host, goal)
    assert np.array_equal(nav.costToGo(), want2) and np.array_equal(nav.path(*start), nr.path(host, want2, start)[0])
    nav.close(); pf.close()


# ---- 6: rejections -------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_grid_and_the_field_in_force(gpu_pkg):
    from rtn_amd.nav import GoalField
    c = gpu_pkg.capi
    L = c.lib()
    size = fc.SIZE["s64"]
    pf, nav, m = _filter(gpu_pkg, size, N=2), _nav(size), _controller(gpu_pkg)
    _set_occ(pf, 0, fc.patterns(size)["random"])
    grid = np.ones((64, 64), dtype=np.uint8)
    grid[7, 9] = 0
    nav.setCost(grid)
    prior = np.random.default_rng(1).random((7, 5)).astype(np.float32)
    m.setCostField(prior, 0.4, 0.1, 0.05, 3.0)
    centres = np.stack([v.ravel() for v in nr.cell_centres(7, 5, 0.4, 0.1, 0.05)], axis=1)
    field_before, geom_before = m.costFieldLookup(centres), m.costField()

    def unchanged():
        return (np.array_equal(nav.cost(), grid) and nav.lastCostKernel() == "" and m.costField() == geom_before and
                np.array_equal(m.costFieldLookup(centres), field_before))

    nan, inf = float("nan"), float("inf")
    for r_robot, r_inflate, k, status in ((-0.1, 0.45, 8.0, c.ERR_INVALID_ARG), (0.45, 0.45, 8.0, c.ERR_INVALID_ARG), (0.5, 0.45, 8.0, c.ERR_INVALID_ARG),
                                          (nan, 0.45, 8.0, c.ERR_INVALID_ARG), (0.1, nan, 8.0, c.ERR_INVALID_ARG), (0.1, inf, 8.0, c.ERR_INVALID_ARG),
                                          (0.1, 10.5, 8.0, c.ERR_INVALID_ARG), (0.1, 1.6, 8.0, c.ERR_UNSUPPORTED), (0.1, 10.0, 8.0, c.ERR_UNSUPPORTED)):
        assert L.tbnav_nav_set_cost_from_rbpf(nav._h, pf._h, 0, r_robot, r_inflate, k) == status, (r_robot, r_inflate, k)
        assert L.tbnav_mppi_set_cost_field_from_rbpf(m._h, pf._h, 0, r_robot, r_inflate, 1.0) == status, (r_robot, r_inflate)
        assert unchanged()
    for k in (-1.0, 63.5, nan, inf):
        assert L.tbnav_nav_set_cost_from_rbpf(nav._h, pf._h, 0, 0.10, 0.45, k) == c.ERR_INVALID_ARG and unchanged()
    for weight in (nan, inf):
        assert L.tbnav_mppi_set_cost_field_from_rbpf(m._h, pf._h, 0, 0.10, 0.45, weight) == c.ERR_INVALID_ARG and unchanged()
    for particle in (2, -2, 1 << 20):       # neither a slot nor TBNAV_NAV_BEST_PARTICLE
        assert L.tbnav_nav_set_cost_from_rbpf(nav._h, pf._h, particle, 0.10, 0.45, 8.0) == c.ERR_INVALID_ARG
        assert L.tbnav_mppi_set_cost_field_from_rbpf(m._h, pf._h, particle, 0.10, 0.45, 1.0) == c.ERR_INVALID_ARG and unchanged()
    assert L.tbnav_nav_set_cost_from_rbpf(nav._h, None, 0, 0.10, 0.45, 8.0) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_set_cost_from_rbpf(None, pf._h, 0, 0.10, 0.45, 8.0) == c.ERR_INVALID_ARG
    assert L.tbnav_mppi_set_cost_field_from_rbpf(m._h, None, 0, 0.10, 0.45, 1.0) == c.ERR_INVALID_ARG
    assert L.tbnav_mppi_set_cost_field_from_rbpf(None, pf._h, 0, 0.10, 0.45, 1.0) == c.ERR_INVALID_ARG and unchanged()
    # a nav handle whose grid is not the filter's: side, corner, resolution
    for kw in (dict(nx=96, ny=96), dict(nx=64, ny=62), dict(xmin=-1.6 + 1e-9), dict(ymin=float(np.nextafter(-1.6, 0.0))), dict(resolution=0.0500001)):
        g = dict(nx=64, ny=64, xmin=-1.6, ymin=-1.6, resolution=0.05)
        g.update(kw)
        other = GoalField(**g)
        og = np.ones((g["nx"], g["ny"]), dtype=np.uint8)
        og[1, 1] = 7
        other.setCost(og)
        assert L.tbnav_nav_set_cost_from_rbpf(other._h, pf._h, 0, 0.10, 0.45, 8.0) == c.ERR_INVALID_ARG, kw
        assert np.array_equal(other.cost(), og) and other.lastCostKernel() == ""
        other.close()
    # a handle without a grid has none to give
    fresh = _nav(size)
    buf = np.zeros((64, 64), dtype=np.uint8)
    assert L.tbnav_nav_get_cost(fresh._h, buf.ctypes.data) == c.ERR_INVALID_ARG and L.tbnav_nav_get_cost(nav._h, None) == c.ERR_INVALID_ARG
    fresh.close()
    # and the accepted call still works afterwards
    nav.setCostFrom(pf, 0.10, 0.45, 8.0, particle=0)
    assert np.array_equal(nav.cost(), fr.cost_from_occ(fc.patterns(size)["random"], size.res, 0.10, 0.45, 8.0)) and nav.lastCostKernel() == KERNEL
    for h in (m, nav, pf):
        h.close()


# ---- 7: no stored field -----------------------------------------------------------------------------------------------------------------
def test_a_filter_too_large_for_a_stored_field_feeds_the_planner(gpu_pkg):
    """70 000 particles of 64 x 64 cells: the stored field's allocation refuses more than 65 535 particles, so occDist — the host
    route's first step — is TBNAV_ERR_UNSUPPORTED on this handle, while the device route, which reads the tiles' bits, works; and it
    has not made the handle allocate that field on the way (occDist is refused afterwards as before)."""
    c = gpu_pkg.capi
    size = fc.SIZE["s64"]
    N = 70000
    pf, nav = _filter(gpu_pkg, size, N=N, pool_bytes=640 << 20), _nav(size)     # (create wants room for a tile per particle: 70 002 x 8.3 KB)
    occ = fc.patterns(size)["seam_rows"]
    _set_occ(pf, N - 1, occ, fresh_field=False)
    prm = fc.PARAMS_5CM["base"]
    for particle in (N - 1, 12345):
        nav.setCostFrom(pf, *prm, particle=particle)
        want = fr.cost_from_occ(occ if particle == N - 1 else np.zeros_like(occ), size.res, *prm)
        assert np.array_equal(nav.cost(), want), particle
    w = np.full(N, 0.5 / (N - 1))
    w[N - 1] = 0.5
    pf.setParticles(w=w)
    nav.setCostFrom(pf, *prm)
    assert np.array_equal(nav.cost(), fr.cost_from_occ(occ, size.res, *prm))
    with pytest.raises(c.TbnavError) as ei:
        pf.occDist(N - 1)
    assert ei.value.status == c.ERR_UNSUPPORTED
    nav.close(); pf.close()


# ---- 8: scenario U from a map ---------------------------------------------------------------------------------------------------------
def test_scenario_u_from_the_filters_map(gpu_pkg):
    """Scenario U's walls as cells of a particle's map (tests/nav_from_map_cases.py: scenario_u_occupancy), the filter created on U's
    grid: setCostFrom, solveAt, applyTo and the MPPI loop of tests/test_nav_gpu.py's scenario test.  The robot arrives within
    nav_restatement.U_MAX_TICKS and never stands on a blocked cell of the grid it was given."""
    from rtn_amd.nav import GoalField
    from rtn_amd.rbpf import ParticleFilter, default_params
    u = fc.U_FILTER
    pf = ParticleFilter(default_params(N=1, k=2, xmin=u["xmin"], xmax=u["xmax"], ymin=u["ymin"], ymax=u["ymax"], resolution=u["resolution"]))
    assert (pf.xsize, pf.ysize) == (nr.U_GRID["nx"], nr.U_GRID["ny"])
    occ = fc.scenario_u_occupancy()
    _set_occ(pf, 0, occ)
    nav = GoalField(**nr.U_GRID)
    nav.setCostFrom(pf, nr.U_R_ROBOT, nr.U_R_INFLATE, nr.U_K)
    cost = nav.cost()
    assert np.array_equal(cost, fr.cost_from_occ(occ, u["resolution"], nr.U_R_ROBOT, nr.U_R_INFLATE, nr.U_K))
    nav.solveAt(*nr.U_WAYPOINT[:2])
    assert nav.lastSolve()["goal"] == nr.U_GOAL_CELL
    m = make_mppi(gpu_pkg, nr.U_PRM)
    m.setWaypoint(*nr.U_WAYPOINT)
    m.setInitialControls(0.0, 0.0)
    nav.applyTo(m, nr.U_CAP, nr.U_WEIGHT)
    visited = []

    def tick(x, noise):
        visited.append(nr.cell_of(**nr.U_GRID, x=x[0], y=x[1]))
        return m.newControls(x[0], x[1], x[2], noise)
    ticks, least, x = nr.scenario_u_run(tick, seed=3)
    visited.append(nr.cell_of(**nr.U_GRID, x=x[0], y=x[1]))
    print("scenario U from the filter's map: ticks", ticks, "least distance to the walls", least, "end", x)
    assert ticks is not None and ticks <= nr.U_MAX_TICKS
    assert all(cell is not None and cost[cell] != 0 for cell in visited)
    m.close(); nav.close(); pf.close()
