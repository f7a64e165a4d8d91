"""GPU tests of the frontiers ranked by information gain (include/tbnav_nav.h G17-G20, csrc/nav_gain.hip) against their restatement
(tests/nav_gain_restatement.py), all with ==: the case table (tests/nav_gain_cases.py) through setLogOdds, weight 0 against the plain
solve, the plain find's results, the kernels' names either side of R = 32, the tile tables, the best particle, a map drawn by scans,
the rejections, the hand-over to MPPI, and the exploration loop with the ranked plan against the CPU leg's."""
import ctypes as C

import numpy as np
import pytest

import nav_frontier_cases as fcs
import nav_frontier_check as ck
import nav_frontier_restatement as ff
import nav_gain_cases as gc
import nav_gain_check as gk
import nav_gain_restatement as gr
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


def _nav(size):
    from rtn_amd.nav import GoalField
    return GoalField(size.xsize, size.xsize, -size.half, -size.half, size.res)


def _scan(pose):
    """A scan of the small room with a sector of beams that do not return: the map ends there."""
    scan = orc.room_scan(pose, walls=rc.ROOM_SMALL, noise_sigma=0.0)
    scan[100:200] = 4.0
    return scan


def _want(pf, slot, cost, mask, min_cells, R):
    """The restatement over the slot's EXPORTED map (the export is the definition of the classes)."""
    return gr.find_gain(pf.particleMap(slot), cost.shape[0], cost, mask, min_cells, R)


# ---- 1: the case table -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size_id", [s.id for s in gc.SIZES])
def test_every_case_equals_the_restatement(gpu_pkg, size_id):
    """Every case in a slot of its own that nobody has written before (an all-zero tile then stays the shared tile, id 0): gain array,
    gain info, cluster gain list and kernel names, then the ranked solves of weights 0, 1, 2 and 4096 — weight 0 also against
    solveFrontiers bit for bit."""
    size = gc.SIZE[size_id]
    table = gc.cases(size)
    pf, nav = _filter(gpu_pkg, size, N=len(table)), _nav(size)
    assert nav.lastGainKernels() == [] and not nav.lastGain()["computed"]
    for slot, (name, case) in enumerate(table.items()):
        pf.setLogOdds(slot, case.lo.reshape(-1))
        assert np.array_equal(pf.particleMap(slot), ff.export_map(case.lo)), name
        ck.install(nav, case.cost, case.discs)
        want = gk.expected(size_id, name)
        info, gi = gk.check_find_gain(nav, pf, slot, case.min_cells, case.R, want, (size_id, name))
        seed, gain = want[2], want[3]
        if not seed.any():
            assert gi["viewpoints"] == 0 and gi["computed"] and nav.solveFrontiersRanked(1) is False
            continue
        for w in gc.WEIGHTS:
            start_cell = gc.NOOK_START if name == "nook" else None
            path = gk.check_ranked(nav, case.cost, seed, gain, size.res, w, (size_id, name), want=gk.expected_ranked(size_id, name, w), start_cell=start_cell)
            if name == "nook":
                assert tuple(int(v) for v in path[-1]) == gc.NOOK_ENDS[w]
            if w == 0:
                d0, f0, p0 = nav.costToGo(), nav.field(gk.CAP), nav.path(*gk.farthest(gk.expected_ranked(size_id, name, 0)[1]))
                assert nav.solveFrontiers() is True
                assert np.array_equal(nav.costToGo(), d0) and np.array_equal(ck.bits(nav.field(gk.CAP)), ck.bits(f0))
                assert np.array_equal(nav.path(*gk.farthest(d0)), p0)
    nav.close(); pf.close()


# ---- 2: the plain find, and the kernels either side of the threshold -----------------------------------------------------------------
def test_plain_find_results_and_kernel_names_at_32_and_33(gpu_pkg):
    size = gc.SIZE["s96"]
    table = gc.cases(size)
    pf, nav = _filter(gpu_pkg, size, N=1), _nav(size)
    case = table["ranges_R32"]
    pf.setLogOdds(0, case.lo.reshape(-1))
    mask = ck.install(nav, case.cost, ())
    info, front, lab, seed = ck.check_find(nav, pf, 0, case.cost, mask, case.min_cells, "plain")
    labels, listed = nav.frontierLabels(), nav.frontiers()
    assert not nav.lastGain()["computed"] and nav.lastGainKernels() == []
    for R, kernel in ((32, "nav_frontier_gain<32>"), (33, "nav_frontier_gain<128>")):
        info_g, gi = gk.check_find_gain(nav, pf, 0, case.min_cells, R, gk.expected("s96", f"ranges_R{R}"), ("names", R))
        for k in ("found", "min_cells", "cells", "clusters", "seed_clusters", "seed_cells"):
            assert info_g[k] == info[k], k
        assert np.array_equal(nav.frontierLabels(), labels) and nav.frontiers() == listed
        assert nav.lastGainKernels() == ["nav_gain_classes", "nav_gain_list", kernel] and gi["range_cells"] == R
    # a later plain find leaves the handle with no gain
    nav.findFrontiers(pf, case.min_cells, particle=0)
    assert not nav.lastGain()["computed"] and nav.lastGainKernels() == []
    # the profile hook gives the same results and five stage times
    info_p, gi_p, us = nav.profileFindFrontiersGain(pf, 33, case.min_cells, particle=0)
    assert gi_p == gr.gain_info(gk.expected("s96", "ranges_R33")[3], seed, 33) and sorted(us) == sorted(("mark", "label", "sizes", "seeds", "gain"))
    assert all(v >= 0.0 for v in us.values()) and us["gain"] > 0.0 and np.array_equal(nav.frontierGain(), gk.expected("s96", "ranges_R33")[3])
    nav.close(); pf.close()


# ---- 3: the tile table -----------------------------------------------------------------------------------------------------------------
def test_slots_that_share_tiles_and_then_diverge_each_give_their_own_gain(gpu_pkg):
    size = gc.SIZE["s96"]
    pf, nav = _filter(gpu_pkg, size, N=3), _nav(size)
    case = gc.cases(size)["ranges_R33"]
    pf.setLogOdds(0, case.lo.reshape(-1))
    pf.gatherLocal(np.array([-1, 0, -1], dtype=np.int32))
    pf.copyParticle(2, pf, 0)
    mask = ck.install(nav, case.cost, ())
    shared = gk.expected("s96", "ranges_R33")
    for p in range(3):
        gk.check_find_gain(nav, pf, p, case.min_cells, case.R, shared, ("shared", p))
    pose = (0.3, 0.1, -0.2)
    pf.integrateScan(1, _scan(pose), pose)
    for p in (0, 2):
        gk.check_find_gain(nav, pf, p, case.min_cells, case.R, shared, ("diverged", p))
    want1 = _want(pf, 1, case.cost, mask, case.min_cells, case.R)
    gk.check_find_gain(nav, pf, 1, case.min_cells, case.R, want1, ("diverged", 1))
    assert not np.array_equal(want1[3], shared[3]) and want1[2].any()
    gk.check_ranked(nav, case.cost, want1[2], want1[3], size.res, 2, "diverged")
    nav.close(); pf.close()


# ---- 4: the best particle --------------------------------------------------------------------------------------------------------------
def test_best_particle_is_the_arg_max_of_the_weights_and_the_first_of_a_tie(gpu_pkg):
    size = gc.SIZE["s64"]
    pf, nav = _filter(gpu_pkg, size, N=4), _nav(size)
    cost = fcs.base_cost(64)
    mask = ck.install(nav, cost, ())
    for p in range(4):
        lo = np.full((64, 64), fcs.K)
        lo[10 + 10 * p, 5:20 + p] = fcs.F
        lo[11 + 10 * p: 14 + 10 * p + p, 5:20 + p] = fcs.U
        pf.setLogOdds(p, lo.reshape(-1))
    wants = [_want(pf, p, cost, mask, fcs.MIN_CELLS, 8) for p in range(4)]
    assert len({int(w[3].sum()) for w in wants}) == 4
    for w, best in (([0.1, 0.4, 0.4, 0.1], 1), ([0.1, 0.2, 0.3, 0.4], 3), ([0.25, 0.25, 0.25, 0.25], 0), ([0.1, 0.2, 0.5, 0.2], 2)):
        pf.setParticles(w=np.array(w))
        gk.check_find_gain(nav, pf, best, fcs.MIN_CELLS, 8, wants[best], ("best", w), particle=None)
        assert pf.getRobotState()[1] == best
    nav.close(); pf.close()


# ---- 5: a map drawn by scans -----------------------------------------------------------------------------------------------------------
def test_a_map_drawn_by_three_scans(gpu_pkg):
    size = gc.SIZE["s80"]
    pf, nav = _filter(gpu_pkg, size, N=1), _nav(size)
    for pose in ((0.0, 0.0, 0.0), (0.07, 0.10, 0.05), (0.14, 0.20, 0.10)):
        pf.integrateScan(0, _scan(pose), pose)
    nav.setCostFrom(pf, 0.10, 0.45, 8.0, particle=0)
    cost = nav.cost()
    nav.markVisited(40, 60, 6)
    mask = ff.disc(80, 80, 40, 60, 6)
    for min_cells, R in ((1, 12), (8, 40)):
        want = _want(pf, 0, cost, mask, min_cells, R)
        info, gi = gk.check_find_gain(nav, pf, 0, min_cells, R, want, ("scans", min_cells, R))
        assert want[2].any() and gi["gain_max"] > gi["gain_min"]
        for w in (0, 3):
            gk.check_ranked(nav, cost, want[2], want[3], size.res, w, ("scans", min_cells, R))
    nav.close(); pf.close()


# ---- 6: rejections ----------------------------------------------------------------------------------------------------------------------
def test_rejections_change_nothing(gpu_pkg):
    c = gpu_pkg.capi
    L = c.lib()
    size = gc.SIZE["s64"]
    case = gc.cases(size)["ranges_R8"]
    pf, nav = _filter(gpu_pkg, size, N=2), _nav(size)
    pf.setLogOdds(0, case.lo.reshape(-1))
    info, gi = c.NavFrontierInfo(), c.NavGainInfo()
    buf32 = np.zeros((64, 64), dtype=np.uint32)
    n = C.c_int32(-5)
    ck.install(nav, case.cost, ())
    # ranked before any find, gain results before any gain
    assert L.tbnav_nav_solve_frontiers_ranked(nav._h, 1) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_get_frontier_gain(nav._h, buf32.ctypes.data) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_frontier_gain_list(nav._h, None, 0, C.byref(n)) == c.ERR_INVALID_ARG and n.value == -5
    # ranked after a plain find: there is no gain on the handle
    nav.findFrontiers(pf, case.min_cells, particle=0)
    assert L.tbnav_nav_solve_frontiers_ranked(nav._h, 1) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_get_frontier_gain(nav._h, buf32.ctypes.data) == c.ERR_INVALID_ARG
    want = gk.expected("s64", "ranges_R8")
    _, gi0 = gk.check_find_gain(nav, pf, 0, case.min_cells, case.R, want, "first")
    nav.solve(40, 40)
    d0, info0, lab0 = nav.costToGo(), nav.lastSolve(), nav.frontierLabels()
    path0 = nav.path(5, 5)

    def unchanged():
        return (np.array_equal(nav.frontierGain(), want[3]) and nav.lastGain() == gi0 and np.array_equal(nav.frontierLabels(), lab0) and
                np.array_equal(nav.costToGo(), d0) and nav.lastSolve() == info0 and np.array_equal(nav.path(5, 5), path0) and
                nav.lastGainKernels() == gk.kernels(case.R))

    for R in (0, 129, -1):
        assert L.tbnav_nav_find_frontiers_gain(nav._h, pf._h, 0, case.min_cells, R, C.byref(info), C.byref(gi)) == c.ERR_INVALID_ARG and unchanged()
    for particle, min_cells in ((0, 0), (2, 1), (-2, 1)):      # the plain find's rejections are its own
        assert L.tbnav_nav_find_frontiers_gain(nav._h, pf._h, particle, min_cells, 8, C.byref(info), C.byref(gi)) == c.ERR_INVALID_ARG and unchanged()
    assert L.tbnav_nav_find_frontiers_gain(nav._h, None, 0, 1, 8, C.byref(info), C.byref(gi)) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_find_frontiers_gain(None, pf._h, 0, 1, 8, C.byref(info), C.byref(gi)) == c.ERR_INVALID_ARG and unchanged()
    ms = (C.c_float * 5)()
    assert L.tbnav_nav_profile_find_frontiers_gain(nav._h, pf._h, 0, 1, 8, C.byref(info), C.byref(gi), None) == c.ERR_INVALID_ARG and unchanged()
    assert L.tbnav_nav_profile_find_frontiers_gain(nav._h, pf._h, 0, 1, 129, C.byref(info), C.byref(gi), ms) == c.ERR_INVALID_ARG and unchanged()
    for w in (-1, 4097):
        assert L.tbnav_nav_solve_frontiers_ranked(nav._h, w) == c.ERR_INVALID_ARG and unchanged()
    assert L.tbnav_nav_solve_frontiers_ranked(None, 1) == c.ERR_INVALID_ARG
    # a buffer too small for the list: the number needed
    assert L.tbnav_nav_frontier_gain_list(nav._h, (c.NavFrontierGain * 1)(), 0, C.byref(n)) == c.ERR_INVALID_ARG and n.value == len(gr.gain_list(want[1], want[3], 1)) > 0
    # the grid or the mask set again since the find: its seeds are no goals any more
    nav.setCost(case.cost)
    assert L.tbnav_nav_solve_frontiers_ranked(nav._h, 1) == c.ERR_INVALID_ARG and unchanged()
    nav.findFrontiersGain(pf, case.R, case.min_cells, particle=0)
    nav.markVisited(0, 0, 0)
    assert L.tbnav_nav_solve_frontiers_ranked(nav._h, 1) == c.ERR_INVALID_ARG
    nav.findFrontiersGain(pf, case.R, case.min_cells, particle=0)
    nav.clearVisited()
    assert L.tbnav_nav_solve_frontiers_ranked(nav._h, 1) == c.ERR_INVALID_ARG and unchanged()
    # no seed: UNSUPPORTED, and the last solution survives
    _, gi20 = nav.findFrontiersGain(pf, case.R, 20, particle=0)
    assert gi20 == dict(computed=True, range_cells=8, rays=48, viewpoints=0, gain_min=0, gain_max=0, best=(-1, -1))
    assert L.tbnav_nav_solve_frontiers_ranked(nav._h, 1) == c.ERR_UNSUPPORTED and nav.solveFrontiersRanked(1) is False
    assert np.array_equal(nav.costToGo(), d0) and nav.lastSolve() == info0 and np.array_equal(nav.path(5, 5), path0)
    assert not nav.frontierGain().any() and nav.lastGainKernels() == []
    assert all(r["gain_max"] == 0 and r["best"] == (-1, -1) for r in nav.frontierGainList())
    # and the accepted calls still work afterwards; a ranked solution keeps its stop rule when a plain find follows it
    nav.findFrontiersGain(pf, case.R, case.min_cells, particle=0)
    gk.check_ranked(nav, case.cost, want[2], want[3], size.res, 4096, "after")
    start, d = gk.expected_ranked("s64", "ranges_R8", 4096)
    cell = gk.farthest(d)
    nav.findFrontiers(pf, 20, particle=0)
    assert np.array_equal(nav.path(*cell), gr.path_ranked(case.cost, d, start, cell))
    nav.close(); pf.close()


# ---- 7: the hand-over -------------------------------------------------------------------------------------------------------------------
def test_apply_to_after_a_ranked_solve_equals_set_cost_field_of_the_host_array(gpu_pkg):
    size = gc.SIZE["s64"]
    case = gc.cases(size)["ranges_R8"]
    pf, nav = _filter(gpu_pkg, size, N=1), _nav(size)
    pf.setLogOdds(0, case.lo.reshape(-1))
    ck.install(nav, case.cost, ())
    nav.findFrontiersGain(pf, case.R, case.min_cells, particle=0)
    assert nav.solveFrontiersRanked(2)
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
@pytest.mark.parametrize("k", range(len(fcs.EXPLORE_STARTS)))
def test_exploration_loop_with_the_ranked_plan_visits_the_cells_of_the_cpu_loop(gpu_pkg, k):
    """tbnav_rbpf_integrate_scan at the true pose, one particle; setCostFrom, findFrontiersGain, solveFrontiersRanked, path, markVisited."""
    from rtn_amd.nav import GoalField
    from rtn_amd.rbpf import ParticleFilter, default_params
    import test_nav_gain_cases as cpu
    start = fcs.EXPLORE_STARTS[k]
    m = fcs.EXPLORE_MAP
    pf = ParticleFilter(default_params(N=1, k=2, map_min=-m["half"], map_max=m["half"], resolution=m["res"]))
    nav = GoalField(m["xsize"], m["xsize"], -m["half"], -m["half"], m["res"])
    assert pf.xsize == m["xsize"]

    def plan(cell):
        nav.setCostFrom(pf, *fcs.EXPLORE_INFLATION, particle=0)
        nav.findFrontiersGain(pf, gc.EXPLORE_GAIN_RANGE, fcs.MIN_CELLS, particle=0)
        if not nav.solveFrontiersRanked(gc.EXPLORE_GAIN_WEIGHT):
            return None
        return nav.path(*cell)

    run = fcs.explore(start, lambda scan, pose: pf.integrateScan(0, scan, pose), plan,
                      lambda cell: nav.markVisited(cell[0], cell[1], fcs.EXPLORE_MARK_RADIUS))
    want = cpu.explore_cpu_ranked_cached(start)
    assert run["cells"] == want["cells"] and run["marks"] == want["marks"] and run["done"] and want["done"]
    assert np.array_equal(pf.particleMap(0), want["exported"])
    nav.close(); pf.close()
