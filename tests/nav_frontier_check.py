"""TEST INFRASTRUCTURE — the == comparison of one frontier find and the solves that follow it against tests/nav_frontier_restatement.py,
shared by tests/test_nav_frontier_gpu.py (the case table) and tests/test_nav_frontier_fuzz_gpu.py (drawn maps)."""
import numpy as np

import nav_frontier_restatement as ff
import nav_restatement as nr

KERNELS = ["nav_frontier_mark", "nav_frontier_label", "nav_frontier_sizes", "nav_frontier_seeds"]
CAP = 10.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def install(nav, cost, discs):
    """The cost grid and the visited mask of a case; returns the mask as the restatement draws it."""
    xs = cost.shape[0]
    nav.setCost(cost)
    nav.clearVisited()
    mask = np.zeros(cost.shape, dtype=bool)
    for ix, iy, r in discs:
        nav.markVisited(ix, iy, r)
        mask |= ff.disc(xs, cost.shape[1], ix, iy, r)
    assert np.array_equal(nav.visited(), mask.astype(np.uint8))
    return mask


def check_find(nav, pf, slot, cost, mask, min_cells, tag, particle="slot"):
    """findFrontiers on the slot's map against the restatement over the slot's EXPORTED map (the export is the definition): labels,
    list, counts, kernel names.  Returns (info, frontier, labels, seeds) of the restatement."""
    xs = cost.shape[0]
    exported = pf.particleMap(slot)
    front, lab, seed = ff.find(exported, xs, cost, mask, min_cells)
    info = nav.findFrontiers(pf, min_cells, particle=slot if particle == "slot" else particle)
    got = nav.frontierLabels()
    assert got.dtype == np.uint32 and np.array_equal(got, lab), (tag, np.argwhere(got != lab)[:8].tolist())
    assert nav.frontiers() == ff.frontier_list(lab, min_cells), tag
    want = ff.counts(lab, min_cells)
    assert {k: info[k] for k in want} == want and info["found"] and info["min_cells"] == min_cells, (tag, info, want)
    assert info["rounds"] >= 1 and info["launches"] >= info["rounds"] and nav.lastFrontiers() == info
    assert (info["tile_visits"] == 0) == (not front.any()), tag
    assert nav.lastFrontierKernels() == KERNELS
    return info, front, lab, seed


def check_solves(nav, cost, seed, res, tag):
    """solveFrontiers and solveGoals with the same cells: cost-to-go, seed set, field bits, path and its last cell."""
    if not seed.any():
        return
    cells = ff.goal_cells(seed)
    want = ff.cost_to_go_goals(cost, cells)
    assert nav.solveFrontiers() is True
    d = nav.costToGo()
    assert np.array_equal(d, want), (tag, np.argwhere(d != want)[:8].tolist())
    assert np.array_equal(d == 0, seed), tag                                   # the goals are the seeds, all of them and nothing else
    info = nav.lastSolve()
    assert info["goal"] == (-1, -1) and info["solved"] and info["kernel"] == "nav_relax_tiles"
    assert np.array_equal(bits(nav.field(CAP)), bits(nr.field(want, res, CAP))), tag
    reached = np.where(want == nr.UNREACHED, 0, want)
    start = tuple(int(v) for v in np.unravel_index(int(np.argmax(reached)), reached.shape))    # the reached cell farthest from every seed
    want_path, _ = nr.path(cost, want, start)
    for solve in ("frontiers", "goals"):
        if solve == "goals":
            nav.solveGoals(cells)
            assert np.array_equal(nav.costToGo(), want), tag
            assert nav.lastSolve()["goal"] == cells[0] and np.array_equal(bits(nav.field(CAP)), bits(nr.field(want, res, CAP)))
        got_path = nav.path(*start)
        assert np.array_equal(got_path, want_path) and seed[tuple(got_path[-1])], (tag, solve)
