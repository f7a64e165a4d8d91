"""TEST INFRASTRUCTURE — what the restatement (tests/nav_gain_restatement.py) gives for a case of tests/nav_gain_cases.py, computed once
and shared read-only by the CPU and the GPU tests, and the == comparison of one find with gain and the ranked solves that follow it,
shared by tests/test_nav_gain_gpu.py (the case table) and tests/test_nav_gain_fuzz_gpu.py (drawn maps)."""
import functools

import numpy as np

import nav_frontier_check as ck
import nav_frontier_restatement as ff
import nav_gain_cases as gc
import nav_gain_restatement as gr
import nav_restatement as nr

CAP = ck.CAP


def kernels(R):
    return ["nav_gain_classes", "nav_gain_list", "nav_frontier_gain<%d>" % (32 if R <= 32 else 128)]


@functools.lru_cache(maxsize=None)
def expected(size_id, name):
    """(frontier, labels, seeds, gain) of a case, read-only."""
    size = gc.SIZE[size_id]
    case = gc.cases(size)[name]
    out = gr.find_gain(ff.export_map(case.lo), size.xsize, case.cost, None, case.min_cells, case.R)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_ranked(size_id, name, weight):
    """(start values, cost-to-go) of a case's ranked solve, read-only."""
    case = gc.cases(gc.SIZE[size_id])[name]
    _, _, seed, gain = expected(size_id, name)
    start = gr.start_values(gain, seed, weight)
    d = gr.cost_to_go_ranked(case.cost, start)
    start.setflags(write=False); d.setflags(write=False)
    return start, d


def farthest(d):
    """The reached cell farthest from every seed."""
    reached = np.where(d == nr.UNREACHED, 0, d)
    return tuple(int(v) for v in np.unravel_index(int(np.argmax(reached)), reached.shape))


def check_find_gain(nav, pf, slot, min_cells, R, want, tag, particle="slot"):
    """findFrontiersGain on the slot's map against want = (frontier, labels, seeds, gain) of the restatement: the plain find's results,
    the gain array, the gain info, the cluster list, the kernel names."""
    front, lab, seed, gain = want
    info, gi = nav.findFrontiersGain(pf, R, min_cells, particle=slot if particle == "slot" else particle)
    assert np.array_equal(nav.frontierLabels(), lab), tag
    assert nav.frontiers() == ff.frontier_list(lab, min_cells), tag
    counts = ff.counts(lab, min_cells)
    assert {k: info[k] for k in counts} == counts and info["found"] and info["min_cells"] == min_cells and nav.lastFrontiers() == info, (tag, info)
    assert nav.lastFrontierKernels() == ck.KERNELS
    got = nav.frontierGain()
    assert got.dtype == np.uint32 and np.array_equal(got, gain), (tag, np.argwhere(got != gain)[:8].tolist())
    assert gi == gr.gain_info(gain, seed, R) and nav.lastGain() == gi, (tag, gi, gr.gain_info(gain, seed, R))
    assert nav.frontierGainList() == gr.gain_list(lab, gain, min_cells), tag
    assert nav.lastGainKernels() == (kernels(R) if seed.any() else []), tag
    return info, gi


def check_ranked(nav, cost, seed, gain, res, weight, tag, want=None, start_cell=None):
    """solveFrontiersRanked against the restatement: cost-to-go, info, field bits, path and its last cell.  Returns the path."""
    start, d = want if want is not None else (lambda s: (s, gr.cost_to_go_ranked(cost, s)))(gr.start_values(gain, seed, weight))
    assert nav.solveFrontiersRanked(weight) is True
    got = nav.costToGo()
    assert np.array_equal(got, d), (tag, weight, np.argwhere(got != d)[:8].tolist())
    info = nav.lastSolve()
    assert info["goal"] == (-1, -1) and info["solved"] and info["kernel"] == "nav_relax_tiles"
    assert np.array_equal(ck.bits(nav.field(CAP)), ck.bits(nr.field(d, res, CAP))), (tag, weight)
    cell = farthest(d) if start_cell is None else start_cell
    want_path = gr.path_ranked(cost, d, start, cell)
    path = nav.path(*cell)
    end = tuple(int(v) for v in path[-1])
    assert np.array_equal(path, want_path) and seed[end] and d[end] == start[end], (tag, weight)
    return path
