"""CPU proof of the frontier case table (tests/nav_frontier_cases.py) against the restatement (tests/nav_frontier_restatement.py): every
case reaches what its name says, every planted error changes the case named for it, the several-goal Dijkstra equals the one-goal one,
and the exploration loop over the oracle's GridMapper ends with the room explored."""
import functools

import numpy as np
import pytest

import nav_frontier_cases as cs
import nav_frontier_restatement as ff
import nav_from_map_restatement as fr
import nav_restatement as nr

IDS = [s.id for s in cs.SIZES]


@functools.lru_cache(maxsize=None)
def _found(size_id, name):
    size = cs.SIZE[size_id]
    case = cs.cases(size)[name]
    front, lab, seed = ff.find(ff.export_map(case.lo), size.xsize, case.cost, cs.visited_mask(size.xsize, case.discs), case.min_cells)
    for a in (front, lab, seed):
        a.setflags(write=False)
    return front, lab, seed


def test_the_five_values_export_as_their_names_say():
    assert [ff.export_value(v) for v in cs.VALUES] == [-1, 0, 0, 100, 82]
    lo = np.array([[cs.U, cs.F], [cs.O, cs.K]])
    unknown, free = ff.classes(ff.export_map(lo), 2)
    assert unknown.tolist() == [[True, False], [False, False]] and free.tolist() == [[False, True], [False, False]]     # (the export is transposed, classes() turns it back)


@pytest.mark.parametrize("size_id", IDS)
def test_each_case_reaches_what_it_names(size_id):
    size = cs.SIZE[size_id]
    xs, last = size.xsize, size.xsize - 1
    table = cs.cases(size)
    get = lambda name: _found(size_id, name)
    for name in ("all_unknown", "all_free", "edge_free", "known_neither"):
        front, lab, seed = get(name)
        assert not front.any() and (lab == ff.UNREACHED).all() and not seed.any(), name
    if xs > 32:
        for name, axis, at in (("half_row31", 0, 31), ("half_row32", 0, 32), ("half_col31", 1, 31), ("half_col32", 1, 32),
                               ("half_row31_touched", 0, 31), ("half_col31_touched", 1, 31)):
            front, lab, seed = get(name)
            want = np.zeros((xs, xs), dtype=bool)
            want[(at, slice(None)) if axis == 0 else (slice(None), at)] = True
            assert np.array_equal(front, want), name
            assert set(np.unique(lab[front]).tolist()) == {at * xs if axis == 0 else at} and seed[front].all()
        assert len(cs.cases(size)) == 8 + 9
    else:
        assert "half_row31" not in table
    # the diagonal chain: one cluster, labelled by its first cell
    front, lab, seed = get("diag_chain")
    k0 = cs.diag_start(xs)
    assert front.sum() == 8 and all(front[k, k] for k in range(k0, k0 + 8)) and (lab[front] == k0 * xs + k0).all() and seed.sum() == 8
    if xs > 32:
        assert front[31, 31] and front[32, 32]      # through the corner four tiles share
    # two runs, one unknown row between them: two clusters
    front, lab, seed = get("two_runs")
    assert sorted(np.unique(lab[front]).tolist()) == [10 * xs + 5, 12 * xs + 5] and front.sum() == 20 and seed.sum() == 20
    # the serpentine: one cluster inside one tile, whose chain is longer than the kernel's 128 sweeps
    front, lab, seed = get("serpentine")
    rows = cs.serpentine_rows(xs)
    assert (lab[front] == 0).all() and front[:rows, :min(xs, 32)].sum() == front.sum() > 2 * 128
    chain = nr.cost_to_go(np.where(front, 1, 0).astype(np.uint8), (0, 0), corner_rule=False)
    assert int(chain[front].max()) // 14 > 128        # even along diagonal short cuts the far end is more than 128 steps from the root
    # a blocked cell splits a cluster
    front, lab, seed = get("blocked_split")
    assert not front[10, 12] and sorted(np.unique(lab[front]).tolist()) == [10 * xs + 4, 10 * xs + 13] and front.sum() == 16 and seed.sum() == 16
    # a visited disc removes a part
    front, lab, seed = get("visited_part")
    assert front[20, 4:15].all() and front.sum() == 11 and not front[20, 15:21].any() and cs.visited_mask(xs, table["visited_part"].discs).sum() == 29
    # sizes min_cells - 1 and min_cells
    front, lab, seed = get("min_cells_edge")
    assert [f["size"] for f in ff.frontier_list(lab, cs.MIN_CELLS)] == [7, 8] and seed.sum() == 8 and seed[9, 2:10].all()
    assert ff.counts(lab, cs.MIN_CELLS) == dict(cells=15, clusters=2, seed_clusters=1, seed_cells=8)
    # an unknown cell across a corner does not count, one across an edge does
    front, lab, seed = get("diagonal_unknown")
    assert np.argwhere(front).tolist() == [[20, 20]] and seed[20, 20]
    # the list's fields on a case with several clusters
    rec = ff.frontier_list(get("two_runs")[1], cs.MIN_CELLS)
    assert rec[0] == dict(root=(10, 5), size=10, seeds=True, box=(10, 5, 10, 14), sum_ix=100, sum_iy=95)


@pytest.mark.parametrize("size_id", IDS)
def test_each_planted_error_changes_its_case(size_id):
    size = cs.SIZE[size_id]
    table = cs.cases(size)
    for wrong, name in cs.PLANTED:
        case = table[name]
        right = _found(size_id, name)
        got = ff.find(ff.export_map(case.lo), size.xsize, case.cost, cs.visited_mask(size.xsize, case.discs), case.min_cells, **{wrong: True})
        assert not (np.array_equal(got[1], right[1]) and np.array_equal(got[2], right[2])), (wrong, name)
    front8 = ff.find(ff.export_map(table["diag_chain"].lo), size.xsize, table["diag_chain"].cost, None, cs.MIN_CELLS, conn4=True)
    assert len(np.unique(front8[1][front8[0]])) == 8 and not front8[2].any()       # eight clusters of one cell with 4-connectivity


def test_several_goals_with_one_goal_is_the_one_goal_solve_and_with_more_the_minimum():
    rng = np.random.default_rng(11)
    cost = rng.integers(0, 6, (40, 37)).astype(np.uint8)
    free = np.argwhere(cost != 0)
    goals = [tuple(int(v) for v in free[i]) for i in rng.choice(len(free), 5, replace=False)]
    one = [nr.cost_to_go(cost, g) for g in goals]
    assert np.array_equal(ff.cost_to_go_goals(cost, goals[:1]), one[0])
    assert np.array_equal(ff.cost_to_go_goals(cost, goals + goals[:2]), np.minimum.reduce(one))


def test_disc_is_cut_at_the_grid():
    d = ff.disc(10, 12, 0, 11, 2)
    assert d.sum() == 6 and d[0, 9] and d[2, 11] and d[1, 10] and not d[2, 10]
    assert ff.disc(5, 5, 2, 2, 0).sum() == 1


# ---- the exploration loop on the CPU ------------------------------------------------------------------------------------------
def explore_cpu(start):
    """The loop of nav_frontier_cases.explore over the oracle's GridMapper and the restatements; also returns the exported map at the end."""
    import oracle_api as orc
    m = cs.EXPLORE_MAP
    xs = m["xsize"]
    grid = orc.GridAPI("orc", grid=(m["res"], -m["half"], m["half"], -m["half"], m["half"]))
    assert (grid.xsize, grid.ysize) == (xs, xs)
    visited = np.zeros((xs, xs), dtype=bool)

    def integrate(scan, pose):
        grid.integrate_scan(scan, pose, esdf=False)

    def plan(cell):
        exported = grid.grid_map()
        occ = (exported.reshape(xs, xs).T == 100).astype(np.uint8)
        cost = fr.cost_from_occ(occ, m["res"], *cs.EXPLORE_INFLATION)
        _, _, seed = ff.find(exported, xs, cost, visited, cs.MIN_CELLS)
        if not seed.any():
            return None
        d = ff.cost_to_go_goals(cost, ff.goal_cells(seed))
        path, _ = nr.path(cost, d, cell)
        assert seed[tuple(path[-1])]
        return path

    def mark(cell):
        visited[:] |= ff.disc(xs, xs, cell[0], cell[1], cs.EXPLORE_MARK_RADIUS)

    run = cs.explore(start, integrate, plan, mark)
    run["exported"] = grid.grid_map()
    grid.close()
    return run


@functools.lru_cache(maxsize=None)
def explore_cpu_cached(start):
    return explore_cpu(start)


@pytest.mark.parametrize("start", cs.EXPLORE_STARTS)
def test_exploration_loop_ends_with_the_room_explored(start):
    run = explore_cpu_cached(start)
    unknown, inside = cs.explore_unknown_inside(run["exported"])
    print("exploration from", start, ": iterations", len(run["cells"]), "marks", len(run["marks"]), "unknown cells inside", unknown, "of", inside)
    assert run["done"] and len(run["cells"]) <= cs.EXPLORE_MAX_ITER
    assert unknown <= cs.EXPLORE_MAX_UNKNOWN * inside
