"""CPU proof of the gain case table (tests/nav_gain_cases.py) against the restatement (tests/nav_gain_restatement.py): every case reaches
what its name says, every planted error changes the case named for it, the host-only ring equals the restatement's for every range,
G20's bound holds as arithmetic, the nook and the doorway flip between two adjacent weights, and the exploration loop with the ranked
plan over the oracle's GridMapper ends with no seed left."""
import functools

import numpy as np
import pytest

import nav_frontier_cases as fcs
import nav_frontier_restatement as ff
import nav_from_map_restatement as fr
import nav_gain_cases as gc
import nav_gain_check as gk
import nav_gain_restatement as gr
import nav_restatement as nr

IDS = [s.id for s in gc.SIZES]


def _seen(size_id, name, view, **wrong):
    size = gc.SIZE[size_id]
    case = gc.cases(size)[name]
    unknown, occupied = gr.classes(ff.export_map(case.lo), size.xsize)
    out, n = gr.seen(unknown, occupied, [view], case.R, **wrong)
    return out[0], int(n[0]), unknown, occupied


def test_ring_sizes_and_the_rays_steps():
    assert [len(gr.ring(R)) for R in (1, 2, 3, 8, 16, 32, 70, 128)] == [8, 12, 16, 48, 112, 188, 428, 788]
    for R in (1, 2, 3, 8, 31, 32, 33, 48, 128):
        ends = gr.ring(R)
        assert ends == sorted(ends) and max(max(abs(ex), abs(ey)) for ex, ey in ends) == R
        for ex, ey in ends:
            steps = gr.ray_steps(ex, ey)
            assert steps[-1] == (ex, ey) and len(steps) == max(abs(ex), abs(ey))
            prev = (0, 0)
            for s in steps:      # a step moves by at most one cell along each axis, and never stands still
                assert max(abs(s[0] - prev[0]), abs(s[1] - prev[1])) == 1
                prev = s
    assert gr.ray_steps(8, 1) == [(1, 0), (2, 0), (3, 0), (4, 1), (5, 1), (6, 1), (7, 1), (8, 1)]
    assert gr.ray_steps(8, 1, trunc=True)[3:7] == [(4, 0), (5, 0), (6, 0), (7, 0)]
    entered = set(s for e in gr.ring(16) for s in gr.ray_steps(*e))
    disc = sum(1 for x in range(-17, 18) for y in range(-17, 18) if 0 < x * x + y * y <= 16 * 16 + 16)
    assert 0.9 < len(entered) / disc <= 1.0       # the rays enter most of the disc's cells, not all: that is the rule


def test_host_ring_equals_the_restatement_for_every_range(pkg):
    """tbnav_nav_gain_rays needs no device."""
    import ctypes as C
    from rtn_amd.nav import gain_rays
    for R in range(1, gr.MAX_GAIN_RANGE + 1):
        got = gain_rays(R)
        assert got.dtype == np.int32 and got.tolist() == [list(e) for e in gr.ring(R)], R
    L, c = pkg.capi.lib(), pkg.capi
    n = C.c_int32(-5)
    for R in (0, -1, 129):
        assert L.tbnav_nav_gain_rays(R, None, 0, C.byref(n)) == c.ERR_INVALID_ARG and n.value == -5
    buf = np.zeros((48, 2), dtype=np.int32)
    assert L.tbnav_nav_gain_rays(8, buf.ctypes.data, 47, C.byref(n)) == c.ERR_INVALID_ARG and n.value == 48 and not buf.any()
    assert L.tbnav_nav_gain_rays(8, buf.ctypes.data, 48, None) == c.OK and buf.tolist() == [list(e) for e in gr.ring(8)]
    assert (c.NAV_MAX_GAIN_RANGE, c.NAV_MAX_GAIN_WEIGHT) == (gr.MAX_GAIN_RANGE, gr.MAX_GAIN_WEIGHT)


def test_the_ranked_start_cannot_overflow():
    """G20 as arithmetic: the most a gain can be, the most a start can be, and with G4's bound the most a cost-to-go can be."""
    most_gain = (2 * gr.MAX_GAIN_RANGE + 1) ** 2 - 1
    most_start = gr.MAX_GAIN_WEIGHT * most_gain
    g4 = nr.MAX_SIDE ** 2 * 14 * nr.MAX_COST
    assert (most_gain, most_start, g4) == (66048, 270532608, 3758096384)
    assert most_start + g4 == 4028628992 < nr.UNREACHED < 2 ** 32


@pytest.mark.parametrize("size_id", IDS)
def test_each_case_reaches_what_it_names(size_id):
    size = gc.SIZE[size_id]
    xs, last = size.xsize, size.xsize - 1
    table = gc.cases(size)
    get = lambda name: gk.expected(size_id, name)
    # distinct count: the rays of one viewpoint enter a cell more than once, and it counts once
    front, lab, seed, gain = get("open_half")
    assert np.array_equal(np.argwhere(seed)[:, 0], np.full(xs, 9)) and seed.sum() == xs
    out, n, unknown, _ = _seen(size_id, "open_half", (9, xs // 2))
    _, n_rays, _, _ = _seen(size_id, "open_half", (9, xs // 2), per_ray=True)
    assert n == gain[9, xs // 2] == out.sum() and n < n_rays and not out[:10].any() and out[10:].any()
    # the wall: nothing behind it, and not the wall itself
    front, lab, seed, gain = get("wall")
    out, n, _, occupied = _seen(size_id, "wall", (9, xs // 2))
    assert n > 0 and not out[12:].any() and out[10:12].any() and occupied[12].all()
    assert not _seen(size_id, "wall", (9, xs // 2), count_occ=True)[0][13:].any()
    # the diagonal wall: only the one unknown cell on the viewpoint's side
    front, lab, seed, gain = get("diag_wall")
    assert np.argwhere(seed).tolist() == [[8, 8]] and gain[8, 8] == 1
    assert _seen(size_id, "diag_wall", (8, 8), leaky=True)[1] > 10
    # grazing a corner: the diagonal's cells are seen past the one occupied cell beside its first step
    front, lab, seed, gain = get("corner_graze")
    out = _seen(size_id, "corner_graze", (10, 10))[0]
    assert np.argwhere(seed).tolist() == [[10, 10]] and gain[10, 10] == 4 and out[11, 11] and out[12, 12] and out[13, 13] and out[9, 10]
    # FREE and known-neither cells are passed through and never counted
    front, lab, seed, gain = get("pass_through")
    out = _seen(size_id, "pass_through", (10, 10))[0]
    assert np.argwhere(seed).tolist() == [[10, 10]] and gain[10, 10] == 4 and out[10, 15:18].all() and not out[10, 10:15].any()
    if xs > 32:
        front, lab, seed, gain = get("id0_half")
        assert seed[31].all() and seed.sum() == xs and (gain[31] > 0).all() and not (table["id0_half"].lo[32:] != 0).any()
    # the map's corners: the window is cut by the map on two sides, at R = 128 on all four
    for name in ("corners", "corners_R128"):
        front, lab, seed, gain = get(name)
        assert np.argwhere(seed).tolist() == [[0, 0], [last, last]] and gain[0, 0] == gain[last, last] > 0
    assert get("corners_R128")[3][0, 0] > get("corners")[3][0, 0] and table["corners_R128"].R == 128 > xs
    # viewpoints either side of the word and tile seams
    front, lab, seed, gain = get("seams")
    assert sorted(map(tuple, np.argwhere(seed).tolist())) == sorted(gc.seam_cells(xs)) and (gain[seed] > 0).all()
    if xs > 32:
        assert {y for _, y in gc.seam_cells(xs)} >= {0, 31, 32, last} and {x for x, _ in gc.seam_cells(xs)} >= {31, 32}
    front, lab, seed, gain = get("seam_bits")
    unknown = gr.classes(ff.export_map(table["seam_bits"].lo), xs)[0]
    assert set(np.argwhere(unknown)[:, 1].tolist()) == ({0, 31, 32, 63, last} if xs > 32 else {0, last}) and (gain[seed] > 0).all()
    for cell in np.argwhere(seed):
        out = gr.seen(unknown, np.zeros_like(unknown), [cell], table["seam_bits"].R)[0][0]
        assert set(np.argwhere(out)[:, 1].tolist()) <= {0, 31, 32, 63, last}
    # the ranges: the gain grows with R, and 32 and 33 are either side of the kernels' threshold
    gains = [int(get(f"ranges_R{R}")[3].sum()) for R in gc.RANGES]
    assert gains == sorted(gains) and gains[0] > 0 and get("ranges_R1")[2].sum() == 12
    assert gk.kernels(32) != gk.kernels(33) and 32 in gc.RANGES and 33 in gc.RANGES
    # the rounding step
    front, lab, seed, gain = get("rounding")
    assert gain[10, 10] == 3 and _seen(size_id, "rounding", (10, 10), trunc=True)[1] == 1
    # a cluster under the threshold is no viewpoint
    front, lab, seed, gain = get("min_cells_edge")
    assert front[5, 2:9].all() and not seed[5].any() and not gain[5].any() and seed[9, 2:10].all() and (gain[9, 2:10] > 0).all()
    assert gr.gain_list(lab, gain, fcs.MIN_CELLS)[0] == dict(root=(5, 2), gain_max=0, best=(-1, -1))
    assert gr.gain_list(lab, gain, fcs.MIN_CELLS)[1]["root"] == (9, 2) and gr.gain_list(lab, gain, fcs.MIN_CELLS)[1]["gain_max"] == gain.max()
    # a tie: the least index wins
    front, lab, seed, gain = get("tie")
    assert gain[4, 10] == gain[12, 10] == 2 and gain[20, 10] == 1
    assert gr.gain_info(gain, seed, 3) == dict(computed=True, range_cells=3, rays=16, viewpoints=3, gain_min=1, gain_max=2, best=(4, 10))
    # no seed
    front, lab, seed, gain = get("no_seed")
    assert not seed.any() and not gain.any()
    assert gr.gain_info(gain, seed, 8) == dict(computed=True, range_cells=8, rays=48, viewpoints=0, gain_min=0, gain_max=0, best=(-1, -1))
    assert ("nook" in table) == (size_id == gc.NOOK_SIZE)


@pytest.mark.parametrize("size_id", IDS)
def test_each_planted_error_changes_its_case(size_id):
    size = gc.SIZE[size_id]
    table = gc.cases(size)
    assert set(w for w, _ in gc.PLANTED) == set(gr.PLANTED)
    for wrong, name in gc.PLANTED:
        case = table[name]
        right = gk.expected(size_id, name)
        got = gr.find_gain(ff.export_map(case.lo), size.xsize, case.cost, None, case.min_cells, case.R, **{wrong: True})
        assert np.array_equal(got[2], right[2]) and not np.array_equal(got[3], right[3]), (wrong, name)


def test_weight_zero_and_equal_gains_are_the_plain_solve():
    size_id = "s64"
    case = gc.cases(gc.SIZE[size_id])["ranges_R8"]
    _, _, seed, gain = gk.expected(size_id, "ranges_R8")
    plain = ff.cost_to_go_goals(case.cost, ff.goal_cells(seed))
    assert np.array_equal(gk.expected_ranked(size_id, "ranges_R8", 0)[1], plain)
    flat = np.where(seed, 7, 0).astype(np.uint32)
    assert np.array_equal(gr.cost_to_go_ranked(case.cost, gr.start_values(flat, seed, 4096)), plain)
    assert not np.array_equal(gk.expected_ranked(size_id, "ranges_R8", 4096)[1], plain)
    start, d = gk.expected_ranked(size_id, "ranges_R8", 4096)
    assert (d[seed] <= start[seed]).all() and (d[seed] < start[seed]).any()       # a seed may be cheaper through another seed


def test_the_nook_and_the_doorway_flip_between_adjacent_weights():
    case = gc.nook()
    front, lab, seed, gain = gk.expected(gc.NOOK_SIZE, "nook")
    pocket = [(19, y) for y in range(gc.NOOK_POCKET_GAP[0], gc.NOOK_POCKET_GAP[1] + 1)]
    door = [(61, y) for y in range(gc.NOOK_DOOR_GAP[0], gc.NOOK_DOOR_GAP[1] + 1)]
    assert front.sum() == 26 == seed.sum() and sorted(map(tuple, np.argwhere(seed).tolist())) == pocket + door
    assert [int(gain[c]) for c in pocket] == [50] * 10
    assert [int(gain[c]) for c in door] == [348, 377, 386, 393, 393, 393, 393, 398, 398, 393, 393, 393, 393, 386, 377, 348]
    assert gr.gain_info(gain, seed, gc.NOOK_R)["best"] == (61, 51)
    ends = {}
    for w in gc.NOOK_ENDS:
        start, d = gk.expected_ranked(gc.NOOK_SIZE, "nook", w) if w in gc.WEIGHTS else (lambda s: (s, gr.cost_to_go_ranked(case.cost, s)))(gr.start_values(gain, seed, w))
        path = gr.path_ranked(case.cost, d, start, gc.NOOK_START)
        ends[w] = tuple(int(v) for v in path[-1])
        print("nook: weight", w, "ends at", ends[w], "d", int(d[ends[w]]), "start", int(start[ends[w]]), "cells", len(path))
        assert d[ends[w]] == start[ends[w]]
    assert ends == gc.NOOK_ENDS
    lo_w, hi_w = gc.NOOK_FLIP
    assert hi_w == lo_w + 1 and gc.in_pocket_gap(ends[lo_w]) and gc.in_door_gap(ends[hi_w])
    # the seed reached at weight 1 does not hold 0: the old stop rule walks past it
    start, d = gk.expected_ranked(gc.NOOK_SIZE, "nook", 1)
    assert d[ends[1]] == start[ends[1]] == 348
    with pytest.raises(RuntimeError):
        gr.path_ranked(case.cost, d, start, gc.NOOK_START, stop_at_zero=True)
    start0, d0 = gk.expected_ranked(gc.NOOK_SIZE, "nook", 0)       # ... and with all starts 0 the two rules are one
    assert np.array_equal(gr.path_ranked(case.cost, d0, start0, gc.NOOK_START, stop_at_zero=True), gr.path_ranked(case.cost, d0, start0, gc.NOOK_START))
    assert np.array_equal(gr.path_ranked(case.cost, d0, start0, gc.NOOK_START), nr.path(case.cost, d0, gc.NOOK_START)[0])


def test_gain_list_fields_on_a_case_with_several_clusters():
    front, lab, seed, gain = gk.expected("s64", "tie")
    assert gr.gain_list(lab, gain, 1) == [dict(root=(4, 10), gain_max=2, best=(4, 10)), dict(root=(12, 10), gain_max=2, best=(12, 10)),
                                          dict(root=(20, 10), gain_max=1, best=(20, 10))]


# ---- the exploration loop on the CPU, ranked ------------------------------------------------------------------------------------
def explore_cpu_ranked(start):
    """nav_frontier_cases.explore over the oracle's GridMapper with the ranked plan; also returns the exported map at the end."""
    import oracle_api as orc
    m = fcs.EXPLORE_MAP
    xs = m["xsize"]
    grid = orc.GridAPI("orc", grid=(m["res"], -m["half"], m["half"], -m["half"], m["half"]))
    visited = np.zeros((xs, xs), dtype=bool)

    def plan(cell):
        exported = grid.grid_map()
        occ = (exported.reshape(xs, xs).T == 100).astype(np.uint8)
        cost = fr.cost_from_occ(occ, m["res"], *fcs.EXPLORE_INFLATION)
        _, _, seed, gain = gr.find_gain(exported, xs, cost, visited, fcs.MIN_CELLS, gc.EXPLORE_GAIN_RANGE)
        if not seed.any():
            return None
        st = gr.start_values(gain, seed, gc.EXPLORE_GAIN_WEIGHT)
        return gr.path_ranked(cost, gr.cost_to_go_ranked(cost, st), st, cell)

    def mark(cell):
        visited[:] |= ff.disc(xs, xs, cell[0], cell[1], fcs.EXPLORE_MARK_RADIUS)

    run = fcs.explore(start, lambda scan, pose: grid.integrate_scan(scan, pose, esdf=False), plan, mark)
    run["exported"] = grid.grid_map()
    grid.close()
    return run


@functools.lru_cache(maxsize=None)
def explore_cpu_ranked_cached(start):
    return explore_cpu_ranked(start)


@pytest.mark.parametrize("k", range(len(fcs.EXPLORE_STARTS)))
def test_exploration_loop_with_the_ranked_plan_terminates(k):
    start = fcs.EXPLORE_STARTS[k]
    run = explore_cpu_ranked_cached(start)
    unknown, inside = fcs.explore_unknown_inside(run["exported"])
    print("ranked exploration from", start, ": iterations", len(run["cells"]), "marks", len(run["marks"]), "unknown cells inside", unknown, "of", inside)
    assert run["done"] and len(run["cells"]) <= fcs.EXPLORE_MAX_ITER
