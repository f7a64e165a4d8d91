"""The shape of the score volume (include/tbnav_icp.h, CORRELATIVE SEARCH, items F1-F6) as tests/icp_search_shape_restatement.py
states it, on the CPU: in a corridor the search alone erases the motion along it and the shape keeps it (the line metric then
ends millimetres from the truth); the correction across the corridor survives; rooms are compact and stay bit for bit what the
search alone gives; and the rule's edges on hand-written score arrays.  The GPU tests compare the kernel with this restatement
with ==; these say that the restatement does what the header promises."""
import math

import numpy as np
import pytest

import icp_line_restatement as LR
import icp_restatement as R
import icp_search_restatement as S
import icp_search_shape_restatement as F
import oracle_api as orc
import rbpf_cases as rc

L = R.lds01()
CORRIDOR = (-50, 50, -1, 1)
P, SP = S.Params(), F.ShapeParams()


def corridor_pair(seed, p0=(0.0, 0.0, 0.0), p1=(0.0, 0.10, 0.0)):
    """two scans 10 cm apart along the corridor, 1 cm range noise -> (s0, s1, the true transform in scan 0's frame)"""
    rng = np.random.default_rng(seed)
    s0 = orc.room_scan(p0, walls=CORRIDOR, rng=rng)
    s1 = orc.room_scan(p1, walls=CORRIDOR, rng=rng)
    truth = tuple(float(v) for v in rc.compose(rc.inverse(np.array(p0)), np.array(p1)))
    return s0, s1, truth


def _along_across(T, truth, axis):
    dx, dy = T[1] - truth[1], T[2] - truth[2]
    return abs((dx * axis[0]) + (dy * axis[1])), abs((dy * axis[0]) - (dx * axis[1]))


@pytest.mark.parametrize("seed", [3, 4])
def test_axis_aligned_corridor_keeps_the_guess_along_it(seed):
    s0, s1, truth = corridor_pair(seed)
    plain, info0 = S.match(s0, s1, L, truth, icp=LR.match)
    assert info0.accepted and abs(info0.T[1] - truth[1]) == pytest.approx(0.10)   # the search overlays the scans: two cells back
    assert plain.ok and abs(plain.T[1] - truth[1]) > 0.07, plain.T
    res, info, sh = F.match(s0, s1, L, truth, icp=LR.match)
    assert sh.computed == 1 and sh.kind == 1 and abs(sh.ey) < 0.05 and sh.l1 > 10 and sh.l2 < 0.5, sh
    assert sh.T_raw == info0.T and info.T[0] == info0.T[0]
    along = ((info.T[1] - truth[1]) * sh.ex) + ((info.T[2] - truth[2]) * sh.ey)
    assert abs(along) < 1e-9, along
    assert res.ok and abs(res.T[1] - truth[1]) < 0.005, res.T
    for f in ("quality", "score", "points", "candidates", "ia", "iy", "ix", "at_edge", "accepted"):
        assert getattr(info, f) == getattr(info0, f), f


def test_corridor_at_a_heading():
    s0, s1, truth = corridor_pair(6, (0.6, 0.0, 0.0), (0.6, 0.10, 0.0))
    axis = (math.cos(-0.6), math.sin(-0.6))                     # the corridor in the scan's frame
    plain, _ = S.match(s0, s1, L, truth, icp=LR.match)
    assert plain.ok and _along_across(plain.T, truth, axis)[0] > 0.20, plain.T
    res, info, sh = F.match(s0, s1, L, truth, icp=LR.match)
    assert sh.kind == 1 and abs(math.atan2(sh.ey, sh.ex) - (-0.60)) < 0.03, sh
    assert res.ok and math.hypot(res.T[1] - truth[1], res.T[2] - truth[2]) < 0.01, res.T


def test_the_correction_across_the_corridor_is_kept():
    s0, s1, truth = corridor_pair(3)
    guess = (0.05, 0.10, 0.15)                                  # right along the corridor, 15 cm and 0.05 rad off across it
    res, info, sh = F.match(s0, s1, L, guess, icp=LR.match)
    assert sh.kind == 1 and info.accepted
    assert abs(info.T[2] - truth[2]) < 0.05 and abs(info.T[1] - guess[1]) < 0.005   # one cell across, the guess along
    assert res.ok and abs(res.T[1] - truth[1]) < 0.005 and abs(res.T[2] - truth[2]) < 0.005, res.T
    plain, _ = S.match(s0, s1, L, guess, icp=LR.match)
    alone = LR.match(s0, s1, L, guess)
    assert abs(plain.T[1] - truth[1]) > 0.07 and abs(alone.T[1] - truth[1]) > 0.02   # neither of the two does it alone


def _room_pairs():
    for room, inc in ((rc.ROOM_BENCH, rc.TRAJ_BENCH), (rc.ROOM_SURVEY, rc.TRAJ_SURVEY)):
        steps, poses = rc.trajectory(8, inc=inc)
        rng = np.random.default_rng(1)
        scans = [orc.room_scan(q, walls=room, rng=rng) for q in poses]
        for s in range(1, 8):
            yield scans[s - 1], scans[s], R.init_guess(poses[s], poses[s - 1]), P
    rng = np.random.default_rng(1)
    s0 = orc.room_scan((0.0, 0.0, 0.0), walls=rc.ROOM_BENCH, rng=rng)
    s1 = orc.room_scan((0.07, 0.02, 0.01), walls=rc.ROOM_BENCH, rng=rng)
    yield s0, s1, (0.07, 0.02 + 0.65, 0.01 + 0.65), S.Params(lin_cells=14)


def test_rooms_are_compact_and_unchanged():
    worst, n = 0.0, 0
    for s0, s1, guess, p in _room_pairs():
        sc = S.scores(s0, s1, L, guess, p)
        plain = S.search(s0, s1, L, guess, p, scores=sc)
        info, sh = F.search(s0, s1, L, guess, p, SP, scores=sc)
        assert sh.kind == 0 and sh.computed == 1 and info == plain and sh.T_raw == plain.T, (guess, sh)
        assert plain.accepted
        worst = max(worst, sh.l1)
        n += 1
    assert n == 15 and worst < 1.0, worst


def _info(score, iy, ix, wl, ia=0):
    return S.Info((0.0, float(ix - wl) * 0.05, float(iy - wl) * 0.05), 0.9, score, 100, 1, ia, iy, ix, 0, 1)


def test_rule_edges_on_hand_written_volumes():
    p2, p3 = S.Params(lin_cells=2, ang_steps=0), S.Params(lin_cells=3, ang_steps=0)
    # drop_q10 = 0: floor = best, nothing is above it
    vol = np.full((1, 5, 5), 1000, dtype=np.uint32)
    sh = F.shape(vol, _info(1000, 2, 2, 2), p2, F.ShapeParams(drop_q10=0))
    assert (sh.S0, sh.cells, sh.kind, sh.computed) == (0, 0, 0, 1) and (sh.l1, sh.l2, sh.ex, sh.ey) == (0.0, 0.0, 0.0, 0.0)
    # best < 4 with the default drop: best * 256 >> 10 == 0
    vol = np.full((1, 5, 5), 3, dtype=np.uint32)
    assert F.shape(vol, _info(3, 2, 2, 2), p2).S0 == 0
    vol = np.zeros((1, 5, 5), dtype=np.uint32)
    assert F.shape(vol, _info(0, 2, 2, 2), p2).S0 == 0
    # wl = 0: one candidate, no spread
    sh = F.shape(np.full((1, 1, 1), 4000, dtype=np.uint32), _info(4000, 0, 0, 0), S.Params(lin_cells=0, ang_steps=0))
    assert (sh.S0, sh.cells, sh.kind) == (1000, 1, 0) and (sh.l1, sh.l2) == (0.0, 0.0) and (sh.ex, sh.ey) == (1.0, 0.0)
    # a uniform +-2 window: variance exactly 2.0 in both axes, not > 2.0
    sh = F.shape(np.full((1, 5, 5), 1024, dtype=np.uint32) + np.zeros((1, 5, 5), dtype=np.uint32), _info(1024, 2, 2, 2), p2,
                 F.ShapeParams(drop_q10=512))
    assert sh.cells == 25 and (sh.l1, sh.l2) == (2.0, 2.0) and sh.kind == 0 and (sh.ex, sh.ey) == (1.0, 0.0)   # b == 0 and hd == 0
    # a uniform +-3 window: variance 4.0 in both, nothing is observed
    sh = F.shape(np.full((1, 7, 7), 1024, dtype=np.uint32), _info(1024, 3, 5, 3), p3, F.ShapeParams(drop_q10=512))
    assert (sh.l1, sh.l2) == (4.0, 4.0) and sh.kind == 2 and (sh.dx, sh.dy) == (0.0, 0.0)
    info = _info(1024, 3, 5, 3)
    assert F.shaped(info, sh, (0.1, 0.2, 0.3), p3).T == (0.0, 0.2, 0.3)
    # a ridge along y: hd < 0, the other form of the eigenvector
    vol = np.zeros((1, 7, 7), dtype=np.uint32)
    vol[0, :, 3] = 1024
    sh = F.shape(vol, _info(1024, 1, 3, 3), p3, F.ShapeParams(drop_q10=512))
    assert (sh.l1, sh.l2) == (4.0, 0.0) and (sh.ex, sh.ey) == (0.0, 1.0) and sh.kind == 1 and (sh.dx, sh.dy) == (0.0, 0.0)
    # a ridge along x: hd > 0; the chosen cell's offset across it stays
    vol = np.zeros((1, 7, 7), dtype=np.uint32)
    vol[0, 4, :] = 1024
    sh = F.shape(vol, _info(1024, 4, 1, 3), p3, F.ShapeParams(drop_q10=512))
    assert (sh.l1, sh.l2) == (4.0, 0.0) and (sh.ex, sh.ey) == (1.0, 0.0) and sh.kind == 1 and (sh.dx, sh.dy) == (0.0, 1.0)
    # a diagonal ridge: b != 0, hd == 0
    vol = np.zeros((1, 7, 7), dtype=np.uint32)
    vol[0, np.arange(7), np.arange(7)] = 1024
    sh = F.shape(vol, _info(1024, 3, 3, 3), p3, F.ShapeParams(drop_q10=512))
    assert sh.kind == 1 and sh.ex == sh.ey == 1.0 / math.sqrt(2.0) and sh.l1 == 8.0 and sh.l2 == 0.0
    # only the chosen angle's slice counts
    vol = np.zeros((3, 7, 7), dtype=np.uint32)
    vol[0] = 1000
    vol[1, 3, 3] = 1024
    sh = F.shape(vol, _info(1024, 3, 3, 3, ia=1), S.Params(lin_cells=3, ang_steps=1), F.ShapeParams(drop_q10=512))
    assert (sh.cells, sh.kind, sh.S0) == (1, 0, 512)
    # the sums are the exact integers of F3
    vol = np.zeros((1, 5, 5), dtype=np.uint32)
    vol[0, 0, 4], vol[0, 2, 2] = 900, 1000                      # w = 150, 250 at (dx, dy) = (2, -2), (0, 0)
    sh = F.shape(vol, _info(1000, 2, 2, 2), p2)
    assert (sh.S0, sh.Sx, sh.Sy, sh.Sxx, sh.Sxy, sh.Syy, sh.cells) == (400, 300, -300, 600, -600, 600, 2)


def test_parameter_limits():
    assert F.valid(F.ShapeParams()) and F.ShapeParams() == F.ShapeParams(256, 2.0)
    assert F.valid(F.ShapeParams(0, 1e-9)) and F.valid(F.ShapeParams(1023, 1e9))
    for bad in (dict(drop_q10=-1), dict(drop_q10=1024), dict(flat_cells2=0.0), dict(flat_cells2=-2.0), dict(flat_cells2=float("nan")),
                dict(flat_cells2=float("inf"))):
        assert not F.valid(F.ShapeParams(**bad)), bad
