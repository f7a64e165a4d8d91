"""The contract of the device ICP's correlative search (include/tbnav_icp.h, CORRELATIVE SEARCH) as tests/icp_search_restatement.py
states it, on the CPU: what the search is for (a guess outside the ICP's basin), when it stands aside (the truth outside its
window, degenerate scans), and the selection rule on ties and with slack.  The GPU tests compare the kernels with this
restatement bit for bit; these say that the restatement does what the header promises."""
import math

import numpy as np
import pytest

import icp_restatement as R
import icp_search_restatement as S
import oracle_api as orc
import rbpf_cases as rc

L = R.lds01()
POSES = ((0.0, 0.0, 0.0), (0.07, 0.02, 0.01))   # (theta, x, y)
OFFSET = (0.0, 0.65, 0.65)


def pair(room):
    rng = np.random.default_rng(1)
    s0 = orc.room_scan(POSES[0], walls=room, rng=rng)
    s1 = orc.room_scan(POSES[1], walls=room, rng=rng)
    return s0, s1, R.init_guess(POSES[1], POSES[0])


def _err(T, truth):
    return math.hypot(T[1] - truth[1], T[2] - truth[2]), abs(T[0] - truth[0])


@pytest.mark.parametrize("room", [rc.ROOM_BENCH, rc.ROOM_SURVEY])
def test_a_guess_outside_the_basin(room):
    s0, s1, truth = pair(room)
    guess = tuple(t + o for t, o in zip(truth, OFFSET))
    alone = R.match(s0, s1, L, guess)
    assert alone.ok and _err(alone.T, truth)[0] > 0.5          # the ICP alone: converged, and wrong
    res, info = S.match(s0, s1, L, guess, S.Params(lin_cells=14))
    assert info.accepted == 1 and info.quality >= 0.7 and info.candidates == 1 and info.at_edge == 0
    d, a = _err(info.T, truth)
    assert d <= 0.05 * math.sqrt(2.0) and a <= math.radians(1.0)   # within one cell and one angle step
    d, a = _err(res.T, truth)
    assert res.ok and d < 0.02 and a < 0.010, (d, a)


@pytest.mark.parametrize("room", [rc.ROOM_BENCH, rc.ROOM_SURVEY])
def test_the_default_window_does_not_contain_the_truth(room):
    s0, s1, truth = pair(room)
    guess = tuple(t + o for t, o in zip(truth, OFFSET))        # 13 cells off, the window is +-6
    res, info = S.match(s0, s1, L, guess)
    assert info.accepted == 0 and info.quality < 0.5
    alone = R.match(s0, s1, L, guess)
    assert (res.ok, res.T, res.iterations, res.mse) == (alone.ok, alone.T, alone.iterations, alone.mse)


def test_three_beams_tie_and_the_rank_rule_names_the_winner():
    s0, s1, truth = pair(rc.ROOM_BENCH)
    three = np.full(360, np.nan, dtype=np.float32)
    three[[10, 130, 250]] = s1[[10, 130, 250]]
    p = S.Params()
    sc = S.scores(s0, three, L, truth, p)
    info = S.search(s0, three, L, truth, p)
    assert info.points == 3 and info.score == 765 and info.candidates == 3 and int((sc == 765).sum()) == 3
    wl, wa, nl = p.lin_cells, p.ang_steps, 2 * p.lin_cells + 1
    ties = [(int(a - wa) ** 2 + int(y - wl) ** 2 + int(x - wl) ** 2, int((a * nl + y) * nl + x), int(a), int(y), int(x))
            for a, y, x in zip(*np.nonzero(sc == 765))]
    assert (info.ia, info.iy, info.ix) == min(ties)[2:]
    assert info.quality == 1.0 and info.accepted == 1


def test_degenerate_inputs_leave_the_guess():
    s0, s1, truth = pair(rc.ROOM_BENCH)
    none = np.full(360, np.inf, dtype=np.float32)
    guess = (0.3, -0.2, 0.1)
    for tgt, src, points in ((s0, none, 0), (none, s1, 360)):
        info = S.search(tgt, src, L, guess)
        assert info.accepted == 0 and info.points == points and info.T == guess and info.score == 0
        assert info.candidates == 41 * 13 * 13 and info.quality == 0.0
    assert S.search(none, none, L, guess).points == 0


def test_a_minimal_window_is_one_candidate():
    s0, s1, truth = pair(rc.ROOM_BENCH)
    p = S.Params(lin_cells=0, ang_steps=0)
    sc = S.scores(s0, s1, L, truth, p)
    info = S.search(s0, s1, L, truth, p)
    assert sc.shape == (1, 1, 1) and info.candidates == 1 and info.at_edge == 0 and info.T == truth
    assert info.score == int(sc[0, 0, 0]) and info.accepted == 1


def test_a_small_table_scores_the_points_outside_it_zero():
    s0, s1, truth = pair(rc.ROOM_BENCH)                       # walls at 2.0 .. 2.2 m: all outside a +-1 m table
    p = S.Params(half_extent=1.0)
    assert S.side(p) == 40 and not S.table(s0, L, p).any()
    assert S.search(s0, s1, L, truth, p).score == 0
    s0, s1, truth = pair(rc.ROOM_SMALL)                       # walls at 1.3 .. 1.7 m: near beams inside, far ones outside
    near = orc.room_scan(POSES[0], walls=(-0.9, 0.8, -0.7, 1.4), rng=np.random.default_rng(4))
    near1 = orc.room_scan(POSES[1], walls=(-0.9, 0.8, -0.7, 1.4), rng=np.random.default_rng(5))
    tab = S.table(near, L, p)
    assert tab.any() and tab[:, 0].any() and not tab[0].any()   # the wall at x = -0.9 is cut by the table's edge, y = -0.7 is inside
    info = S.search(near, near1, L, truth, p)
    assert 0 < info.score < 255 * info.points
    full = S.search(near, near1, L, truth, S.Params())
    assert full.score > info.score                            # the points outside the small table score 0


def test_stamp_and_sigma():
    st = S.stamp(S.Params())
    assert st.shape == (7, 7) and st[3, 3] == 255 and st[3, 4] == 155 and st[0, 0] == 0 and np.array_equal(st, st.T)
    wide = S.stamp(S.Params(stamp_cells=8, sigma=0.2))
    assert wide.shape == (17, 17) and wide.min() > 0 and wide[8, 8] == 255
    assert S.stamp(S.Params(stamp_cells=1, sigma=0.01))[0, 1] == 0
    s0, s1, truth = pair(rc.ROOM_BENCH)
    q = [S.search(s0, s1, L, truth, S.Params(stamp_cells=k, sigma=s)).quality for k, s in ((1, 0.02), (3, 0.05), (8, 0.2))]
    assert q[0] < q[1] < q[2]                                   # a wider stamp forgives more


def test_slack_never_moves_the_choice_away_from_the_guess():
    s0, s1, truth = pair(rc.ROOM_BENCH)
    for guess in (truth, (truth[0] + 0.1, truth[1] + 0.12, truth[2] - 0.08)):
        sc = S.scores(s0, s1, L, guess)
        base = S.search(s0, s1, L, guess, S.Params(), scores=sc)
        D0 = (base.ia - 20) ** 2 + (base.iy - 6) ** 2 + (base.ix - 6) ** 2
        last = 1
        for slack in (1, 32, 64, 256, 1023):
            info = S.search(s0, s1, L, guess, S.Params(slack_q10=slack), scores=sc)
            assert (info.ia - 20) ** 2 + (info.iy - 6) ** 2 + (info.ix - 6) ** 2 <= D0, slack
            assert info.candidates >= last and info.score <= base.score
            last = info.candidates
        assert (info.ia, info.iy, info.ix) == (20, 6, 6) or last < sc.size   # slack 1023 / 1024 takes nearly everything


def test_limits():
    assert S.valid(S.Params()) and S.valid(S.Params(lin_cells=16, ang_steps=90)) and S.side(S.Params()) == 160
    assert not S.valid(S.Params(resolution=0.04)) and S.valid(S.Params(resolution=0.04, half_extent=3.0))   # 200 + 12 > 208
    for bad in (dict(stamp_cells=0), dict(stamp_cells=9), dict(lin_cells=-1), dict(lin_cells=17), dict(ang_steps=91), dict(slack_q10=1024),
                dict(resolution=0.0), dict(sigma=-1.0), dict(half_extent=float("nan")), dict(half_extent=4.45, lin_cells=16)):
        assert not S.valid(S.Params(**bad)), bad
