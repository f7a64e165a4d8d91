"""The wide second stage of the correlative search (include/tbnav_icp.h, CORRELATIVE SEARCH, items W1-W8) as
tests/icp_search_wide_restatement.py states it, on the CPU: guesses 1.7-2.5 m off, which every window of the first stage rejects,
are found by a window of 48 cells and the ICP from there ends on the truth; 32 cells reject the furthest of them; the wide volume
contains the first stage's; W3's truth table; the corridor case of W6; the limits of W1.  The GPU tests compare the kernels with
this restatement with ==; these say that the restatement does what the header promises."""
import math

import numpy as np
import pytest

import icp_line_restatement as LR
import icp_restatement as R
import icp_search_restatement as S
import icp_search_shape_restatement as F
import icp_search_wide_restatement as W
import oracle_api as orc
import rbpf_cases as rc

L = R.lds01()
P1 = (0.07, 0.02, 0.01)
GUESSES = [(0.0, 1.3, -1.1), (0.35, 1.6, 0.9), (-0.5, -2.0, 1.5)]
ROOMS = [("bench", rc.ROOM_BENCH), ("survey", rc.ROOM_SURVEY)]
CORRIDOR = (-50, 50, -1, 1)

_clouds = {}


def clouds(name, room):
    """360 beams, scans at (0, 0, 0) and P1, seed 1, 1 cm noise -> (s0, s1, their clouds, the true transform)"""
    if name not in _clouds:
        rng = np.random.default_rng(1)
        s0 = orc.room_scan((0.0, 0.0, 0.0), walls=room, rng=rng)
        s1 = orc.room_scan(P1, walls=room, rng=rng)
        _clouds[name] = (s0, s1, R.cloud(s0, L)[0], R.cloud(s1, L)[0], R.init_guess(P1, (0.0, 0.0, 0.0)))
    return _clouds[name]


def _off(T, truth, p):
    """(angular steps, cells in x, cells in y) between T and the truth, rounded"""
    return (round((T[0] - truth[0]) / p.ang_step), round((T[1] - truth[1]) / p.resolution), round((T[2] - truth[2]) / p.resolution))


@pytest.mark.parametrize("room", ROOMS, ids=[r[0] for r in ROOMS])
@pytest.mark.parametrize("off", GUESSES, ids=[str(g) for g in GUESSES])
def test_the_guess_table(room, off):
    s0, s1, tgt, src, truth = clouds(*room)
    guess = tuple(t + o for t, o in zip(truth, off))
    for wl in (6, 16):
        first = S.search_clouds(tgt, src, guess, S.Params(lin_cells=wl))
        assert S.valid(S.Params(lin_cells=wl)) and not first.accepted, (wl, first)
    wp = W.WideParams(lin_cells=48, ang_steps=30)
    out = W.search_clouds(tgt, src, guess, S.Params(), wp)
    print(room[0], off, "first q %.3f, wide q %.3f, off by %s" % (out.first.quality, out.info.quality, _off(out.info.T, truth, S.Params())))
    assert out.ran == 1 and out.first.searched == 1 and not out.first.accepted
    assert out.info.accepted and max(abs(v) for v in _off(out.info.T, truth, S.Params())) <= 1, out.info
    for icp in (R.match, LR.match):
        res, _ = W.match(s0, s1, L, guess, S.Params(), wp, icp=icp, outcome=out)
        d, a = math.hypot(res.T[1] - truth[1], res.T[2] - truth[2]), abs(res.T[0] - truth[0])
        print("   ", icp.__module__, "ends %.1f mm and %.1f mrad off" % (1e3 * d, 1e3 * a))
        assert res.ok and d < 0.01 and a < 0.01, (icp.__module__, res)


@pytest.mark.parametrize("room", ROOMS, ids=[r[0] for r in ROOMS])
def test_32_cells_reject_the_furthest_guess(room):
    s0, s1, tgt, src, truth = clouds(*room)
    guess = tuple(t + o for t, o in zip(truth, GUESSES[2]))
    out = W.search_clouds(tgt, src, guess, S.Params(), W.WideParams(lin_cells=32, ang_steps=30))
    assert out.ran == 1 and not out.info.accepted and out.info.at_edge == 1, out.info
    res, _ = W.match(s0, s1, L, guess, outcome=out)
    assert res == R.match(s0, s1, L, guess)                      # a rejected outcome: the ICP from the guess, unchanged


def test_the_wide_volume_contains_the_first_stages():
    s0, s1, tgt, src, truth = clouds(*ROOMS[0])
    guess = (truth[0] + 0.03, truth[1] + 0.4, truth[2] - 0.2)
    p = S.Params(ang_steps=2)
    for wp in (W.WideParams(lin_cells=20, ang_steps=3), W.WideParams(lin_cells=6, ang_steps=2)):
        first = S.scores_of_clouds(tgt, src, guess, p)
        wide = S.scores_of_clouds(tgt, src, guess, W.window(p, wp))
        a, w = wp.ang_steps - p.ang_steps, wp.lin_cells - p.lin_cells
        na, nl = 2 * p.ang_steps + 1, 2 * p.lin_cells + 1
        assert wide.shape == (2 * wp.ang_steps + 1,) + (2 * wp.lin_cells + 1,) * 2
        assert np.array_equal(wide[a:a + na, w:w + nl, w:w + nl], first) and first.any()
        assert int(wide.max()) >= int(first.max())


FIRST = S.Params(ang_steps=2)
WIDE = W.WideParams(lin_cells=14, ang_steps=2)
# the first stage's fate -> the guess's offset from the truth: well inside its window, exactly on its border, outside it
FATES = {"accepted": (0.0, 0.1, -0.05), "accepted at the edge": (0.0, 0.3, 0.0), "rejected": (0.0, 0.55, 0.2)}


@pytest.mark.parametrize("fate", list(FATES))
def test_w3_truth_table(fate):
    s0, s1, tgt, src, truth = clouds(*ROOMS[0])
    guess = tuple(t + o for t, o in zip(truth, FATES[fate]))
    first = S.search_clouds(tgt, src, guess, FIRST)
    assert (bool(first.accepted), bool(first.at_edge)) == {"accepted": (True, False), "accepted at the edge": (True, True),
                                                          "rejected": (False, True)}[fate], first
    wide = S.search_clouds(tgt, src, guess, W.window(FIRST, WIDE))
    assert wide.accepted and not wide.at_edge
    want_ran = {"accepted": (0, 0, 1), "accepted at the edge": (0, 1, 1), "rejected": (1, 1, 1)}[fate]
    for when, ran in zip((W.ON_REJECT, W.ON_REJECT_OR_EDGE, W.ALWAYS), want_ran):
        assert W.runs(first, when) == bool(ran)
        out = W.search_clouds(tgt, src, guess, FIRST, WIDE.with_(when=when))
        assert out.ran == ran, (fate, when)
        assert out.first == (W.NOT_SEARCHED if when == W.ALWAYS else first)
        assert out.info == (wide if ran else first), (fate, when)
        res, _ = W.match(s0, s1, L, guess, FIRST, WIDE.with_(when=when), outcome=out)
        assert res == R.match(s0, s1, L, out.info.T)
    assert W.NOT_SEARCHED.searched == 0 and W.NOT_SEARCHED.T == (0.0, 0.0, 0.0) and W.NOT_SEARCHED.score == 0


def _corridor_pair(seed=3):
    rng = np.random.default_rng(seed)
    s0 = orc.room_scan((0.0, 0.0, 0.0), walls=CORRIDOR, rng=rng)
    s1 = orc.room_scan((0.0, 0.10, 0.0), walls=CORRIDOR, rng=rng)
    return s0, s1, (0.0, 0.10, 0.0)


@pytest.mark.parametrize("guess,lin", [((0.45, 0.10, 0.15), 32), ((0.45, 0.10, 0.6), 32), ((0.45, 0.10, 0.6), 64)])
def test_the_corridor_case_of_w6(guess, lin):
    s0, s1, truth = _corridor_pair()
    wp = W.WideParams(lin_cells=lin, ang_steps=30)
    raw = W.search(s0, s1, L, guess, S.Params(), wp)
    assert raw.ran == 1 and not raw.first.accepted and raw.info.accepted
    assert abs(raw.info.T[1]) < 0.026, raw.info                  # the raw choice overlays the scans: the 10 cm along it are gone
    out = W.search(s0, s1, L, guess, S.Params(), wp, shape_params=F.ShapeParams())
    sh = out.shape
    print(guess, lin, "first q %.3f, l1 %.1f, l2 %.3f, T %s" % (out.first.quality, sh.l1, sh.l2, out.info.T))
    assert sh.kind == 1 and sh.computed == 1 and sh.T_raw == raw.info.T and sh.l1 > 100 and sh.l2 < 0.5, sh
    assert abs(out.info.T[1] - guess[1]) < 0.005 and out.info.T[0] == raw.info.T[0], out.info   # along the corridor: the guess's
    shaped, _ = W.match(s0, s1, L, guess, S.Params(), wp, icp=LR.match, outcome=out)
    plain, _ = W.match(s0, s1, L, guess, S.Params(), wp, icp=LR.match, outcome=raw)
    d_shaped, d_plain = abs(shaped.T[1] - truth[1]), abs(plain.T[1] - truth[1])
    print("    the line metric ends %.1f mm off along the corridor from the shaped pose, %.1f mm from the raw one" % (1e3 * d_shaped, 1e3 * d_plain))
    assert shaped.ok and plain.ok and d_shaped < d_plain and abs(shaped.T[2] - truth[2]) < 0.005


def test_the_limits_of_w1():
    assert W.WideParams() == W.WideParams(48, 45, W.ON_REJECT) and W.valid(W.WideParams())
    assert (W.MAX_LIN, W.MAX_ANG, W.MAX_TABLE) == (64, 180, 176)
    assert W.valid(W.WideParams(64, 180, W.ALWAYS)) and W.valid(W.WideParams(6, 20)) and W.valid(W.WideParams(1, 0), S.Params(lin_cells=1, ang_steps=0))
    for bad in (dict(lin_cells=0), dict(lin_cells=65), dict(ang_steps=-1), dict(ang_steps=181), dict(when=-1), dict(when=3),
                dict(lin_cells=5), dict(ang_steps=19)):
        assert not W.valid(W.WideParams().with_(**bad)), bad
    assert W.valid(W.WideParams(), S.Params(half_extent=4.4)) and S.side(S.Params(half_extent=4.4)) == 176
    assert not W.valid(W.WideParams(), S.Params(half_extent=4.45, lin_cells=6)) and S.side(S.Params(half_extent=4.45)) == 178
    assert not W.valid(W.WideParams(lin_cells=15), S.Params(lin_cells=16)) and W.valid(W.WideParams(lin_cells=16), S.Params(lin_cells=16))
    assert not W.valid(W.WideParams(ang_steps=45), S.Params(ang_steps=46))
    # the first stage's own limits are untouched: 17 cells are still outside them
    assert not S.valid(S.Params(lin_cells=17)) and S.MAX_LIN == 16
