"""30 drawn cases of the wide second stage of the correlative search (include/tbnav_icp.h, items W1-W8; csrc/icp_search_wide.hip)
against tests/icp_search_wide_restatement.py with ==: the hook's whole score volume and record, and the outcome of the stateless
search under the drawn policy.  The seed is fixed; W is drawn from 1..64 and A from 0..3, and the beam count, the room, the
guess's offset, Trs, the slack, the first stage's window and `when` are drawn as well."""
import numpy as np
import pytest

import icp_restatement as R
import icp_search_restatement as S
import icp_search_wide_restatement as W
import oracle_api as orc
import rbpf_cases as rc

pytestmark = pytest.mark.gpu

N_CASES = 30
ROOMS = (rc.ROOM_BENCH, rc.ROOM_SURVEY, (-0.9, 0.8, -0.7, 1.4))
FIELDS = ("resolution", "half_extent", "sigma", "ang_step", "min_quality", "stamp_cells", "lin_cells", "ang_steps", "slack_q10")


def _draw(i):
    rng = np.random.default_rng(9000 + i)
    lin, ang = int(rng.integers(1, 65)), int(rng.integers(0, 4))
    n_beams = int(rng.choice([90, 255, 360, 361, 720, 1080]))
    room = ROOMS[int(rng.integers(0, len(ROOMS)))]
    reach = lin * 0.05
    off = (float(rng.uniform(-0.05, 0.05)), float(rng.uniform(-1.1, 1.1)) * reach, float(rng.uniform(-1.1, 1.1)) * reach)
    Trs = (0.0, 0.0, 0.0) if rng.random() < 0.5 else (float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-0.1, 0.1)), float(rng.uniform(-0.1, 0.1)))
    slack = int(rng.choice([0, 0, 0, 16, 200]))
    sp = S.Params(lin_cells=int(rng.integers(0, min(lin, 16) + 1)), ang_steps=int(rng.integers(0, ang + 1)), slack_q10=slack,
                  half_extent=float(rng.choice([4.0, 4.0, 2.0, 1.0, 4.4])))
    wp = W.WideParams(lin, ang, int(rng.integers(0, 3)))
    p1 = (float(rng.uniform(-0.1, 0.1)), float(rng.uniform(-0.1, 0.1)), float(rng.uniform(-0.1, 0.1)))
    return n_beams, room, off, Trs, sp, wp, p1, rng


@pytest.mark.parametrize("i", range(N_CASES))
def test_drawn_case(gpu_pkg, i):
    from rtn_amd import icp
    n_beams, room, off, Trs, sp, wp, p1, rng = _draw(i)
    assert S.valid(sp) and W.valid(wp, sp)
    dd = 360.0 / n_beams
    s0 = orc.room_scan((0.0, 0.0, 0.0), n_beams=n_beams, beam_delta_deg=dd, walls=room, rng=rng)
    s1 = orc.room_scan(p1, n_beams=n_beams, beam_delta_deg=dd, walls=room, rng=rng)
    truth = R.init_guess(p1, (0.0, 0.0, 0.0))
    guess = tuple(t + o for t, o in zip(truth, off))
    p = icp.default_params(beam_delta_deg=dd, Trs=Trs)
    a = icp.ScanAlignment(p, search={f: getattr(sp, f) for f in FIELDS}, wide=dict(lin_cells=wp.lin_cells, ang_steps=wp.ang_steps, when=wp.when))
    L = R.Laser(p.beam_min, p.beam_max, p.beam_delta, p.range_min, p.range_max)
    want, want_sc = W.wide_scores(s0, s1, L, guess, sp, wp, Trs)
    acc, T, info, sc = a.searchWideScores(guess, s0, s1)
    assert np.array_equal(sc, want_sc), (i, sp, wp)
    for f in ("T", "quality", "score", "points", "candidates", "ia", "iy", "ix", "at_edge", "accepted", "searched"):
        assert info[f] == getattr(want, f), (i, f, info, want)
    # the outcome under the drawn policy: the wide stage's record where W3 makes it run, the first stage's otherwise
    first = None if wp.when == W.ALWAYS else S.search(s0, s1, L, guess, sp, Trs)
    ran = wp.when == W.ALWAYS or W.runs(first, wp.when)
    outcome = want if ran else first
    acc, T, info = a.search(guess, s0, s1)
    for f in ("T", "quality", "score", "points", "candidates", "ia", "iy", "ix", "at_edge", "accepted", "searched"):
        assert info[f] == getattr(outcome, f), (i, f, ran, info, outcome)
    # and in front of the ICP the same record, with the first stage's beside it
    a.pclICP(guess, s0, s1)
    lw, last = a.lastSearchWide(), a.lastSearch()
    assert lw["ran"] == int(ran) and last == info, (i, lw, last)
    if first is not None:
        for f in ("T", "score", "ia", "iy", "ix", "accepted", "at_edge", "searched"):
            assert lw["first"][f] == getattr(first, f), (i, f)
    else:
        assert lw["first"]["searched"] == 0 and lw["first"]["score"] == 0
    a.close()
