"""Fifty seeded random cases of the device ICP's correlative search (csrc/icp_search.hip) against its numpy restatement
(tests/icp_search_restatement.py): window, resolution, table size, stamp, slack, acceptance threshold, beam count, invalid beams,
laser offset and guess are drawn; the whole score volume and the result are equal on every one.  No case is skipped: the draw
only ever produces parameters inside the header's limits (a draw outside them is shrunk, and the test says how many were)."""
import numpy as np
import pytest

import icp_restatement as R
import icp_search_restatement as S
import oracle_api as orc
import rbpf_cases as rc

pytestmark = pytest.mark.gpu

N_CASES = 50
ROOMS = (rc.ROOM_BENCH, rc.ROOM_SURVEY, rc.ROOM_SMALL, (-0.9, 0.8, -0.7, 1.4))
BEAMS = (1, 2, 3, 7, 64, 255, 256, 257, 360, 511, 513, 720, 1080)
FIELDS = ("resolution", "half_extent", "sigma", "ang_step", "min_quality", "stamp_cells", "lin_cells", "ang_steps", "slack_q10")
BUDGET = 6e6   # table lookups of the restatement per case: keeps a case at some tens of milliseconds


def draw(seed):
    rng = np.random.default_rng(1000 + seed)
    n_beams = int(rng.choice(BEAMS))
    room = ROOMS[int(rng.integers(len(ROOMS)))]
    p1 = (float(rng.normal(0, 0.1)), float(rng.normal(0, 0.1)), float(rng.normal(0, 0.1)))
    dd = 360.0 / n_beams
    s0 = orc.room_scan((0.0, 0.0, 0.0), n_beams=n_beams, beam_delta_deg=dd, walls=room, rng=rng)
    s1 = orc.room_scan(p1, n_beams=n_beams, beam_delta_deg=dd, walls=room, rng=rng)
    for sc in (s0, s1):
        bad = rng.random(n_beams) < float(rng.choice((0.0, 0.05, 0.5)))
        sc[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.05, 5.0], dtype=np.float32), size=int(bad.sum()))
    kw = dict(resolution=float(rng.choice((0.05, 0.04, 0.1, 0.025))), half_extent=float(rng.choice((1.0, 2.0, 3.0, 4.0))),
              sigma=float(rng.choice((0.02, 0.05, 0.1, 0.2))), ang_step=float(rng.choice((np.pi / 180.0, 0.01, 0.05))),
              min_quality=float(rng.choice((0.0, 0.5, 0.9))), stamp_cells=int(rng.integers(1, 9)), lin_cells=int(rng.integers(0, 17)),
              ang_steps=int(rng.integers(0, 9)), slack_q10=int(rng.choice((0, 0, 0, 1, 32, 64, 300, 1023))))
    shrunk = 0
    while not S.valid(S.Params(**kw)):          # the table does not fit: halve it
        kw["half_extent"] /= 2.0
        shrunk = 1
    while (2 * kw["ang_steps"] + 1) * (2 * kw["lin_cells"] + 1) ** 2 * n_beams > BUDGET and kw["ang_steps"] > 0:
        kw["ang_steps"] -= 1
    Trs = (0.0, 0.0, 0.0) if rng.random() < 0.5 else (float(rng.normal(0, 0.3)), float(rng.normal(0, 0.1)), float(rng.normal(0, 0.1)))
    truth = R.init_guess(p1, (0.0, 0.0, 0.0))
    guess = (truth[0] + float(rng.normal(0, 0.1)), truth[1] + float(rng.normal(0, 0.3)), truth[2] + float(rng.normal(0, 0.3)))
    return s0, s1, dd, S.Params(**kw), Trs, guess, shrunk


def test_fifty_random_cases_equal_the_restatement(gpu_pkg):
    from rtn_amd import icp
    accepted = slow = shrunk = 0
    for seed in range(N_CASES):
        s0, s1, dd, sp, Trs, guess, sh = draw(seed)
        shrunk += sh
        p = icp.default_params(beam_delta_deg=dd, Trs=Trs)
        a = icp.ScanAlignment(p, search={f: getattr(sp, f) for f in FIELDS})
        L = R.Laser(p.beam_min, p.beam_max, p.beam_delta, p.range_min, p.range_max)
        want_sc = S.scores(s0, s1, L, guess, sp, Trs)
        want = S.search(s0, s1, L, guess, sp, Trs, scores=want_sc)
        acc, T, info, sc = a.searchScores(guess, s0, s1)
        assert np.array_equal(sc, want_sc), (seed, sp)
        for f in ("T", "quality", "score", "points", "candidates", "ia", "iy", "ix", "at_edge", "accepted", "searched"):
            assert info[f] == getattr(want, f), (seed, f, info, want, sp)
        assert np.array_equal(a.searchTable(s0), S.table(s0, L, sp, Trs)), (seed, sp)
        accepted += want.accepted
        slow += sp.half_extent < 3.0
        a.close()
    # the draw reaches both outcomes and the small tables whose borders the window crosses
    assert 0 < accepted < N_CASES and slow > 5, (accepted, slow, shrunk)
