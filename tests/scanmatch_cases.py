"""The case table of the RBPF scan matcher (csrc/rbpf_propose.hip: rbpf_scanmatch, with the lookups it makes through csrc/rbpf_lookup.hpp's
lookup_code / nearest_code_query_body and its per-beam cell cache).  Plain data and the two host expressions that decide which lookup path a case takes,
restated: the window half-width and the LDS bitmap slice (csrc/rbpf_plan.hpp: lookup_half_cells, sampling_spread, plan_propose).  tests/test_scanmatch_cases.py proves the table on the CPU with the
oracle alone (the matcher really moves, leaves the slice / the window, wraps, hits the move cap where a case says so, and no
decision of any matcher call is nearer than 5e-10 to going the other way); tests/test_rbpf_scanmatch_gpu.py runs it on the device,
nothing injected.

A run: the filters start at `start - inc` and every scan s moves them by the odometry increment to `start + s * inc`, the pose the
scan was taken from — so the particles' frame is the world's, and walls, map borders, slices and windows are where the table says.
The guess handed to the filter on scan s is that increment plus `err[s]` (theta, x, y: body frame, as T_icp is).
"""
import math
from collections import namedtuple

import numpy as np

import oracle_api as orc
import rbpf_cases as rc

OFF = (math.radians(1.5), 0.03, -0.02)     # the bad guess of tests/test_rbpf_gpu.py's matcher test
ZERO = (0.0, 0.0, 0.0)
DEFAULT_STEPS = (0.05, 0.05, 5)
MAX_MOVES = 64                              # tbnav_rbpf_set_scan_matching's round limit, PF::sm_max_moves
SAMPLE_RANGE = (1e-10, 1e-8, 1e-8)          # slam.launch's, as default_params / pf_params set them
MOTION_NOISE = (1e-10, 1e-10, 1e-10)
MARGIN_MIN = 5e-10                          # the least decision margin every matcher call of every case must keep

ROOM_CORRIDOR = (-8.0, 7.95, -1.0, 1.0)     # 13.95 m ahead of x = -6: the forward beams end just inside range_max = 14 m
ROOM_EDGE = (-1.7, 1.7, -1.7, 1.7)          # 6 cells inside the border of a +-2 m map

# id; map half-extent / resolution -> cells; room; range_max; Trs (theta, x, y); start pose; true increment per scan; guess error per
# scan; (lstep, astep, iterations); N, k, beams; device distance-field mode; the scans the matcher runs on; seed of the range noise;
# window = rows / columns of the oracle's maps that get storage (None: all); resample_at = scan before which weights are skewed;
# valid = {scan: number of beams left valid, or {beam: range in metres} — a hand-made scan of exactly those beams}; odometry = "true": the twist u handed over is the true increment's, "guess": the guess's
# (wheel odometry that is as short as the guess: u only sizes the window); slice = (margin, occ_half) the case claims for the LDS slice (query mode);
# half_cells = the window half-width the case claims per scan (window mode); expect = what else the case claims (see the CPU test).
Case = namedtuple("Case", "id half res cells room range_max trs start inc err steps N k beams mode match_on seed window resample_at "
                          "valid odometry slice half_cells expect")


def _case(id, half=3.0, res=0.05, room=rc.ROOM_SMALL, range_max=3.5, trs=ZERO, start=ZERO, inc=(0.04, 0.03, 0.02),
          err=(ZERO, ZERO, ZERO, OFF, OFF), steps=DEFAULT_STEPS, N=8, k=10, beams=360, mode="query", match_on=None, seed=5, window=None,
          resample_at=None, valid=None, odometry="true", slice=None, half_cells=None, expect=None):
    match_on = tuple(range(len(err))) if match_on is None else match_on
    return Case(id, half, res, int(math.ceil(2 * half / res)), room, range_max, trs, start, inc, tuple(err), steps, N, k, beams, mode,
                match_on, seed, window, resample_at, valid or {}, odometry, slice, half_cells, expect or {})


_SMALL_WIN = (290, 410, 290, 410)           # +-3 m round the centre of the 700-cell map
_MODES = dict(half=3.0, N=24, k=20, err=(ZERO, ZERO, ZERO, OFF, OFF, OFF), expect=dict(empty_at=(0,), moves_at=(3, 4, 5)))
_BIG = dict(half=17.5, err=(ZERO, ZERO, OFF, OFF), window=_SMALL_WIN, expect=dict(empty_at=(0,), moves_at=(2, 3)))
_STEP = dict(expect=dict(empty_at=(0,), moves_at=(3, 4)))

CASES = (
    # the existing small-room run, nothing injected, matcher on from scan 0 (an empty map), in the three modes that hold the exact field
    _case("modes-query", mode="query", slice=(48, 121), **_MODES),
    _case("modes-window", mode="window", half_cells=(120,) * 6, **_MODES),
    _case("modes-full", mode="full", half_cells=(120,) * 6, **_MODES),
    # the LDS slice of the bitmap: margin 48, 16, 0 and dropped, through range_max on one 700-cell map — the first multiple of 100 cells
    # on which these four values of range_max take the four regimes (on 600 cells the clamp to the map's 10 words keeps margin 48 at 12 m)
    _case("slice-m48", range_max=3.5, slice=(48, 121), **_BIG),
    _case("slice-m16", range_max=12.0, slice=(16, 259), **_BIG),
    _case("slice-m0", range_max=14.0, slice=(0, 283), **_BIG),
    _case("slice-dropped", range_max=16.0, slice=(None, 0), **_BIG),
    # leaving the slice: margin 0, the wall 13.85 / 13.80 m ahead and the guess 0.4 / 0.35 m (8 / 7 cells) short of it along the
    # corridor — the matched pose's forward end points lie beyond the slice's last row, and on the way the 7 x 7 look straddles it.
    # 1080 beams, so that the far wall is dense (a cell every 1.6 columns, in rows 508 / 509: it stands on a cell border), and on
    # scan 3 the slice's last row is 508.  (This does not hold `clear`: a wall that dense always has a cell inside the slice at
    # least as near as any outside.  slice-clear below does.)
    _case("slice-leave", half=17.5, room=ROOM_CORRIDOR, range_max=14.0, start=(0.0, -6.0, 0.0), inc=(0.0, 0.05, 0.0),
          err=(ZERO, ZERO, (0.0, -0.4, 0.0), (0.0, -0.35, 0.0)), beams=1080, window=(180, 520, 320, 380), slice=(0, 283),
          expect=dict(empty_at=(0,), moves_at=(2, 3), leaves_slice_at=(2, 3))),
    # `clear` at the slice's last row, on a hand-made map of two cells ahead of the robot (which backs away 3 cells per scan, so that
    # earlier beams reach farther than the slice): scan 0 marks A = (516, 350) with beam 0, scan 1 marks B = (508, 352) with beam 1
    # (1/3 degree to the left: its ray shares no cell with the others near the end), and on scan 2 the slice ends at row
    # R1 = 232 + 283 = 515 — A is one row outside — while the only beam ends on L = (512, 350).  d2(L, A) = 16, d2(L, B) = 20: the
    # slice alone answers 20, which `clear` = R1 - 512 + 1 = 4 refuses (20 > 16), so the global bitmap answers 16.  A `clear` one too
    # large accepts the 20.  Steps far below a cell: the matched pose is the first guess, and its score is that one lookup.
    _case("slice-clear", half=17.5, room=ROOM_CORRIDOR, range_max=14.0, start=(0.0, -5.575, 0.035), inc=(0.0, -0.15, 0.0),
          err=(ZERO, ZERO, ZERO), steps=(0.003, 0.0001, 3), beams=1080, match_on=(2,),
          valid={0: {0: 13.90}, 1: {1: 13.65}, 2: {0: 13.99}}, window=(200, 540, 330, 370), slice=(0, 283),
          expect=dict(clear_at=2, outside=(516, 350), inside=(508, 352), lookup=(512, 350), last_row=515)),
    # ... and its mirror image (the beams that look backwards, 540 and 541 of 1080; every position mirrored) for the slice's FIRST
    # row: R0 = 467 - 283 = 184, A one row before it
    _case("slice-clear-first-row", half=17.5, room=ROOM_CORRIDOR, range_max=14.0, start=(0.0, 5.575, -0.035), inc=(0.0, 0.15, 0.0),
          err=(ZERO, ZERO, ZERO), steps=(0.003, 0.0001, 3), beams=1080, match_on=(2,),
          valid={0: {540: 13.90}, 1: {541: 13.65}, 2: {540: 13.99}}, window=(160, 500, 330, 370), slice=(0, 283),
          expect=dict(clear_at=2, outside=(183, 349), inside=(191, 347), lookup=(187, 349), first_row=184)),
    # leaving the window: 0.5 m per scan towards a wall that comes into range (3.45 m) on scan 2, whose guess says 0.1 m
    _case("window-leave", half=10.0, room=rc.ROOM_SURVEY, mode="window", start=(0.0, -1.45, 0.0), inc=(0.0, 0.5, 0.0),
          err=(ZERO, ZERO, (0.0, -0.4, 0.0), ZERO), odometry="guess", half_cells=(148, 148, 140, 148),
          expect=dict(empty_at=(0,), moves_at=(2,), leaves_unwidened_window_at=(2,))),
    # far walk: 0.8 m off with 1 cm steps — 64 rounds are not enough, the run ends at the cap with halvings to spare
    _case("move-cap", err=(ZERO, ZERO, ZERO, (0.0, -0.8, 0.0)), steps=(0.01, 0.05, 5), slice=(48, 121),
          expect=dict(empty_at=(0,), moves_at=(3,), cap_at=(3,))),
    # steps: a step of four cells (every round moves a beam's end point out of any 2 x 2 neighbourhood: the cache's slots are replaced),
    # steps far below a cell halved 32 times (trials on identical cells: the 1 + 1e-9 rule must refuse to move), and a small budget
    _case("steps-coarse", steps=(0.2, 0.1, 1), err=(ZERO, ZERO, ZERO, (0.0, -0.5, 0.4), (0.0, 0.45, -0.5)), slice=(48, 121),
          expect=dict(empty_at=(0,), moves_at=(3, 4))),
    _case("steps-fine", steps=(0.003, 0.002, 32), slice=(48, 121), expect=dict(empty_at=(0,), moves_at=(3, 4), ties_at=(3, 4))),
    _case("steps-short", steps=(0.01, 0.01, 3), slice=(48, 121), **_STEP),
    # a trial angle crosses +-pi on every round
    _case("wrap", start=(3.12, 0.0, 0.0), inc=(0.004, 0.03, 0.02), slice=(48, 121), expect=dict(empty_at=(0,), moves_at=(3, 4), wraps_at=(1, 2, 3, 4))),
    _case("sensor-offset", trs=(0.3, 0.05, -0.02), slice=(48, 121), **_STEP),
    _case("after-resample", N=16, resample_at=2, slice=(48, 121), expect=dict(empty_at=(0,), moves_at=(3, 4), resampled_at=(2,))),
    _case("ragged", err=(ZERO, ZERO, OFF, OFF, OFF, OFF), valid={2: 0, 3: 1, 4: 65}, slice=(48, 121),
          expect=dict(empty_at=(0,), moves_at=(4, 5), still_at=(2,))),
    _case("beams-1080", beams=1080, err=(ZERO, ZERO, OFF, OFF), slice=(48, 121), expect=dict(empty_at=(0,), moves_at=(2, 3))),
    # out of world: the +x wall at 1.7 m on a +-2 m map, the guess 0.27 m too far along x — its own end points stay inside (1.97 m), the
    # +x trial's do not (2.02 m).  Statuses only.
    _case("out-of-world", half=2.0, room=ROOM_EDGE, inc=(0.0, 0.03, 0.02), err=(ZERO, ZERO, ZERO, (0.0, 0.27, 0.0)), slice=(48, 121),
          expect=dict(empty_at=(0,), out_of_world_at=3)),
)
CASE = {c.id: c for c in CASES}
MODE_CASES = ("modes-query", "modes-window", "modes-full")


# ---- the two host expressions, restated (csrc/rbpf_plan.hpp: lookup_half_cells, plan_propose) ------------------------------------------------------------------
def _spread():
    return 8.0 * math.sqrt(max(SAMPLE_RANGE[1], SAMPLE_RANGE[2], MOTION_NOISE[1], MOTION_NOISE[2]))


def half_cells(case, guess, u, matching, widened=True):
    """Half-width, in cells, of the window the stored field is refreshed in before a scan (window mode; full mode and a window wider
    than the map: the whole map).  widened=False: without the matcher's travel, the rule before this table existed."""
    move = max(math.hypot(guess[1], guess[2]), abs(u[1]))
    half = float(np.float32(case.range_max)) + math.hypot(case.trs[1], case.trs[2]) + move + _spread()
    if matching and widened:
        half += MAX_MOVES * case.steps[0]
    hc = int(math.ceil(half / case.res)) + 3
    return case.cells if (case.mode == "full" or hc > case.cells) else hc


def slice_regime(case):
    """(margin, occ_half) of the LDS slice of the occupancy bitmap (query mode): the reach of a lookup plus a margin of 48, 16 or 0
    cells, the first that fits 48 KB; (None, 0): no slice."""
    words = (case.cells + 63) // 64
    reach = int(math.ceil((float(np.float32(case.range_max)) + _spread()) / case.res)) + 2
    for margin in (48, 16, 0):
        half = reach + margin
        rows, nw = min(case.cells, 2 * half + 1), min(words, (2 * half + 1 + 63) // 64 + 1)
        if rows * nw * 8 + rows * 4 <= 48 * 1024:
            return margin, half
    return None, 0


def cell_of(case, x, y):
    """grid_mapper.cpp:852-887 for a point inside the world."""
    return int(math.floor((x + case.half) / case.res)), int(math.floor((y + case.half) / case.res))


def first_guess_sensor_cells(case, poses, guess):
    """Cell of the sensor at T(pose) * guess * Trs for every particle pose (theta, x, y): the centre of the matcher's LDS slice."""
    out = []
    for p in poses:
        s = rc.compose(rc.compose(p, np.asarray(guess)), np.asarray(case.trs))
        out.append(cell_of(case, s[1], s[2]))
    return np.array(out)


# ---- a run --------------------------------------------------------------------------------------------------------------------------
def params(case):
    """Keyword arguments common to orc.pf_params and rtn_amd.rbpf.default_params."""
    lo = tuple(a - b for a, b in zip(case.start, case.inc))
    return dict(N=case.N, k=case.k, map_min=-case.half, map_max=case.half, pose0=lo, beam_delta_deg=360.0 / case.beams,
                range_max=case.range_max, Trs=list(case.trs), resolution=case.res)


Scan = namedtuple("Scan", "s scan u cur prev guess normals matching weights")


def scans(case):
    """The inputs of every scan of the case, in order."""
    n = len(case.err)
    steps, poses = rc.trajectory(n, inc=case.inc, start=case.start)
    rng = np.random.default_rng(case.seed)
    for s, (prev, cur, t_icp, u) in enumerate(steps):
        scan = orc.room_scan(poses[s], n_beams=case.beams, beam_delta_deg=360.0 / case.beams, walls=case.room, rng=rng,
                             range_max=case.range_max)
        if s in case.valid:       # every `stride`-th beam (or the beams named) stays, the rest fall below range_min
            keep = np.zeros(scan.size, dtype=bool)
            nv = case.valid[s]
            if isinstance(nv, dict):
                for b, r in nv.items():
                    keep[b] = True; scan[b] = r
            elif nv:
                keep[(np.arange(nv) * (scan.size // nv) + 7) % scan.size] = True
            scan = np.where(keep, scan, np.float32(0.01)).astype(np.float32)
        weights = None
        if case.resample_at == s:   # tests/test_rbpf_field_gpu.py::_free_run's forced resample
            weights = np.full(case.N, 0.2 / case.N); weights[3] += 0.5; weights[case.N // 2] += 0.3; weights /= weights.sum()
        normals = orc.normal_stream(900 + s, case.N * (3 * case.k + 3) + 1, 0.0, 1.0)
        guess = np.asarray(t_icp) + np.asarray(case.err[s])
        if case.odometry == "guess":
            u = np.array([guess[0], np.hypot(guess[1], guess[2]), 0.0])
        yield Scan(s, scan, u, cur, prev, guess, normals, s in case.match_on, weights)


def oracle_filter(case):
    return orc.PfAPI(orc.pf_params(**params(case)), exact_field=True, window=case.window)


def oracle_step(pf, case, sc):
    """One scan on the oracle: the trace of PfAPI.slam."""
    pf.set_scan_matching(sc.matching, *case.steps)
    if sc.weights is not None:
        pf.set_particles(w=sc.weights)
    return pf.slam(sc.scan, sc.u, sc.cur, sc.prev, True, sc.guess, sc.normals)
