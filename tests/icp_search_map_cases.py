"""The case table of the map search (include/tbnav_icp.h, MAP SEARCH M1-M9; csrc/icp_search_map.hip): small maps, tables, origins,
occupancies and parameters at which icp_search_table_from_occ and the route round it can still go wrong.  tests/
test_icp_search_map_cases.py proves on the CPU, on the restatement, that each case reaches what its `reaches` names;
tests/test_icp_search_map_gpu.py holds the device to the restatement with == on every one.

Maps: side 64 (2 x 2 tiles of the filter's pool), 96 (3 x 3), 80 (a ragged last tile) at 0.05 m, side 24 at 0.5 m (nav_from_map_cases'
sizes), and 400 x 400 for the behaviour cases.  Tables: n = 32 (one table tile), 34 and 48 (a ragged table tile), 160 (the default).

BEHAVIOUR (measured on the restatement; 1 cm range noise; maps drawn by the oracle's GridMapper from 12 scans of ROOM_BENCH, 658
occupied cells, and 20 scans of ROOM_SURVEY, 692; the scan is taken at BEHAVIOUR truth; asserted in test_icp_search_map_cases.py):
  map     guess off by (rad, m, m)   window (cells, steps)   quality  accepted  error (angle steps, cells x, cells y)
  bench   (0, 0, 0)                  +-6, +-20               0.995    1         (-1.0, 0, 0)
  bench   (0.1, 0.2, -0.15)          +-6, +-20               0.992    1         (0.73, 0, 0)
  bench   (0.3, 0.5, 0.4)            +-6, +-20               0.299    0         at the window's edge
  bench   (0.3, 0.5, 0.4)            +-14, +-20              0.996    1         (-0.81, 0, 0)
  bench   (0.25, -0.65, 0.65)        +-6, +-20               0.182    0         at the window's edge
  bench   (0.25, -0.65, 0.65)        +-14, +-20              0.996    1         (-0.68, 0, 0)
  survey  (0.6, 1.6, 0.9)            +-48, +-45, wide stage  0.872    1         (-0.62, 0, 0)
  survey  (-0.7, -2.0, 1.5)          +-48, +-45, wide stage  0.984    1         (0.89, 0, 0)   the scan taken at (0.2, 1.2, -0.9)
  survey  (-0.7, -2.0, 1.5)          +-48, +-45, wide stage  0.417    0         (0.89, 0, 0)   the scan taken at BEHAVIOUR truth: FOUND to the
                                                                                cell and REJECTED.  The table stands round the GUESS's cell
                                                                                (M3), here 2.5 m from the truth: the walls at x = 3 and
                                                                                y = -2.5 lie outside it, their points add nothing (M9) and
                                                                                the quality, which divides by all valid points, stays low.
  bench   the other room's scan      +-14, +-20              0.402    0         -
  bench   the other room's scan      +-48, +-45, wide stage  0.557    1         RECORDED, NOT ASSERTED: min_quality = 0.5 does not separate
                                                                                a wrong room from a true match over a wide window (M9)
BEHAVIOUR_RECORD holds the qualities; the CPU test fails when one is no longer what it measures."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import icp_restatement as R
import icp_search_map_restatement as M
import icp_search_restatement as S
import icp_search_shape_restatement as F
import icp_search_wide_restatement as W
import nav_from_map_cases as fc
import rbpf_cases as rc

LASER = R.lds01()


def geom(size_id) -> M.Geom:
    s = fc.SIZE[size_id]
    return M.Geom(-s.half, -s.half, s.res, s.xsize)


def guess(size_id, cx, cy, th=0.1, fx=0.37, fy=0.61):
    """a world pose inside map cell (cx, cy)"""
    g = geom(size_id)
    T = (th, g.xmin + (cx + fx) * g.resolution, g.ymin + (cy + fy) * g.resolution)
    assert M.cell_of(g, T[1], T[2]) == (cx, cy)
    return T


def scan_wavy(n_beams=360, lo=0.25, amp=0.3, seed=1):
    """ranges that put points inside and outside a table of +-0.8 m, some beams invalid"""
    i = np.arange(n_beams)
    r = lo + amp * (1.0 + np.sin(0.05 * i * 360.0 / max(n_beams, 1))) + np.random.default_rng(seed).random(n_beams) * 0.05
    r[::17] = 0.05          # below range_min
    return r.astype(np.float32)


# parameter sets; half_extent is never a whole number of cells in the small ones (M3's E')
P32 = S.Params(half_extent=0.79, sigma=0.1, lin_cells=6, ang_steps=2)          # n = 32
P34 = P32.with_(half_extent=0.84)                                                # n = 34
P48 = P32.with_(half_extent=1.19)                                                # n = 48
P160 = S.Params(sigma=0.1, ang_steps=2)                                          # n = 160, the default table
P50CM = S.Params(resolution=0.5, half_extent=7.9, sigma=0.7, stamp_cells=3, lin_cells=6, ang_steps=2)   # n = 32 at 0.5 m
for _p, _n in ((P32, 32), (P34, 34), (P48, 48), (P160, 160), (P50CM, 32)):
    assert S.side(_p) == _n and S.valid(_p)


@dataclass
class Case:
    name: str
    size_id: str
    occ: object                  # () -> uint8 [side][side]
    p: S.Params
    T: tuple
    scan: np.ndarray
    reaches: str
    check: object                # (case, Result) -> bool: the proof that the case reaches what it names
    wp: object = None            # W.WideParams: the handle has the wide stage on
    shape: object = None         # F.ShapeParams: ... the shape
    plants: tuple = ()           # planted errors this case is known to expose

    @property
    def geom(self):
        return geom(self.size_id)


def _cells(size_id, cells):
    return lambda: fc._occ(fc.SIZE[size_id], cells)


def _pattern(size_id, name):
    return lambda: fc.patterns(fc.SIZE[size_id])[name]


def _tab_at(res, case, mx, my):
    """the table byte at map cell (mx, my), or None outside the table"""
    fr = M.frame(case.geom, case.T, case.p)
    ix, iy = mx - (fr.cx - fr.h2), my - (fr.cy - fr.h2)
    n = S.side(case.p)
    return int(res.table[iy, ix]) if 0 <= ix < n and 0 <= iy < n else None


def _stamp_probe(k):
    """one occupied cell: the stamp stands round it, square not disc, nothing at k + 1"""
    def check(case, res):
        (mx, my), = np.argwhere(case.occ())
        v = M.stamp_by_d2(case.p)
        ok = _tab_at(res, case, mx, my) == 255 and res.tgt_points == 1
        ok &= _tab_at(res, case, mx + k, my) == v[k * k] > 0 and _tab_at(res, case, mx, my + k) == v[k * k]
        ok &= _tab_at(res, case, mx + k, my + k) == v[2 * k * k] > 0 and _tab_at(res, case, mx - k, my - k) == v[2 * k * k]
        ok &= _tab_at(res, case, mx + k + 1, my) == 0 and _tab_at(res, case, mx, my + k + 1) == 0 and _tab_at(res, case, mx, my - k - 1) == 0
        return bool(ok)
    return check


def _origin_probe(bit_x, bit_y):
    def check(case, res):
        fr = M.frame(case.geom, case.T, case.p)
        return (fr.cx - fr.h2) % 32 == bit_x and (fr.cy - fr.h2) % 32 == bit_y and res.tgt_points > 0 and res.outcome.info.score > 0
    return check


def _any_score(case, res):
    return res.tgt_points > 0 and res.outcome.info.score > 0


def build():
    cases = []
    add = cases.append
    wav = scan_wavy()
    # ---- origins: cx - h2 at bit offsets 0, 1, 31, 32 of a map word, rows likewise across the tile seam (n = 32, h2 = 16) ----
    for bx, by in ((0, 0), (1, 31), (31, 1), (32, 32)):
        add(Case(f"origin_{bx}_{by}", "s96", _pattern("s96", "random"), P32, guess("s96", 16 + bx, 16 + by), wav,
                 f"cx - h2 = {bx}, cy - h2 = {by}: bit offsets within a word and rows across a seam", _origin_probe(bx % 32, by % 32),
                 plants=("origin", "transposed") if (bx, by) == (1, 31) else ()))
    add(Case("corner_low", "s64", _pattern("s64", "corners"), P32, guess("s64", 0, 0), wav,
             "the guess in cell (0, 0): the window hangs over the map's corner", lambda c, r: M.frame(c.geom, c.T, c.p).cx == 0 and r.tgt_points == 1,
             plants=("outside",)))
    add(Case("corner_high", "s80", _pattern("s80", "corners"), P32, guess("s80", 79, 79), wav,
             "the guess in cell (side - 1, side - 1) of a map with a ragged last tile", lambda c, r: r.tgt_points == 1 and _tab_at(r, c, 79, 79) == 255))
    add(Case("inside_one_tile", "s96", _pattern("s96", "one_tile"), S.Params(half_extent=0.39, sigma=0.1, lin_cells=2, ang_steps=1), guess("s96", 48, 48),
             scan_wavy(lo=0.13, amp=0.1), "a window (n = 16) wholly inside map tile (1, 1), untouched tiles beside it",
             lambda c, r: S.side(c.p) == 16 and r.tgt_points > 0 and not c.occ()[:32].any()))
    # ---- occupancy ----
    for k, sig in ((1, 0.1), (3, 0.1), (8, 0.3)):
        add(Case(f"stamp_k{k}", "s64", _cells("s64", ((30, 33),)), P32.with_(stamp_cells=k, sigma=sig), guess("s64", 31, 31), wav,
                 f"one cell at offsets (k, 0), (0, k), (k, k) inside the stamp and (k + 1, 0), (0, k + 1) outside, k = {k}", _stamp_probe(k),
                 plants=("disc",) if k == 3 else ()))
    # (3, 0) against (2, 2) round probe (20, 20): d2 9 against 8; (4, 0) against (3, 3) round probe (40, 40): d2 16 against 18, where the
    # Chebyshev distance says 4 against 3
    def metric_check(case, res):
        v = M.stamp_by_d2(case.p)
        return _tab_at(res, case, 20, 20) == v[8] != v[9] and _tab_at(res, case, 40, 40) == v[16] != v[18]
    add(Case("metric", "s64", _cells("s64", ((23, 20), (22, 22), (44, 40), (43, 43))), P48.with_(stamp_cells=4, sigma=0.15), guess("s64", 32, 32), wav,
             "a nearest pair that a wrong metric gets wrong: (3, 0) / (2, 2), and (4, 0) / (3, 3)", metric_check, plants=("chebyshev",)))
    def tie_check(case, res):
        return _tab_at(res, case, 30, 30) == M.stamp_by_d2(case.p)[5] and res.tgt_points == 2
    add(Case("equal_d2", "s64", _cells("s64", ((31, 32), (28, 29))), P32, guess("s64", 30, 30), wav, "two cells at equal d2 = 5 either side", tie_check))
    # cells just outside the n x n window (n = 32 round cell (32, 32): map cells 16 .. 47): at distance 1 and k they stamp in, at k + 1
    # they do not, and none is counted
    def rim_check(case, res):
        v = M.stamp_by_d2(case.p)
        return (res.tgt_points == 0 and _tab_at(res, case, 16, 20) == v[1] and _tab_at(res, case, 30, 47) == v[9] and
                _tab_at(res, case, 47, 40) == 0 and _tab_at(res, case, 15, 20) is None and res.table.any())
    add(Case("rim", "s64", _cells("s64", ((15, 20), (30, 50), (51, 40))), P32, guess("s64", 32, 32), wav,
             "occupied cells outside the window at distance 1 and k (they stamp in) and k + 1 (not), none in tgt_points", rim_check))
    for name in ("full_row", "full_col", "full_map", "seam_rows", "seam_cols"):
        at = dict(seam_rows=(32, 16), seam_cols=(16, 32)).get(name, (40, 41))
        add(Case(name, "s80", _pattern("s80", name), P34, guess("s80", *at), wav, f"nav_from_map_cases' {name} under a ragged table tile (n = 34)",
                 _any_score, plants=("E",) if name == "full_map" else ()))
    add(Case("untouched_beside", "s96", _pattern("s96", "one_tile"), P48, guess("s96", 40, 40), wav,
             "an untouched tile (id 0) beside a written one, n = 48", lambda c, r: _any_score(c, r) and not c.occ()[:32].any()))
    add(Case("empty", "s64", _pattern("s64", "empty"), P32, guess("s64", 20, 40), wav, "no occupied cell: the table is zero and nothing is accepted",
             lambda c, r: r.tgt_points == 0 and not r.table.any() and r.outcome.info.accepted == 0))
    # ---- parameters ----
    add(Case("wl0_wa0", "s64", _pattern("s64", "random"), P32.with_(lin_cells=0, ang_steps=0), guess("s64", 30, 33), wav, "wl = 0, wa = 0: one candidate",
             lambda c, r: r.scores.shape == (1, 1, 1)))
    add(Case("wl16_wa20", "s64", _pattern("s64", "random"), P32.with_(lin_cells=16, ang_steps=20), guess("s64", 30, 33), wav,
             "wl = 16, wa = 20 (5 translations a thread)", lambda c, r: r.scores.shape == (41, 33, 33) and r.scores.any()))
    add(Case("slack", "s64", _pattern("s64", "full_col"), P32.with_(slack_q10=300), guess("s64", 30, 33), wav, "slack_q10 > 0: the second pass",
             lambda c, r: r.outcome.info.candidates > 1))
    add(Case("tiny_sigma", "s64", _pattern("s64", "random"), P32.with_(sigma=0.005, stamp_cells=2), guess("s64", 30, 33), wav,
             "a sigma so small that the stamp is one cell", lambda c, r: set(np.unique(r.table)) == {0, 255} and M.stamp_by_d2(c.p)[1] == 0))
    add(Case("beams_1", "s64", _pattern("s64", "full_map"), P32, guess("s64", 30, 33), np.array([0.4], dtype=np.float32), "1 beam",
             lambda c, r: r.outcome.info.points == 1 and r.outcome.info.score == 255))
    add(Case("beams_7", "s64", _pattern("s64", "full_map"), P32, guess("s64", 30, 33), scan_wavy(7)[::-1].copy(), "7 beams", lambda c, r: 0 < r.outcome.info.points <= 7))
    def slow_check(case, res):
        return M.slow_list_points(case.scan_cloud, M.frame(case.geom, case.T, case.p), case.p) > 0 and res.scores.any()
    add(Case("slow_list", "s64", _pattern("s64", "full_map"), P32, guess("s64", 30, 33), scan_wavy(lo=0.5, amp=0.2),
             "source points whose base cell is outside the table (the bounds-tested list)", slow_check))
    add(Case("default_table", "s96", _pattern("s96", "random"), P160, guess("s96", 50, 47), scan_wavy(lo=0.4, amp=1.2),
             "n = 160: 5 x 5 table tiles over a 96-cell map, the window over every side of it", lambda c, r: r.table.shape == (160, 160) and _any_score(c, r)))
    add(Case("cells_50cm", "r20", _pattern("r20", "random"), P50CM, guess("r20", 11, 13), scan_wavy(lo=0.5, amp=1.4), "0.5 m cells, side 24",
             lambda c, r: c.geom.side == 24 and _any_score(c, r)))
    # ---- shape and wide stage on the map's table ----
    add(Case("shape", "s80", _pattern("s80", "full_col"), P34, guess("s80", 40, 41), wav, "F1-F6 on the map's table: a full column is flat along it",
             lambda c, r: r.outcome.shape is not None and r.outcome.shape.computed == 1 and r.outcome.shape.kind >= 1, shape=F.ShapeParams()))
    add(Case("wide_reject", "s64", _pattern("s64", "random"), P32.with_(min_quality=0.99), guess("s64", 30, 33), wav,
             "the wide stage runs behind a rejected first stage (W = 20, A = 4: 2 x 2 tiles)", lambda c, r: r.outcome.ran == 1 and r.outcome.first.accepted == 0,
             wp=W.WideParams(20, 4, W.ON_REJECT)))
    add(Case("wide_idle", "s64", _pattern("s64", "full_map"), P32.with_(min_quality=0.01), guess("s64", 30, 33), wav,
             "the wide stage is on and does not run", lambda c, r: r.outcome.ran == 0 and r.outcome.info.accepted == 1, wp=W.WideParams(20, 4, W.ON_REJECT)))
    add(Case("wide_always_shape", "s80", _pattern("s80", "full_col"), P34, guess("s80", 40, 41), wav, "when = ALWAYS with the shape over the wide window",
             lambda c, r: r.scores is None and r.outcome.ran == 1 and r.outcome.shape.computed == 1, wp=W.WideParams(17, 3, W.ALWAYS), shape=F.ShapeParams()))
    for c in cases:
        c.scan_cloud = R.cloud(c.scan, LASER)[0]
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = build()
CASE = {c.name: c for c in CASES}
PLANTS = ("disc", "transposed", "origin", "E", "outside", "chebyshev")


@functools.lru_cache(maxsize=None)
def expected(name) -> M.Result:
    """the restatement's result of a case: computed once, shared, never changed"""
    c = CASE[name]
    res = M.search(c.occ(), c.geom, c.scan_cloud, c.T, c.p, c.wp, c.shape)
    for a in (res.table, res.scores, res.wide_scores):
        if a is not None:
            a.setflags(write=False)
    return res


# ---- behaviour: maps drawn by the oracle's GridMapper from the rooms' own trajectories ------------------------------------------------
S400 = M.Geom(-10.0, -10.0, 0.05, 400)
BEHAVIOUR_MAPS = dict(bench=(rc.ROOM_BENCH, rc.TRAJ_BENCH, 12), survey=(rc.ROOM_SURVEY, rc.TRAJ_SURVEY, 20))
BEHAVIOUR_SEED = 7


@functools.lru_cache(maxsize=None)
def behaviour_map(which):
    """-> (log-odds [400][400] as the oracle's GridMapper holds them, occupancy uint8 [400][400], the trajectory's poses)"""
    import oracle_api as orc
    walls, inc, n = BEHAVIOUR_MAPS[which]
    _, poses = rc.trajectory(n, inc)
    rng = np.random.default_rng(BEHAVIOUR_SEED)
    g = orc.GridAPI("orc", grid=(0.05, -10.0, 10.0, -10.0, 10.0))
    assert (g.xsize, g.ysize) == (400, 400)
    for pose in poses:
        g.integrate_scan(orc.room_scan(tuple(pose), walls=walls, rng=rng), tuple(pose), esdf=False)
    lo = g.dump()["log_odds"].reshape(400, 400).copy()
    occ = np.zeros(400 * 400, dtype=np.uint8)
    occ[g.occ_cells()] = 1
    g.close()
    return lo, occ.reshape(400, 400), poses


def behaviour_scan(which, pose, seed=11):
    import oracle_api as orc
    return orc.room_scan(tuple(pose), walls=BEHAVIOUR_MAPS[which][0], rng=np.random.default_rng(seed))


@dataclass
class Behaviour:
    name: str
    map: str            # whose map
    room: str           # whose scan
    off: tuple          # the guess = truth + off (theta, x, y)
    p: S.Params
    wp: object
    accepted: object    # 1, 0, or None: recorded, not asserted
    truth: tuple = (0.2, 0.35, 0.22)
    to_cell: bool = False   # rejected, and all the same within one cell and one step of the truth


PB = S.Params()                      # the defaults: +-6 cells, +-20 steps
BEHAVIOURS = (
    Behaviour("b0", "bench", "bench", (0.0, 0.0, 0.0), PB, None, 1),
    Behaviour("b1", "bench", "bench", (0.1, 0.2, -0.15), PB, None, 1),
    Behaviour("b2", "bench", "bench", (0.3, 0.5, 0.4), PB, None, 0),
    Behaviour("b3", "bench", "bench", (0.3, 0.5, 0.4), PB.with_(lin_cells=14), None, 1),
    Behaviour("b4", "bench", "bench", (0.25, -0.65, 0.65), PB, None, 0),
    Behaviour("b5", "bench", "bench", (0.25, -0.65, 0.65), PB.with_(lin_cells=14), None, 1),
    Behaviour("s0", "survey", "survey", (0.6, 1.6, 0.9), PB, W.WideParams(48, 45, W.ALWAYS), 1),
    Behaviour("s1", "survey", "survey", (-0.7, -2.0, 1.5), PB, W.WideParams(48, 45, W.ALWAYS), 1, truth=(0.2, 1.2, -0.9)),
    Behaviour("s2", "survey", "survey", (-0.7, -2.0, 1.5), PB, W.WideParams(48, 45, W.ALWAYS), 0, to_cell=True),
    Behaviour("w0", "bench", "survey", (0.0, 0.0, 0.0), PB.with_(lin_cells=14), None, 0),
    Behaviour("w1", "bench", "survey", (0.0, 0.0, 0.0), PB, W.WideParams(48, 45, W.ALWAYS), None),
)


@functools.lru_cache(maxsize=None)
def behaviour_result(name) -> M.Result:
    b = {x.name: x for x in BEHAVIOURS}[name]
    _, occ, _ = behaviour_map(b.map)
    src = R.cloud(behaviour_scan(b.room, b.truth), LASER)[0]
    T = tuple(t + o for t, o in zip(b.truth, b.off))
    return M.search(occ, S400, src, T, b.p, b.wp)


# the qualities test_icp_search_map_cases.py measured, rounded to 3 places
BEHAVIOUR_RECORD = dict(b0=0.995, b1=0.992, b2=0.299, b3=0.996, b4=0.182, b5=0.996, s0=0.872, s1=0.984, s2=0.417, w0=0.402, w1=0.557)
