"""The case table of the map check (include/tbnav_icp.h, MAP CHECK V1-V10; csrc/icp_verify_map.hip): small maps, windows, log-odds,
scans and parameters at which icp_verify_map and the route round it can still go wrong.  tests/test_icp_verify_map_cases.py proves on
the CPU, on the restatement, that each case reaches what its `reaches` names and that each planted error changes a case;
tests/test_icp_verify_map_gpu.py holds the device to the restatement with == on every one.

Maps: side 64, 96, 80 (a ragged last tile) at 0.05 m and side 24 at 0.5 m (nav_from_map_cases' sizes); 400 x 400 for the behaviour.
A case's map is a grid of log-odds: U (0, unknown), F (free), FC (exactly the free cut), K (known and neither), O (occupied).  Probe
cases put single beams on chosen end cells: the pose stands at a cell's centre with theta = 0, so beam 0 / 45 / 90 / ... of range
n cells (n * sqrt 2 on a diagonal) ends n cells along +x / the diagonal / +y.  Room cases stand in a box of wall cells 8 cells (3 at
0.5 m) round the pose's cell over a drawn background of all five values, with a scan ray-cast to that box and every seventh beam cut
to half its range, so that it ends inside the room.

BEHAVIOUR (measured on the restatement at the defaults, H = 96, k = 2; maps drawn by the oracle's GridMapper,
icp_search_map_cases.behaviour_map; each pose is the one the search of icp_search_map_cases.BEHAVIOURS returned; `reverse` is the
bench room's scan searched in the survey room's map over WideParams(48, 45, ALWAYS) from (0.2, 0.35, 0.22); `mirror` is the bench
truth mirrored through the bench room's centre; asserted in test_icp_verify_map_cases.py).  BEHAVIOUR_RECORD holds the figures:
  pose (quality from the search)                        walked  hit  through  missing  unseen  accepted
  b0, b1, b3, b5 (true, 0.99)                           360     360  0        0        0       1
  s0 (true, 0.872)                                      291     291  0        0        0       1
  s1 (true, 0.984)                                      240     239  1        0        0       1
  s2 (true, REJECTED by the search at 0.417)            291     291  0        0        0       1
  b2 (the window's edge, rejected)                      360     149  136      74       1       0
  b4 (the window's edge, rejected)                      360     91   151      118      0       0
  w1 (survey scan, bench map, ACCEPTED at 0.557)        291     162  129      0        0       0
  reverse (bench scan, survey map, wide window)         360     200  0        138      22      0
  mirror (a symmetry of the finished rectangle)         360     360  0        0        0       1   (no method that reads the map can refuse it)
The largest share of beams THROUGH a wall at a true pose is 1 / 240 = 0.4 %, of beams MISSING 0; the wrong room shows 44 % THROUGH one
way round (w1) and 38 % MISSING the other (reverse): each wrong room trips one counter only, so both are needed.  The defaults
(102 / 1024 = 10 % each) stand at least 5 x above the former and below half the latter; test_icp_verify_map_cases.py asserts that."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np

import icp_restatement as R
import icp_verify_map_restatement as V
from icp_align_map_cases import box_walls, cast, centre, probe_scan
from icp_search_map_cases import geom
from nav_frontier_cases import F, K, O, U
import nav_from_map_cases as fc

LASER = R.lds01()
MAX_BEAMS = 4096            # TBNAV_ICP_MAX_BEAMS
FC = V.free_cut()           # the largest log-odds that is FREE
assert V.export_value(F) == 0 and V.export_value(FC) == 0 and V.export_value(U) == -1 and V.export_value(O) == 100 and 35 < V.export_value(K) < 90


def lo_grid(size_id, base, cells=None, rects=()):
    """() -> log-odds float64 [side][side]: `base` everywhere, then rects ((i0, i1, j0, j1) inclusive, value), then cells {(i, j): value};
    what falls outside the map is dropped"""
    def make():
        n = fc.SIZE[size_id].xsize
        lo = np.full((n, n), base, dtype=np.float64)
        for (i0, i1, j0, j1), v in rects:
            lo[max(i0, 0):i1 + 1, max(j0, 0):j1 + 1] = v
        for (i, j), v in (cells or {}).items():
            if 0 <= i < n and 0 <= j < n:
                lo[i, j] = v
        return lo
    return make


def occ_of(lo):
    """the occupancy bits of a log-odds grid: probability >= 0.90"""
    vals = {float(v): V.export_value(float(v)) == 100 for v in np.unique(lo)}
    return np.vectorize(lambda v: vals[float(v)], otypes=[np.uint8])(lo)


def drawn(size_id, seed, box=None):
    """a background drawn from all five values (2 % occupied) with the outline of the box of cells (cx - h .. cx + h) x (cy - h ..
    cy + h) on top, clipped to the map; the occupied cells the draw put inside the box send some beams THROUGH"""
    def make():
        n = fc.SIZE[size_id].xsize
        rng = np.random.default_rng(seed)
        lo = rng.choice(np.array([U, F, FC, K, O]), size=(n, n), p=[0.3, 0.4, 0.08, 0.2, 0.02])
        if box is not None:
            cx, cy, h = box
            for q in range(-h, h + 1):
                for i, j in ((cx - h, cy + q), (cx + h, cy + q), (cx + q, cy - h), (cx + q, cy + h)):
                    if 0 <= i < n and 0 <= j < n:
                        lo[i, j] = O
        return lo
    return make


@dataclass
class Case:
    name: str
    size_id: str
    lo: object                   # () -> float64 [side][side]
    p: V.Params
    T: tuple
    scan: np.ndarray
    reaches: str
    check: object                # (case, Result) -> bool: the proof that the case reaches what it names
    icp: dict = field(default_factory=dict)      # icp.default_params' keywords (Trs)
    plants: tuple = ()           # planted errors this case is known to expose

    @property
    def geom(self):
        return geom(self.size_id)

    @property
    def Trs(self):
        return self.icp.get("Trs", (0.0, 0.0, 0.0))


P8, P16, P32 = V.Params(half_cells=8), V.Params(half_cells=16), V.Params(half_cells=32)
AT = (30, 33)
DIRS = {0: (1, 0), 45: (1, 1), 90: (0, 1), 135: (-1, 1), 180: (-1, 0), 225: (-1, -1), 270: (0, -1), 315: (1, -1)}


def aim(di, dj, res=0.05):
    """(beam, range) whose end lies in the cell (di, dj) from the pose's cell; the case's check proves it"""
    return int(round(math.degrees(math.atan2(dj, di)))) % 360, math.hypot(di, dj) * res


def _at(cells, at=AT):
    return {(at[0] + i, at[1] + j): v for (i, j), v in cells.items()}


def _beam(beam, **want):
    """the hook's record of one beam holds these values (e relative to the sensor cell as de)"""
    def check(case, res):
        b, s = res.beams, res.info["sensor_cell"]
        ok = True
        for f, v in want.items():
            if f == "de":
                ok &= (b["ei"][beam] - s[0], b["ej"][beam] - s[1]) == tuple(v)
            else:
                ok &= int(b[f][beam]) == v
        return bool(ok)
    return check


def _all(*checks):
    return lambda case, res: all(ch(case, res) for ch in checks)


def _info(**want):
    return lambda case, res: all(res.info[f] == v for f, v in want.items())


def _probe(name, cells, beams, check, reaches, p=P16, plants=(), size_id="s64", at=AT, base=F, rects=(), icp=None):
    """beams: {beam: range in cells}"""
    res = fc.SIZE[size_id].res
    return Case(name, size_id, lo_grid(size_id, base, _at(cells, at), rects), p, centre(size_id, *at),
                probe_scan({b: r * res for b, r in beams.items()}), reaches, check, icp=icp or {}, plants=plants)


def _room(name, size_id, cx, cy, p, reaches, check, seed=5, th=0.1, h=None, n_beams=360, mutate=None, plants=(), icp=None):
    h = h if h is not None else (3 if size_id == "r20" else 8)
    truth = centre(size_id, cx, cy, th=th)
    scan = cast(truth, box_walls(size_id, cx, cy, h), n_beams)
    scan[3::7] *= np.float32(0.5)        # these end inside the room, on whatever the draw put there
    if mutate is not None:
        scan = mutate(scan)
    return Case(name, size_id, drawn(size_id, seed, (cx, cy, h)), p, truth, scan, reaches, check, icp=icp or {}, plants=plants)


def _mixed(case, res):
    """a room over a drawn background reaches every class"""
    i = res.info
    return min(i["hit"], i["through"], i["missing"], i["unseen"], i["undecided"], i["free_cells"], i["unknown_cells"]) > 0


def _accept_case(name, classes, p, accepted, reaches):
    """eight beams of n = 6 along the axes and diagonals, each made HIT, THROUGH or MISSING by what the map holds on its ray"""
    cells, beams = {}, {}
    for (beam, (ui, uj)), kind in zip(DIRS.items(), classes):
        beams[beam] = 6 * math.hypot(ui, uj)
        if kind == V.HIT:
            cells[(6 * ui, 6 * uj)] = O
        elif kind == V.THROUGH:
            cells[(2 * ui, 2 * uj)] = O
    want = dict(walked=8, hit=classes.count(V.HIT), through=classes.count(V.THROUGH), missing=classes.count(V.MISSING), accepted=accepted)
    return _probe(name, cells, beams, _info(**want), reaches, p=p)


def build():
    cases = []
    add = cases.append
    s2 = math.sqrt(2.0)
    # ---- rays: a row, a column, the exact diagonal, and the (8, 1) rounding step ----
    add(_probe("ray_row", {(7, 0): O}, {0: 7}, _beam(0, cls=V.HIT, de=(7, 0), n=7, b=7, D=0, free_cells=6, unknown_cells=0), "a ray along +x: n = 7, blocked at its end cell"))
    add(_probe("ray_col", {(0, -5): O, (0, -2): U}, {270: 5}, _beam(270, cls=V.HIT, de=(0, -5), n=5, b=5, free_cells=3, unknown_cells=1),
               "a ray along -y with one UNKNOWN cell on it"))
    add(_probe("ray_diag", {(-6, 6): O}, {135: 6 * s2}, _beam(135, cls=V.HIT, de=(-6, 6), n=6, b=6, free_cells=5), "the exact diagonal (-1, +1)"))
    b81, r81 = aim(8, 1)
    add(_probe("ray_8_1", {(4, 0): O}, {b81: r81 / 0.05}, _beam(b81, cls=V.MISSING, de=(8, 1), n=8, b=-1, free_cells=7),
               "(8, 1): the closed form turns at step 4 to (4, 1) and grazes the wall (4, 0); a carried error turns at step 5 and hits it", plants=("bresenham",)))
    # ---- THROUGH on its edge: a wall at b = n - k - 1 (beam 0) and at b = n - k (beam 180), n = 12 ----
    for k in (0, 2, 8):
        pk = P16.with_(slack_cells=k)
        add(_probe(f"through_k{k}", {(12 - k - 1, 0): O, (-(12 - k), 0): O}, {0: 12, 180: 12},
                   _all(_beam(0, cls=V.THROUGH, n=12, b=12 - k - 1, D=-1), _beam(180, cls=V.HIT, n=12, b=12 - k, D=k * k)),
                   f"k = {k}: b + k = n - 1 is THROUGH, b + k = n is not (and D = k^2 is a HIT)", p=pk, plants=("through_le",) if k == 2 else ()))
    # ---- D on its edge (k = 2), beside the ray so that nothing blocks ----
    add(_probe("D_eq", {(6, 2): O}, {0: 6}, _beam(0, cls=V.HIT, b=-1, D=4), "D = k^2 = 4: HIT"))
    add(_probe("D_over", {(7, 2): O}, {0: 6}, _beam(0, cls=V.MISSING, b=-1, D=5), "D = k^2 + 1 = 5, inside the box and outside the disc: not a HIT", plants=("chebyshev",)))
    add(_probe("D_corner", {(8, -2): O, (9, 0): O}, {0: 6}, _beam(0, cls=V.MISSING, b=-1, D=8), "(2, -2) inside the box (D = 8), (3, 0) outside it"))
    add(_probe("D_none", {(9, 0): O}, {0: 6}, _beam(0, cls=V.MISSING, b=-1, D=-1), "the box holds no occupied cell: D = -1"))
    add(_probe("D_k0", {(6, 1): O}, {0: 6}, _beam(0, cls=V.MISSING, D=-1), "k = 0: the box is the end cell alone", p=P16.with_(slack_cells=0)))
    # ---- the corner rule ----
    add(_probe("corner_wall", {(3, 4): O, (4, 3): O}, {45: 8 * s2}, _beam(45, cls=V.THROUGH, n=8, b=4, free_cells=3),
               "a diagonal wall that is only 8-connected blocks the diagonal step", plants=("no_corner",)))
    add(_probe("corner_graze", {(3, 4): O}, {45: 8 * s2}, _beam(45, cls=V.MISSING, n=8, b=-1, free_cells=7), "one orthogonal cell occupied: the ray goes on"))
    # ---- n = 0 (0.5 m cells: a range of 0.2 m stays in the pose's cell) ----
    add(_probe("n_zero", {}, {0: 0.4}, _beam(0, cls=V.MISSING, de=(0, 0), n=0, b=-1, free_cells=0), "n = 0: never THROUGH, no path", size_id="r20", at=(11, 13), p=P8))
    add(_probe("n_zero_hit", {(0, 1): O}, {0: 0.4}, _beam(0, cls=V.HIT, n=0, D=1), "n = 0 beside a wall: HIT", size_id="r20", at=(11, 13), p=P8))
    # ---- the end cell's class ----
    add(_probe("end_free", {}, {90: 5}, _beam(90, cls=V.MISSING, free_cells=4), "the end cell FREE: MISSING; it is not counted on the path", plants=("count_end",)))
    add(_probe("end_free_cut", {}, {90: 5}, _beam(90, cls=V.MISSING, free_cells=4), "log-odds exactly the free cut are FREE", base=FC, plants=("free_strict",)))
    add(_probe("end_unknown", {(0, 5): U, (0, 4): U}, {90: 5}, _beam(90, cls=V.UNSEEN, free_cells=3, unknown_cells=1), "the end cell UNKNOWN: UNSEEN"))
    add(_probe("end_other", {(0, 5): K, (0, 3): K}, {90: 5}, _beam(90, cls=V.UNDECIDED, free_cells=3, unknown_cells=0), "the end cell known and neither: UNDECIDED"))
    add(_probe("end_tile_0", {}, {0: 6}, _all(_beam(0, cls=V.UNSEEN, de=(6, 0), free_cells=3, unknown_cells=2), lambda c, r: not c.lo()[32:, 32:].any()),
               "the end cell in a tile nobody has written (id 0), the path across the tile seam: rows 29 .. 31 FREE, 32 and 33 UNKNOWN",
               at=(28, 36), rects=(((32, 63, 32, 63), U),)))
    add(_probe("end_outside_window", {}, {0: 8, 180: 9, 90: 7}, _all(_beam(0, cls=V.OUTSIDE, n=0), _beam(180, cls=V.OUTSIDE), _beam(90, cls=V.MISSING, n=7), _info(points=3, outside=2, walked=1)),
               "H = 8: sx + 8 and sx - 9 are outside the window, sy + 7 is its last column", p=P8))
    add(_probe("end_outside_map", {}, {0: 5, 90: 4}, _all(_beam(0, cls=V.OUTSIDE), _beam(90, cls=V.MISSING), _info(outside=1, walked=1)),
               "the end cell beyond the map's last row", at=(60, 30)))
    add(_probe("end_outside_ragged", {}, {90: 5, 0: 4}, _all(_beam(90, cls=V.OUTSIDE), _beam(0, cls=V.MISSING), _info(outside=1, walked=1)),
               "the end cell in the ragged part of the last tile (side 80)", size_id="s80", at=(40, 76)))
    # ---- the sensor cell on the map's edge and in its corners: the window hangs over ----
    last = 63
    for name, (cx, cy), beam, p in (("corner_00", (0, 0), 0, P8), ("corner_0L", (0, last), 0, P16), ("corner_L0", (last, 0), 180, P32),
                                    ("corner_LL", (last, last), 180, P8), ("edge_low_x", (0, 40), 0, P16), ("edge_high_y", (40, last), 270, P8)):
        ui, uj = DIRS[beam]
        add(_probe(name, {(4 * ui, 4 * uj): O, (2 * ui, 2 * uj): U}, {beam: 4}, _all(_beam(beam, cls=V.HIT, n=4, b=4, free_cells=2, unknown_cells=1), _info(sensor_cell=(cx, cy), sensor_class=V.C_FREE)),
                   f"the sensor in cell {(cx, cy)}, H = {p.half_cells}: the window hangs over the map's side", at=(cx, cy), p=p))
    add(_probe("sensor_classes", {(0, 0): K}, {0: 4}, _info(sensor_class=V.C_OTHER), "the sensor cell known and neither: reported"))
    add(_probe("sensor_occupied", {(0, 0): O}, {0: 4}, _all(_info(sensor_class=V.C_OCCUPIED), _beam(0, cls=V.MISSING, b=-1)), "the sensor cell OCCUPIED: reported, never tested as a step"))
    # ---- window origins at bit offsets 0, 1, 31, 32 of a map word (H = 16: sy - H = the offset), rows across the tile seam too ----
    for b in (0, 1, 31, 32):
        add(_room(f"origin_{b}", "s96", 16 + (32 - b), 16 + b, P16, f"sy - H = {b}, sx - H = {32 - b}: the bit offset of the window in a word",
                  lambda c, r, b=b: (r.info["sensor_cell"][1] - 16) % 32 == b % 32 and _mixed(c, r), seed=100 + b, plants=("transposed",) if b == 1 else ()))
    # ---- whole rooms: other sizes, H and k ----
    add(_room("room_defaults", "s80", 40, 41, V.Params(), "H = 96 round an 80-cell map with a ragged last tile, the defaults", _mixed))
    add(_room("room_H128_k8", "s80", 75, 4, V.Params(half_cells=128, slack_cells=8), "H = 128 (8 words a row), k = 8 (every end within 8 cells of the box is a HIT), the room over the map's edge",
              lambda c, r: r.info["outside"] > 100 and r.info["hit"] > 100 and r.info["free_cells"] > 0 and r.info["unknown_cells"] > 0, seed=8))
    add(_room("room_odd_H", "s96", 50, 47, V.Params(half_cells=9, slack_cells=1), "H = 9 (18 bits a row), k = 1", _mixed, seed=9))
    add(_room("room_50cm", "r20", 11, 13, P8, "0.5 m cells, side 24, H = 8", lambda c, r: c.geom.side == 24 and r.info["hit"] > 100))
    add(_room("room_trs", "s64", 30, 33, P16, "a sensor offset Trs: s and the robot in different cells",
              lambda c, r: r.info["sensor_cell"] != V.cell_of(c.geom, c.T[1], c.T[2]) and r.info["walked"] > 100, icp=dict(Trs=(0.3, 0.2, 0.1)), plants=("no_trs",)))
    # ---- beam counts ----
    for nb in (1, 255, 256, 257, 360, 1080, MAX_BEAMS):
        add(_room(f"beams_{nb}", "s64", 30, 33, P16, f"{nb} beams ({-(-nb // 256)} a thread)",
                  lambda c, r, nb=nb: r.beams["cls"].size == nb and r.info["points"] == nb and (nb < 255 or _mixed(c, r)), n_beams=nb, seed=nb))
    # ---- ranges that are no number or out of range ----
    def holes(scan):
        scan = scan.copy()
        scan[5::11] = np.nan
        scan[7::13] = np.inf
        scan[3::17] = -np.inf
        scan[2::19] = 0.05      # below range_min
        scan[9::23] = 3.5       # range_max itself
        return scan
    add(_room("nan_inf", "s64", 30, 33, P16, "NaN, inf and out-of-range ranges are no points", lambda c, r: 200 < r.info["points"] < 300 and (r.beams["cls"][5::11] == V.NONE).all(), mutate=holes))
    # ---- acceptance: each inequality on its edge and one beam either side of it ----
    H_, T_, M_ = V.HIT, V.THROUGH, V.MISSING
    open_ = dict(half_cells=16, max_through_q10=1024, max_missing_q10=1024, min_hit_q10=0)
    for m in (3, 4, 5):      # of 8 walked beams against 512 / 1024: 4 is the edge
        add(_accept_case(f"accept_through_{m}", [T_] * m + [H_] * (8 - m), V.Params(**dict(open_, max_through_q10=512)), int(m <= 4),
                         f"through = {m} of 8 against max_through_q10 = 512"))
        add(_accept_case(f"accept_missing_{m}", [M_] * m + [H_] * (8 - m), V.Params(**dict(open_, max_missing_q10=512)), int(m <= 4),
                         f"missing = {m} of 8 against max_missing_q10 = 512"))
        add(_accept_case(f"accept_hit_{m}", [H_] * m + [M_] * (8 - m), V.Params(**dict(open_, min_hit_q10=512)), int(m >= 4),
                         f"hit = {m} of 8 against min_hit_q10 = 512"))
    add(_probe("accept_nothing_walked", {}, {0: 9}, _info(points=1, walked=0, accepted=0), "walked = 0 is not accepted, whatever the thresholds",
               p=V.Params(**dict(open_, half_cells=8))))
    add(Case("accept_no_points", "s64", lo_grid("s64", F), V.Params(**open_), centre("s64", *AT), probe_scan({}), "a scan without a point", _info(points=0, walked=0, accepted=0)))
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        c.cloud, c.beam = R.cloud(c.scan, LASER, c.Trs)
    return cases


CASES = build()
CASE = {c.name: c for c in CASES}
PLANTS = V.PLANTS
NON_FINITE_POSES = ((float("nan"), 0.0, 0.0), (0.1, float("nan"), 0.0), (0.1, 0.0, float("inf")), (float("-inf"), 0.0, 0.0))


def classes_of(c: Case, plant=None) -> V.Classes:
    lo = c.lo()
    return V.Classes.from_log_odds(lo, occ_of(lo), plant)


def run(c: Case, plant=None, T=None, p=None) -> V.Result:
    return V.verify(classes_of(c, plant), c.geom, c.cloud, c.beam, c.scan.size, c.T if T is None else T, c.p if p is None else p,
                    V.origin_of(c.Trs), plant=plant)


@functools.lru_cache(maxsize=None)
def expected(name) -> V.Result:
    """the restatement's result of a case: computed once, shared, never changed"""
    res = run(CASE[name])
    for a in res.beams.values():
        a.setflags(write=False)
    return res


def digest(res: V.Result):
    """every bit of a result"""
    if res is None:
        return None
    return (tuple(sorted(res.info.items())), tuple(a.tobytes() for a in res.beams.values()))


# ---- behaviour: maps drawn by the oracle's GridMapper (icp_search_map_cases.behaviour_map) ------------------------------------------------
BEHAVIOUR_TRUE = ("b0", "b1", "b3", "b5", "s0", "s1", "s2")      # true poses: accepted at the defaults, s2 (which the search rejects) included
BEHAVIOUR_REFUSED = ("b2", "b4", "w1", "reverse")                # the window's edge twice, and the wrong room both ways round
BEHAVIOUR_TRUTH = (0.2, 0.35, 0.22)


@functools.lru_cache(maxsize=None)
def behaviour_classes(room) -> V.Classes:
    import icp_search_map_cases as mc
    lo, occ, _ = mc.behaviour_map(room)
    return V.Classes.from_log_odds(lo, occ)


@functools.lru_cache(maxsize=None)
def behaviour_pose(name):
    """-> (whose map, the scan, the pose the search returned or the mirror pose)"""
    import icp_search_map_cases as mc
    import icp_search_map_restatement as M
    import icp_search_wide_restatement as W
    import rbpf_cases as rc
    if name == "reverse":
        scan = mc.behaviour_scan("bench", BEHAVIOUR_TRUTH)
        _, occ, _ = mc.behaviour_map("survey")
        res = M.search(occ, mc.S400, R.cloud(scan, LASER)[0], BEHAVIOUR_TRUTH, mc.PB, W.WideParams(48, 45, W.ALWAYS))
        return "survey", scan, tuple(res.outcome.info.T)
    if name == "mirror":
        x0, x1, y0, y1 = rc.ROOM_BENCH
        th, x, y = BEHAVIOUR_TRUTH
        return "bench", mc.behaviour_scan("bench", BEHAVIOUR_TRUTH), (th + math.pi, (x0 + x1) - x, (y0 + y1) - y)
    b = {q.name: q for q in mc.BEHAVIOURS}[name]
    return b.map, mc.behaviour_scan(b.room, b.truth), tuple(mc.behaviour_result(name).outcome.info.T)


@functools.lru_cache(maxsize=None)
def behaviour(name) -> dict:
    """V7's record of one behaviour pose at the defaults"""
    import icp_search_map_cases as mc
    room, scan, T = behaviour_pose(name)
    cloud, beam = R.cloud(scan, LASER)
    return V.verify(behaviour_classes(room), mc.S400, cloud, beam, scan.size, T, V.Params()).info


# what test_icp_verify_map_cases.py measured: pose -> (walked, hit, through, missing, unseen, undecided, accepted)
BEHAVIOUR_RECORD = dict(
    b0=(360, 360, 0, 0, 0, 0, 1), b1=(360, 360, 0, 0, 0, 0, 1), b3=(360, 360, 0, 0, 0, 0, 1), b5=(360, 360, 0, 0, 0, 0, 1),
    s0=(291, 291, 0, 0, 0, 0, 1), s1=(240, 239, 1, 0, 0, 0, 1), s2=(291, 291, 0, 0, 0, 0, 1),
    b2=(360, 149, 136, 74, 1, 0, 0), b4=(360, 91, 151, 118, 0, 0, 0), w1=(291, 162, 129, 0, 0, 0, 0), reverse=(360, 200, 0, 138, 22, 0, 0),
    mirror=(360, 360, 0, 0, 0, 0, 1))
BEHAVIOUR_FIELDS = ("walked", "hit", "through", "missing", "unseen", "undecided", "accepted")
