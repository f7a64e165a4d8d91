"""The case table of the map alignment (include/tbnav_icp.h, MAP ALIGNMENT A1-A11; csrc/icp_align_map.hip): small maps, windows,
occupancies, scans and parameters at which icp_align_map and the route round it can still go wrong.  tests/test_icp_align_map_cases.py
proves on the CPU, on the restatement, that each case reaches what its `reaches` names and that each planted error changes a case;
tests/test_icp_align_map_gpu.py holds the device to the restatement with == on every one.

Maps: side 64, 96, 80 (a ragged last tile) at 0.05 m and side 24 at 0.5 m (nav_from_map_cases' sizes); 400 x 400 for the behaviour.
Probe cases put ONE beam on a chosen home cell: the pose stands at a cell's centre with theta = 0, so beam 0 / 90 / 180 / 270 of
range 4 cells has its home 4 cells along +x / +y / -x / -y.  Room cases stand in a box of wall cells 6 cells (3 at 0.5 m) round the
pose's cell, with a scan ray-cast to that box.

BEHAVIOUR (measured on the restatement, H = 128, the defaults; maps drawn by the oracle's GridMapper from 12 scans of ROOM_BENCH and
20 scans of ROOM_SURVEY, icp_search_map_cases.behaviour_map; the scan taken at the truth (0.2, 0.35, 0.22) with 1 cm range noise;
BEHAVIOUR_STARTS starts per room drawn with seed BEHAVIOUR_SEED within half a cell and half a degree of the truth; asserted in
test_icp_align_map_cases.py: both means after alignment are below the starts'; no millimetre figure is asserted):
  room    starts (mean / max)      after (mean / max)      iterations (mean / max)   converged
  bench   14.8 / 30.8 mm, 4.5 / 7.9 mrad   0.9 / 0.9 mm, 0.5 / 0.5 mrad   2.7 / 3   12 of 12
  survey  14.8 / 30.8 mm, 4.5 / 7.9 mrad   1.3 / 1.3 mm, 0.1 / 0.1 mrad   2.3 / 3   12 of 12
Every start of a room ends on the same pose: one scan and one map have one fixed point inside this basin, and what is left is that
scan's noise and the map's rasterisation.  BEHAVIOUR_RECORD holds the figures."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np

import icp_align_map_restatement as A
import icp_restatement as R
import nav_from_map_cases as fc
from icp_search_map_cases import geom, guess

LASER = R.lds01()
MAX_BEAMS = 4096            # TBNAV_ICP_MAX_BEAMS
ICP = dict(max_iter=100, transform_eps=1e-8, fitness_eps=1e-6)      # tbnav_icp_default_params


def centre(size_id, cx, cy, th=0.0):
    """the world pose at the centre of map cell (cx, cy)"""
    return guess(size_id, cx, cy, th=th, fx=0.5, fy=0.5)


def probe_scan(ranges: dict, n_beams=360):
    """a scan whose only points are the named beams"""
    s = np.full(n_beams, 0.05, dtype=np.float32)       # below range_min
    for b, r in ranges.items():
        s[b] = r
    return s


def cast(pose, walls, n_beams=360):
    """ranges of n_beams beams (the laser's own angles, wrap included) from pose to the inside of the box walls = (x0, x1, y0, y1)"""
    cs = R.beam_table(LASER, n_beams).astype(np.float64)
    c, s = math.cos(pose[0]), math.sin(pose[0])
    dx, dy = c * cs[:, 0] - s * cs[:, 1], s * cs[:, 0] + c * cs[:, 1]
    x0, x1, y0, y1 = walls
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = np.where(dx > 0, (x1 - pose[1]) / dx, np.where(dx < 0, (x0 - pose[1]) / dx, np.inf))
        ty = np.where(dy > 0, (y1 - pose[2]) / dy, np.where(dy < 0, (y0 - pose[2]) / dy, np.inf))
    return np.minimum(tx, ty).astype(np.float32)


def box_occ(size_id, cx, cy, h, extra=None):
    """the outline of the box of cells (cx - h .. cx + h) x (cy - h .. cy + h), clipped to the map, over `extra`"""
    def make():
        s = fc.SIZE[size_id]
        occ = np.zeros((s.xsize, s.xsize), dtype=np.uint8) if extra is None else fc.patterns(s)[extra].copy()
        for k in range(-h, h + 1):
            for i, j in ((cx - h, cy + k), (cx + h, cy + k), (cx + k, cy - h), (cx + k, cy + h)):
                if 0 <= i < s.xsize and 0 <= j < s.xsize:
                    occ[i, j] = 1
        return occ
    return make


def box_walls(size_id, cx, cy, h):
    """the box of wall-cell CENTRES round cell (cx, cy): what a scan of box_occ's room measures"""
    g = geom(size_id)
    x, y = g.xmin + (cx + 0.5) * g.resolution, g.ymin + (cy + 0.5) * g.resolution
    d = h * g.resolution
    return (x - d, x + d, y - d, y + d)


def cells_occ(size_id, cells):
    return lambda: fc._occ(fc.SIZE[size_id], cells)


@dataclass
class Case:
    name: str
    size_id: str
    occ: object                  # () -> uint8 [side][side]
    p: A.Params
    T: tuple
    scan: np.ndarray
    reaches: str
    check: object                # (case, Result) -> bool: the proof that the case reaches what it names
    icp: dict = field(default_factory=lambda: dict(ICP))
    plants: tuple = ()           # planted errors this case is known to expose

    @property
    def geom(self):
        return geom(self.size_id)


P8, P16, P32 = A.Params(half_cells=8), A.Params(half_cells=16), A.Params(half_cells=32)
HOME = (34, 33)                  # beam 0's home from the pose at the centre of (30, 33)
AT = (30, 33)


def _off(cells, at=HOME):
    return tuple((at[0] + i, at[1] + j) for i, j in cells)


def _probe(name, cells, check, reaches, p=P16, plants=(), beams=None, size_id="s64", at=AT):
    return Case(name, size_id, cells_occ(size_id, cells), p, centre(size_id, *at), probe_scan(beams or {0: 0.2}), reaches, check, plants=plants)


def _target(beam, home, target, D=None, kept=None, has=None):
    def check(case, res):
        q = res.pairing
        ok = q.has_home[beam] == 1 and (q.hi[beam], q.hj[beam]) == tuple(home)
        ok &= (q.mi[beam], q.mj[beam]) == tuple(target)
        if D is not None:
            ok &= q.D[beam] == D
        if kept is not None:
            ok &= q.kept[beam] == kept
        if has is not None:
            ok &= q.has_normal[beam] == has
        return bool(ok)
    return check


def _feature(has, normal=None, centroid_off=None):
    """beam 0's target is its home cell HOME; its feature"""
    def check(case, res):
        q, g = res.pairing, case.geom
        ok = (q.mi[0], q.mj[0]) == HOME and q.D[0] == 0 and q.has_normal[0] == has and q.kept[0] == has
        if normal is not None:
            ok &= abs(float(q.nx[0]) - normal[0]) < 1e-6 and abs(float(q.ny[0]) - normal[1]) < 1e-6
        if centroid_off is not None:
            ok &= abs(q.bx[0] - (g.xmin + (HOME[0] + 0.5 + centroid_off[0]) * g.resolution)) < 1e-12
            ok &= abs(q.by[0] - (g.xmin + (HOME[1] + 0.5 + centroid_off[1]) * g.resolution)) < 1e-12
        return bool(ok)
    return check


def _room(name, size_id, cx, cy, p, reaches, check, off=(0.03, 0.011, -0.008), h=None, n_beams=360, icp=None, extra=None, plants=(), mutate=None):
    h = h if h is not None else (3 if size_id == "r20" else 6)
    g = geom(size_id)
    truth = centre(size_id, cx, cy, th=0.1)
    scan = cast(truth, box_walls(size_id, cx, cy, h), n_beams)
    if mutate is not None:
        scan = mutate(scan)
    scale = g.resolution / 0.05
    T = (truth[0] + off[0], truth[1] + off[1] * scale, truth[2] + off[2] * scale)
    return Case(name, size_id, box_occ(size_id, cx, cy, h, extra), p, T, scan, reaches, check, icp=dict(ICP, **(icp or {})), plants=plants)


def _ended(crit, iterations=None):
    def check(case, res):
        return res.criterion == crit and (iterations is None or res.iterations == iterations) and res.ok == (crit <= R.REL_MSE)
    return check


def build():
    cases = []
    add = cases.append
    # ---- windows over the map's corners and edges: H = 8, 16, 32 ----
    last = 63
    for name, (cx, cy), beam, wall, p in (
            ("corner_00", (0, 0), 0, [(4, 0), (4, 1), (4, 2), (4, 3)], P8),
            ("corner_0L", (0, last), 0, [(4, last), (4, last - 1), (4, last - 2)], P16),
            ("corner_L0", (last, 0), 180, [(last - 4, 0), (last - 4, 1), (last - 4, 2)], P32),
            ("corner_LL", (last, last), 180, [(last - 4, last), (last - 4, last - 1), (last - 4, last - 2)], P8),
            ("edge_low_x", (0, 40), 0, [(4, 39), (4, 40), (4, 41)], P16),
            ("edge_high_y", (40, last), 270, [(39, last - 4), (40, last - 4), (41, last - 4)], P8)):
        home = {0: (cx + 4, cy), 180: (cx - 4, cy), 270: (cx, cy - 4)}[beam]
        add(Case(name, "s64", cells_occ("s64", wall), p, centre("s64", cx, cy), probe_scan({beam: 0.2}),
                 f"the guess in cell {(cx, cy)}, H = {p.half_cells}: the window hangs over the map's side", _target(beam, home, home, 0, 1, 1)))
    # the window's own edge: a wall 2 cells outside the window does not exist, one on its last row does (H = 8 round (30, 33))
    add(_probe("window_edge", [(38, 33), (38, 34), (38, 32), (37, 36)], _target(0, HOME, (37, 36), 18, 0, 0),
               "cells on row cx + H do not exist; the window's last row cx + H - 1 does", p=P8))
    # ---- window origins at bit offsets 0, 1, 31, 32 of a map word (H = 16: cy - H = the offset), rows across the tile seam too ----
    for b in (0, 1, 31, 32):
        add(_room(f"origin_{b}", "s96", 16 + (32 - b), 16 + b, P16, f"cy - H = {b}, cx - H = {32 - b}: the bit offset of the window in a word",
                  lambda c, r, b=b: (A.cell_of(c.geom, c.T[1], c.T[2])[1] - 16) % 32 == b % 32 and r.pairing.kept.sum() > 100, extra="random",
                  plants=("transposed",) if b == 1 else ()))
    # ---- ties ----
    add(_probe("tie_4", _off([(-3, 0), (0, -3), (0, 3), (3, 0)]), _target(0, HOME, (HOME[0] - 3, HOME[1]), 9, 0, 0),
               "equal D = 9 at (-3, 0), (0, -3), (0, 3), (3, 0): the lowest mi", plants=("tie_high",)))
    add(_probe("tie_rows", _off([(0, -3), (0, 3)]), _target(0, HOME, (HOME[0], HOME[1] - 3), 9, 0, 0), "equal D in one row: the lowest mj"))
    add(_probe("tie_3", _off([(-3, 4), (-4, 3), (-5, 0)]), _target(0, HOME, (HOME[0] - 5, HOME[1]), 25, 0, 0),
               "equal D = 25 at (-3, 4), (-4, 3), (-5, 0): the row at dr^2 == D wins", plants=("early_stop", "chebyshev")))
    # ---- the gate: G = 3 ----
    g3 = P16.with_(gate_cells=3)
    add(_probe("gate_eq", _off([(3, -2), (3, -1), (3, 0), (3, 1), (3, 2)]), _target(0, HOME, (HOME[0] + 3, HOME[1]), 9, 1, 1), "D = G^2 = 9 is kept", p=g3))
    add(_probe("gate_over", _off([(3, 1), (3, 2), (3, 3)]), _target(0, HOME, (HOME[0] + 3, HOME[1] + 1), 10, 0, 1),
               "D = G^2 + 1 = 10, inside the Chebyshev box and outside the disc: the target, with a normal, dropped", p=g3))
    add(_probe("gate_box", _off([(4, 0), (4, 1), (4, -1)]), _target(0, HOME, (-1, -1), -1, 0, 0), "a wall one column outside the box: no target", p=g3))
    # ---- features (beam 0's target is HOME itself) ----
    s2 = math.sqrt(0.5)
    feats = (
        ("feat_n2", [(0, 0), (0, 1)], 2, 0, None, (0.0, 0.5), "n = 2: no normal"),
        ("feat_collinear_3", [(0, -1), (0, 0), (0, 1)], 2, 1, (1.0, 0.0), (0.0, 0.0), "three collinear cells along j (b = 0, a < c): the normal (1, 0)"),
        ("feat_along_i", [(-2, 0), (-1, 0), (0, 0), (1, 0)], 2, 1, (0.0, 1.0), (-0.5, 0.0), "b = 0, a > c: the normal (0, 1), the centroid half a cell off"),
        ("feat_blob", [(i, j) for i in range(-2, 3) for j in range(-2, 3)], 2, 0, None, (0.0, 0.0), "a full 5 x 5 blob (b = 0, a = c): no normal"),
        ("feat_plus", [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)], 2, 0, None, (0.0, 0.0), "b = 0 with a = c (a plus): no normal"),
        ("feat_diag_pos", [(-2, -2), (-1, -1), (0, 0), (1, 1), (2, 2)], 2, 1, (s2, -s2), (0.0, 0.0), "a diagonal with b > 0"),
        ("feat_diag_neg", [(-2, 2), (-1, 1), (0, 0), (1, -1), (2, -2)], 2, 1, (-s2, -s2), (0.0, 0.0), "a diagonal with b < 0"),
        ("feat_corner_L", [(0, 0), (1, 0), (2, 0), (0, 1), (0, 2)], 2, 0, None, (0.6, 0.6), "the inside of an L corner: lmin / lmax = 0.28 > f"),
        ("feat_thick_wall", [(i, j) for i in (0, 1) for j in range(-2, 3)], 2, 1, (1.0, 0.0), (0.5, 0.0), "a two-cell-thick wall: the centroid lies between the rows"),
        ("feat_w1", [(0, -2), (0, -1), (0, 0), (0, 1), (0, 2), (2, 0)], 1, 1, (1.0, 0.0), (0.0, 0.0), "w = 1: the cell 2 columns off takes no part"),
        ("feat_w4", [(0, -4), (0, 0), (0, 4), (4, 0)], 4, 0, None, (1.0, 0.0), "w = 4: cells 4 off take part (n = 4, no line)"),
    )
    for name, cells, w, has, normal, coff, reaches in feats:
        plants = dict(feat_thick_wall=("centre", "no_half"), feat_w1=("w_plus",), feat_w4=("w_minus",)).get(name, ())
        add(_probe(name, _off(cells), _feature(has, normal, coff), reaches, p=P16.with_(feature_cells=w), plants=plants))
    # ---- 2 and 3 kept pairs ----
    # beam 0 -> (34, 33) and beam 45 at 0.3 m -> (34, 37), walls along j; beam 270 -> (30, 29), a wall along i.  (Beam 45's normal does not
    # point along its ray: three points whose normals do leave the rotation undetermined.)
    three = _off([(0, -1), (0, 0), (0, 1)]) + _off([(-1, 0), (0, 0), (1, 0)], (30, 29)) + _off([(0, -1), (0, 0), (0, 1)], (34, 37))
    add(_probe("kept_2", three, lambda c, r: r.criterion == R.NO_CORRESPONDENCES and r.correspondences == 2 and r.T == c.T and not r.ok,
               "2 kept pairs: NO_CORRESPONDENCES, T_out = T_init", beams={0: 0.2, 270: 0.2}))
    add(_probe("kept_3", three, lambda c, r: r.pairing.kept.sum() == 3 and r.criterion not in (R.NO_CORRESPONDENCES, R.DEGENERATE),
               "3 kept pairs with normals along both axes: a step is taken", beams={0: 0.2, 270: 0.2, 45: 0.3}))
    # ---- a corridor: two walls along x, nothing that holds x ----
    def corridor_occ():
        occ = np.zeros((64, 64), dtype=np.uint8)
        occ[:, 33 - 6] = 1
        occ[:, 33 + 6] = 1
        return occ
    ang = np.deg2rad(np.arange(360))
    cor = np.full(360, 0.05, dtype=np.float32)
    side = (np.abs(np.sin(ang)) > 0.8)
    cor[side] = (0.3 / np.abs(np.sin(ang[side]))).astype(np.float32)
    cT = centre("s64", 30, 33)
    add(Case("corridor", "s64", corridor_occ, P16, (0.0, cT[1] + 0.01, cT[2] + 0.012), cor, "a corridor: DEGENERATE, T_out = T_init",
             lambda c, r: r.criterion == R.DEGENERATE and r.T == c.T and not r.ok and r.correspondences > 50 and r.mse > 0.0))
    # ---- the stop rules, max_iter 1 and 2 ----
    add(_room("stop_iter_1", "s64", 30, 33, P16, "max_iter = 1: ITERATIONS after one step", _ended(R.ITERATIONS, 1), icp=dict(max_iter=1)))
    add(_room("stop_iter_2", "s64", 30, 33, P16, "max_iter = 2: ITERATIONS after two", _ended(R.ITERATIONS, 2), icp=dict(max_iter=2)))
    add(_room("stop_transform", "s64", 30, 33, P16, "TRANSFORM", _ended(R.TRANSFORM), icp=dict(transform_eps=1e-4)))
    add(_room("stop_abs", "s64", 30, 33, P16, "ABS_MSE", _ended(R.ABS_MSE), icp=dict(transform_eps=0.0, fitness_eps=0.0), off=(0.0, 0.0, 0.0)))
    add(_room("stop_rel", "s64", 30, 33, P16, "REL_MSE", _ended(R.REL_MSE), icp=dict(transform_eps=0.0, fitness_eps=1e-2)))
    add(_room("room_defaults", "s80", 40, 41, A.Params(), "H = 128 round an 80-cell map with a ragged last tile, the defaults",
              lambda c, r: r.ok and r.pairing.kept.sum() > 300, extra="random"))
    add(_room("room_50cm", "r20", 11, 13, P8, "0.5 m cells, side 24, H = 8", lambda c, r: c.geom.side == 24 and r.ok and r.pairing.kept.sum() > 300))
    add(_room("room_odd_H", "s96", 50, 47, A.Params(half_cells=9, gate_cells=16, feature_cells=3), "H = 9 (18 bits a row), G = 16, w = 3",
              lambda c, r: r.ok and r.pairing.kept.sum() > 300))
    add(_room("room_H256", "s96", 50, 47, A.Params(half_cells=256, gate_cells=1, feature_cells=1), "H = 256 (16 words a row), G = 1, w = 1",
              lambda c, r: r.pairing.kept.sum() > 100))
    # ---- beam counts ----
    for nb in (1, 3, 255, 256, 257, 1000, 1080, 2000, MAX_BEAMS):
        add(_room(f"beams_{nb}", "s64", 30, 33, P16, f"{nb} beams ({-(-nb // 256)} a thread)",
                  lambda c, r, nb=nb: r.pairing.has_home.size == nb and r.pairing.kept.sum() == min(nb, r.pairing.kept.sum()) and (nb < 3) == (r.criterion == R.NO_CORRESPONDENCES),
                  n_beams=nb, icp=dict(max_iter=4 if nb > 360 else 100)))
    # ---- ranges that are no number ----
    def holes(scan):
        scan = scan.copy()
        scan[5::11] = np.nan
        scan[7::13] = np.inf
        scan[3::17] = -np.inf
        return scan
    add(_room("nan_inf", "s64", 30, 33, P16, "NaN and inf ranges are no points", lambda c, r: r.ok and 250 < r.pairing.has_home.sum() < 320, mutate=holes))
    add(Case("empty", "s64", cells_occ("s64", ()), P16, centre("s64", 30, 33), cast(centre("s64", 30, 33), box_walls("s64", 30, 33, 6)), "no occupied cell",
             lambda c, r: r.criterion == R.NO_CORRESPONDENCES and r.correspondences == 0 and r.pairing.has_home.sum() == 360 and (r.pairing.mi == -1).all()))
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        c.cloud, c.beam = R.cloud(c.scan, LASER)
    return cases


CASES = build()
CASE = {c.name: c for c in CASES}
PLANTS = ("no_half", "tie_high", "early_stop", "chebyshev", "transposed", "w_plus", "w_minus", "centre")
NON_FINITE_GUESSES = ((float("nan"), 0.0, 0.0), (0.1, float("nan"), 0.0), (0.1, 0.0, float("inf")), (float("-inf"), 0.0, 0.0))


def run(c: Case, plant=None, T=None, p=None) -> A.Result:
    return A.align(c.occ(), c.geom, c.cloud, c.beam, c.scan.size, c.T if T is None else T, c.p if p is None else p, plant=plant, **c.icp)


@functools.lru_cache(maxsize=None)
def expected(name) -> A.Result:
    """the restatement's result of a case: computed once, shared, never changed"""
    res = run(CASE[name])
    for a in vars(res.pairing).values():
        a.setflags(write=False)
    return res


def digest(res: A.Result):
    """every bit of a result"""
    if res is None:
        return None
    return (res.ok, tuple(float(v).hex() for v in res.T), res.iterations, res.correspondences, float(res.mse).hex(), res.criterion,
            tuple(a.tobytes() for a in vars(res.pairing).values()))


# ---- behaviour: maps drawn by the oracle's GridMapper (icp_search_map_cases.behaviour_map) ------------------------------------------------
BEHAVIOUR_TRUTH = (0.2, 0.35, 0.22)
BEHAVIOUR_SEED = 19
BEHAVIOUR_STARTS = 12
BEHAVIOUR_ROOMS = ("bench", "survey")


@functools.lru_cache(maxsize=None)
def behaviour(room):
    """-> list of (start error (m, rad), end error (m, rad), iterations, ok) over the room's starts"""
    import icp_search_map_cases as mc
    _, occ, _ = mc.behaviour_map(room)
    scan = mc.behaviour_scan(room, BEHAVIOUR_TRUTH)
    cloud, beam = R.cloud(scan, LASER)
    rng = np.random.default_rng(BEHAVIOUR_SEED)
    th, x, y = BEHAVIOUR_TRUTH
    out = []
    for _ in range(BEHAVIOUR_STARTS):
        d = rng.uniform(-1.0, 1.0, 3) * (0.5 * math.pi / 180.0, 0.025, 0.025)
        T0 = (th + d[0], x + d[1], y + d[2])
        res = A.align(occ, mc.S400, cloud, beam, scan.size, T0, A.Params(), **ICP)
        err = lambda T: (math.hypot(T[1] - x, T[2] - y), abs(T[0] - th))
        out.append((err(T0), err(res.T), res.iterations, res.ok))
    return out


# what test_icp_align_map_cases.py measured: room -> mean / max translation error (mm) and angle error (mrad), of the starts and after
BEHAVIOUR_RECORD = dict(
    bench=dict(start_mm=(14.8, 30.8), end_mm=(0.9, 0.9), start_mrad=(4.5, 7.9), end_mrad=(0.5, 0.5), iterations=(2.7, 3), ok=12),
    survey=dict(start_mm=(14.8, 30.8), end_mm=(1.3, 1.3), start_mrad=(4.5, 7.9), end_mrad=(0.1, 0.1), iterations=(2.3, 3), ok=12))
