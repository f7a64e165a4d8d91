"""The case table of the global search (include/tbnav_icp.h, GLOBAL SEARCH L1-L10; csrc/icp_global.hip): the smallest maps, scans and
parameters at which the field, pooling, offset, bound and refinement kernels and the pruning round them can still go wrong.
tests/test_icp_global_cases.py proves on the CPU, on the exhaustive restatement, that each case reaches what its `reaches` names, that
no bound falls below a score, and that each planted error changes a case; tests/test_icp_global_gpu.py holds the device to the
restatement with == on every one.

Maps: side 64 (2 x 2 tiles of the filter's pool), 96 (3 x 3), 72 (a ragged last tile of 8) and 44 (a ragged tile AND, at s = 8, a ragged
block) at 0.05 m, and 24 cells of 0.5 m.  No case has more than 96 cells a side, 72 headings or 360 points.

BEHAVIOUR (measured on the restatement): a 96 x 96 map drawn by the oracle's GridMapper from 8 scans of ROOM_BENCH (1 cm range noise)
along rbpf_cases.trajectory from BEHAVIOUR_START, in the room's lower left corner: 271 occupied cells.  The walls at x = 2.2 and y = 2.0
are further than the laser's 3.5 m from there and are missing or partly drawn, which is what tells the pose from its mirror image
through the room's centre (a finished rectangle looks the same from both: L10).  The scan is taken at BEHAVIOUR_TRUTH, 1.38 m from the
nearest pose that drew the map; 72 headings of 5 degrees, q = 3, no guess.  Found to the cell and the step at quality 0.644 (the scan
sees the walls the map lacks; the best block elsewhere 0.564); 3 of 10 368 blocks have a bound that reaches the best score."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

import icp_global_restatement as G
import icp_restatement as R
import icp_search_restatement as S
import rbpf_cases as rc

LASER = R.lds01()
SIDES = {"s64": (64, 0.05, 1.6), "s96": (96, 0.05, 2.4), "s72": (72, 0.05, 1.8), "s44": (44, 0.05, 1.1), "r24": (24, 0.5, 6.0)}   # side, cell, half
SP5 = S.Params(sigma=0.1)                                                                   # 0.05 m cells, k = 3
SP50 = S.Params(resolution=0.5, half_extent=7.9, sigma=0.7, stamp_cells=3)                  # 0.5 m cells
SP_K1 = S.Params(sigma=0.05, stamp_cells=1)
assert S.valid(SP5) and S.valid(SP50) and S.valid(SP_K1)


def geom(size_id) -> G.Geom:
    side, res, half = SIDES[size_id]
    assert math.ceil((half - -half) / res) == side
    return G.Geom(-half, -half, res, side)


def sp_of(size_id) -> S.Params:
    return SP50 if size_id == "r24" else SP5


def cells(size_id, where):
    def make():
        occ = np.zeros((SIDES[size_id][0],) * 2, dtype=np.uint8)
        for i, j in where:
            occ[i, j] = 1
        return occ
    return make


def room(size_id):
    """walls a few cells inside the map, a box and a partition: no symmetry"""
    def make():
        n = SIDES[size_id][0]
        occ = np.zeros((n, n), dtype=np.uint8)
        a, b, c, d = 3, n - 5, 2, n - 4
        occ[a, c:d + 1] = 1; occ[b, c:d + 1] = 1; occ[a:b + 1, c] = 1; occ[a:b + 1, d] = 1
        occ[a + n // 4:a + n // 4 + n // 8, c + n // 5:c + n // 5 + n // 6] = 1           # the box
        occ[b - n // 3, c:c + n // 3] = 1                                                 # the partition
        return occ
    return make


def scan_in(occ, g: G.Geom, pose, n_beams=360, keep=None, step=0.2):
    """ranges a lidar at pose = (theta, x, y) sees in the occupancy (a ray marched in steps of `step` cells); keep: the beams that
    stay valid, the others are set below range_min"""
    th, x, y = pose
    r = np.full(n_beams, 0.05, dtype=np.float64)
    ang = th + np.deg2rad(360.0 / n_beams) * np.arange(n_beams)
    d = np.arange(0.13 / g.resolution, 3.4 / g.resolution, step) * g.resolution
    for i in range(n_beams):
        ci = np.floor((x + d * math.cos(ang[i]) - g.xmin) / g.resolution).astype(int)
        cj = np.floor((y + d * math.sin(ang[i]) - g.ymin) / g.resolution).astype(int)
        inside = (ci >= 0) & (ci < g.side) & (cj >= 0) & (cj < g.side)
        hit = np.zeros(d.size, dtype=bool)
        hit[inside] = occ[ci[inside], cj[inside]] != 0
        if hit.any():
            r[i] = d[int(np.argmax(hit))]
    if keep is not None:
        mask = np.zeros(n_beams, dtype=bool)
        mask[np.asarray(keep)] = True
        r[~mask] = 0.05
    return r.astype(np.float32)


def spread(n, n_beams=360):
    """n beam indices spread over the turn"""
    return (np.arange(n) * n_beams) // n


ONE_POINT = np.full(360, 0.05, dtype=np.float32)
ONE_POINT[0] = 0.125            # beam 0 looks along x: the point (0.125, 0) exactly, 2.5 cells of 0.05 m


@dataclass
class Case:
    name: str
    size_id: str
    occ: object                  # () -> uint8 [side][side]
    gp: G.Params
    scan: np.ndarray
    reaches: str
    check: object                # (case, Result) -> bool: the proof that the case reaches what it names
    sp: object = None
    plants: tuple = ()           # planted errors this case is known to expose

    @property
    def geom(self):
        return geom(self.size_id)

    @property
    def search(self) -> S.Params:
        return self.sp if self.sp is not None else sp_of(self.size_id)

    @functools.cached_property
    def cloud(self):
        return R.cloud(self.scan, LASER)[0]


def _points(n):
    return lambda c, r: r.info.points == n and len(c.cloud) == n


def _found(c, r):
    return r.info.score > 0 and r.occupied > 0


def _room_case(name, size_id, gp, pose, reaches, check=_found, keep=None, n_beams=360, plants=()):
    occ = room(size_id)
    return Case(name, size_id, occ, gp, scan_in(occ(), geom(size_id), pose, n_beams, keep), reaches, check, plants=plants)


V = [int(math.floor(255.0 * math.exp(-(d2 * 0.0025 / (2.0 * 0.01))) + 0.5)) for d2 in range(19)]     # SP5's stamp by d2
assert V[0] == 255 and V[4] > V[9] > V[18] > 0


def _copies(first):
    """One point with offset (3, 0), region rows 0 .. 31, columns 0 .. 27 (the last block is ragged: columns 24 .. 27, its pool
    reaching 31).  Two copies of one occupied cell 16 columns apart, two rows beyond the rows any candidate reads: both blocks have
    bound == score == V[4].  The decoy: an occupied cell at column 30, three columns beyond the region: its block's bound is 255, the
    largest, and its exact best V[9]."""
    rows = (1, 0) if first else (36, 31)          # the copies' row, and the candidates' row that reads two rows from it
    occ = cells("s64", ((rows[0], 4), (rows[0], 20), (13, 30)))

    def check(c, r):
        s, nbx, nby, _ = G.block_grid(c.gp, 64)
        bx = rows[1] // s
        mx = G.block_maxima(r.scores, s)[0]
        b = r.bounds[0]
        ok = b[bx, 0] == mx[bx, 0] == V[4] and b[bx, 2] == mx[bx, 2] == V[4] and r.info.score == V[4]
        ok &= b[1, 3] == 255 == b.max() and int((b == 255).sum()) == 1 and mx[1, 3] == V[9]
        ok &= (r.info.tx, r.info.ty) == (rows[1], 4) and r.survivors == 3
        ok &= (bx * nby + 0 < 1 * nby + 3) == first
        return bool(ok)
    return Case("copies_before_decoy" if first else "copies_after_decoy", "s64", occ, G.Params(ang_count=1, region=(0, 0, 31, 27)), ONE_POINT,
                "bound == score in two blocks, a decoy block with the largest bound and a lower best", check, plants=("tie_high",))


def build():
    P = G.Params
    out = []
    add = out.append
    add(_room_case("s64_q3_na8", "s64", P(ang_count=8, ang_step=math.pi / 4), (0.0, 0.31, -0.42), "2 x 2 tiles, 8 x 8 blocks, 360 points",
                   lambda c, r: _found(c, r) and r.info.points >= 300, plants=("centred", "transposed")))
    add(_room_case("s96_q5_na4", "s96", P(ang_count=4, ang_step=math.pi / 2, pool_log2=5), (math.pi / 2, -0.6, 0.45), "3 x 3 tiles, s = 32",
                   lambda c, r: _found(c, r) and r.bounds.shape == (4, 3, 3), keep=spread(120)))
    add(_room_case("s72_q2_step", "s72", P(ang_count=4, ang_step=0.7, pool_log2=2), (1.4, 0.2, 0.3), "a ragged tile, s = 4, a step that does not divide the turn",
                   lambda c, r: _found(c, r) and r.info.ia == 2, keep=spread(90)))
    add(_room_case("s44_q3_ragged", "s44", P(ang_count=4, ang_step=math.pi / 2), (0.0, 0.1, -0.2), "a ragged tile and a ragged block",
                   lambda c, r: _found(c, r) and r.bounds.shape == (4, 6, 6) and 44 % 8 == 4, keep=spread(90)))
    add(_room_case("r24_q1_na8", "r24", P(ang_count=8, ang_step=math.pi / 4, pool_log2=1), (math.pi / 4, 0.7, -0.4), "0.5 m cells, s = 2",
                   lambda c, r: _found(c, r) and r.bounds.shape == (8, 12, 12), keep=spread(72)))
    add(_room_case("na1", "s64", P(ang_count=1), (0.0, -0.3, 0.4), "one heading", _found, keep=spread(60)))
    add(_room_case("na72", "s64", P(ang_count=72, ang_step=math.pi / 36), (math.pi / 36 * 50, 0.35, 0.25), "72 headings",
                   lambda c, r: _found(c, r) and abs(r.info.ia - 50) <= 1, keep=spread(65)))
    add(_room_case("region_odd", "s64", P(ang_count=4, ang_step=math.pi / 2, region=(5, 7, 37, 29)), (0.0, -0.4, -0.5), "a region with an odd origin",
                   lambda c, r: _found(c, r) and r.scores.shape == (4, 33, 23) and r.bounds.shape == (4, 5, 3), keep=spread(90)))
    add(_room_case("region_one_cell", "s64", P(ang_count=4, ang_step=math.pi / 2, region=(22, 19, 22, 19)), (0.0, -0.475, -0.625), "a region of one cell",
                   lambda c, r: r.scores.shape == (4, 1, 1) and r.info.blocks == 4 and (r.info.tx, r.info.ty) == (22, 19) and r.info.score > 0,
                   keep=spread(90)))
    for n in (1, 63, 64, 65):
        add(_room_case(f"points_{n}", "s64", P(ang_count=4, ang_step=math.pi / 2), (0.0, 0.31, -0.42), f"{n} valid points", _points(n), keep=spread(n)))
    add(_room_case("points_360", "s64", P(ang_count=2, ang_step=math.pi), (0.0, 0.0, 0.0), "360 valid points", _points(360)))
    add(Case("no_valid_beam", "s64", room("s64"), P(ang_count=4), np.full(360, 0.05, dtype=np.float32), "no valid beam: the first candidate, rejected",
             lambda c, r: r.info.points == 0 and (r.info.ia, r.info.tx, r.info.ty, r.info.score, r.info.accepted) == (0, 0, 0, 0, 0)))
    add(Case("no_valid_beam_region", "s64", room("s64"), P(ang_count=4, region=(9, 3, 20, 30)), np.full(360, 0.05, dtype=np.float32),
             "no valid beam in a region: its first candidate", lambda c, r: (r.info.ia, r.info.tx, r.info.ty, r.info.accepted) == (0, 9, 3, 0)))
    add(Case("empty_map", "s64", cells("s64", ()), P(ang_count=4), scan_in(room("s64")(), geom("s64"), (0.0, 0.0, 0.0), keep=spread(90)),
             "an empty map: every score 0, the first candidate, rejected",
             lambda c, r: r.occupied == 0 and r.info.points == 90 and (r.info.ia, r.info.tx, r.info.ty, r.info.score, r.info.accepted) == (0, 0, 0, 0, 0)))
    ring = scan_in(room("s64")(), geom("s64"), (0.0, 0.31, -0.42), keep=spread(40))
    add(Case("cell_0_0", "s64", cells("s64", ((0, 0),)), P(ang_count=2, ang_step=math.pi), ring, "one occupied cell at (0, 0)",
             lambda c, r: r.occupied == 1 and r.lik[0, 0] == 255 and r.lik[3, 3] == V[18] and r.lik[4, 0] == 0 and r.pool[0, 0] == 255 and r.info.score > 0,
             plants=("outside",)))
    add(Case("cell_last", "s64", cells("s64", ((63, 63),)), P(ang_count=2, ang_step=math.pi), ring, "one occupied cell at (side - 1, side - 1)",
             lambda c, r: r.occupied == 1 and r.lik[63, 63] == 255 and r.lik[60, 60] == V[18] and r.pool[63 + 7, 63 + 7] == 255 and r.pool[52 + 7, 63 + 7] == 0
             and r.info.score > 0))
    seams = ((31, 7), (32, 20), (9, 31), (22, 32), (5, 0), (6, 31), (40, 32), (41, 63), (63, 0), (0, 63))
    add(Case("seams", "s64", cells("s64", seams), P(ang_count=4, ang_step=math.pi / 2, pool_log2=2), ring,
             "occupied cells either side of tile and word seams, at bit offsets 0 and 31",
             lambda c, r: r.occupied == len(seams) and all(r.lik[i, j] == 255 for i, j in seams) and r.lik[31, 8] == V[1] and r.lik[33, 20] == V[1]))
    add(Case("seams_k1", "s64", cells("s64", seams), P(ang_count=4, ang_step=math.pi / 2, pool_log2=1), ring, "the same at k = 1",
             lambda c, r: r.lik[31, 9] == 0 and r.lik[30, 6] > 0 and r.lik[29, 7] == 0, sp=SP_K1))
    far = scan_in(room("s64")(), geom("s64"), (0.0, 0.31, -0.42), keep=spread(30)).copy()
    far[5::12] = 3.45            # 69 cells: further than the map is wide
    add(Case("offsets_leave", "s64", room("s64"), P(ang_count=4, ang_step=math.pi / 2), far, "points whose offsets leave the map for every cell",
             lambda c, r: _found(c, r) and int((np.hypot(c.cloud[:, 0], c.cloud[:, 1]) > 3.4).sum()) == 30))
    # (the cell of the world position xmin + (tx + 0.5) * 0.05 + 0.125 is tx + 2, not tx + 3, at tx = 0, 1, 5 and 10: "per_cell")
    add(Case("half_cell", "s64", cells("s64", ((30, 30), (8, 30))), P(ang_count=1), ONE_POINT, "a rotated coordinate exactly on x.5 cells: the rounding rule",
             lambda c, r: float(c.cloud[0, 0]) * (1.0 / 0.05) == 2.5 and r.info.points == 1 and (r.info.score, r.info.tx, r.info.ty) == (255, 5, 30)
             and r.scores[0, 27, 30] == 255 and r.scores[0, 28, 30] == V[1],
             plants=("nohalf", "per_cell")))
    add(_copies(True))
    add(_copies(False))
    return out


CASES = build()
CASE = {c.name: c for c in CASES}
PLANTS = ("centred", "nohalf", "transposed", "tie_high", "outside", "per_cell")
assert all(len(c.cloud) <= 360 and c.geom.side <= 96 and c.gp.ang_count <= 72 for c in CASES)


@functools.lru_cache(maxsize=None)
def expected(name) -> G.Result:
    """the restatement's result of a case: computed once, shared, never changed"""
    c = CASE[name]
    res = G.localize(c.occ(), c.geom, c.cloud, c.search, c.gp)
    for a in (res.lik, res.pool, res.bounds, res.scores):
        a.setflags(write=False)
    return res


# ---- behaviour: a map drawn by the oracle's GridMapper -----------------------------------------------------------------------------------
S96 = geom("s96")
BEHAVIOUR_SCANS, BEHAVIOUR_SEED = 8, 7
BEHAVIOUR_START = (0.0, -1.6, -1.4)
BEHAVIOUR_TRUTH = (4.03, -0.53, -0.31)          # on neither a cell centre nor an angle step
BEHAVIOUR_GP = G.Params(ang_count=72, ang_step=math.pi / 36)
BEHAVIOUR_SHARE = 0.01                          # the blocks whose bound reaches the best score: at most this share of all blocks


@functools.lru_cache(maxsize=None)
def behaviour_map():
    """-> (log-odds [96][96] as the oracle's GridMapper holds them, occupancy uint8 [96][96], the poses that drew it)"""
    import oracle_api as orc
    _, poses = rc.trajectory(BEHAVIOUR_SCANS, rc.TRAJ_BENCH, start=BEHAVIOUR_START)
    rng = np.random.default_rng(BEHAVIOUR_SEED)
    g = orc.GridAPI("orc", grid=(0.05, -2.4, 2.4, -2.4, 2.4))
    assert (g.xsize, g.ysize) == (96, 96)
    for pose in poses:
        g.integrate_scan(orc.room_scan(tuple(pose), walls=rc.ROOM_BENCH, rng=rng), tuple(pose), esdf=False)
    lo = g.dump()["log_odds"].reshape(96, 96).copy()
    occ = np.zeros(96 * 96, dtype=np.uint8)
    occ[g.occ_cells()] = 1
    g.close()
    return lo, occ.reshape(96, 96), poses


def behaviour_scan(seed=11):
    import oracle_api as orc
    return orc.room_scan(BEHAVIOUR_TRUTH, walls=rc.ROOM_BENCH, rng=np.random.default_rng(seed))


@functools.lru_cache(maxsize=None)
def behaviour_result() -> G.Result:
    _, occ, _ = behaviour_map()
    return G.localize(occ, S96, R.cloud(behaviour_scan(), LASER)[0], SP5, BEHAVIOUR_GP)
