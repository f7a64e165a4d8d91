"""The case table of the hypotheses of the global search (include/tbnav_icp.h, HYPOTHESES H1-H10; csrc/icp_hyp.hip behind
csrc/icp_global.hip), on icp_global_cases' geometries: at most 96 cells a side, 72 headings and q = 1..5 (the two 200-cell refusals score
one point).  tests/test_icp_hyp_cases.py proves on the CPU, on the restatement (tests/icp_hyp_restatement.py), that each case reaches
what its `reaches` names and that each planted error changes a case; tests/test_icp_hyp_gpu.py holds the device to the restatement with
== on every one.

Most cases score ONE point (icp_global_cases.ONE_POINT: the offset (3, 0) at heading 0) at stamp_cells = 1 or 3, so that the score volume
is a shifted copy of lik and a peak stands where a cell is occupied: an occupied cell (i, j) scores 255 at (tx, ty) = (i - 3, j).  With a
step of pi / 2 the headings 0, 4, 8, ... are copies of one another, and in a region of one cell only they score: that places peaks along
the heading axis.  The rectangle and the room are the two maps of the issue that asked for this entry, with its numbers."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

import icp_align_map_restatement as A
import icp_global_cases as gc
import icp_global_restatement as G
import icp_hyp_restatement as H
import icp_restatement as R
import icp_search_restatement as S
import icp_verify_map_restatement as V

LASER = gc.LASER
ONE_POINT = gc.ONE_POINT
HP = H.HypParams
GP = G.Params
QUARTER = math.pi / 2
V5 = gc.V                                    # SP5's stamp by squared distance: 255, 225, 199, ...
L_FREE, L_OCC = -2.0, 2.2


@dataclass
class Case:
    name: str
    size_id: str
    occ: object                  # () -> uint8 [side][side]
    gp: G.Params
    hp: H.HypParams
    scan: np.ndarray
    reaches: str
    check: object                # (case, H.Result, G.Result) -> bool
    sp: object = None
    plants: tuple = ()           # planted errors this case is known to expose

    @property
    def geom(self):
        return gc.geom(self.size_id)

    @property
    def search(self) -> S.Params:
        return self.sp if self.sp is not None else gc.sp_of(self.size_id)

    @functools.cached_property
    def cloud(self):
        return R.cloud(self.scan, LASER)[0]


def _at(r: H.Result):
    return [(y.ia, y.tx, y.ty) for y in r.hyps]


def _is(want, n_peaks=None, **info):
    """the hypotheses are exactly `want`, in that order"""
    def check(c, r, g):
        ok = r.status == "ok" and _at(r) == list(want) and r.info["n_peaks"] == (len(want) if n_peaks is None else n_peaks)
        return ok and all(r.info[k] == v for k, v in info.items())
    return check


def _one(name, where, hp, want, reaches, gp=GP(ang_count=1), size_id="s64", sp=gc.SP_K1, plants=(), n_peaks=None, **info):
    return Case(name, size_id, gc.cells(size_id, where), gp, hp, ONE_POINT, reaches, _is(want, n_peaks, **info), sp=sp, plants=plants)


def _winners_case():
    """One row of candidates (region ty = 30), bins of 4 cells from tx0 = 1: [17..20], [21..24], [25..28].  The occupied cell (27, 30)
    scores 255 at tx = 24, 225 at 23, 155 at 22, 83 at 21; the occupied cell (23, 33) scores 83 at tx = 20.  The floor is 83.  tx = 20 wins
    its bin; the winner of the next bin, tx = 24, lies 4 cells off, outside the window of 3; tx = 23, which is no winner and no peak
    (24 suppresses it), lies inside and beats tx = 20."""
    def check(c, r, g):
        row = g.scores[0, :, 0]
        ok = [int(row[tx - 1]) for tx in (20, 21, 22, 23, 24, 25)] == [V5[9], V5[9], V5[4], V5[1], 255, V5[1]] and r.info["floor_score"] == V5[9]
        return ok and _at(r) == [(0, 24, 30)] and r.info["n_peaks"] == 1 and _at(H.hypotheses(g, c.geom, c.gp, c.hp, "winners_only")) == [(0, 24, 30), (0, 20, 30)]
    return Case("non_winner_suppresses", "s64", gc.cells("s64", ((27, 30), (23, 33))), GP(ang_count=1, region=(1, 30, 40, 30)),
                HP(sep_cells=3, sep_steps=0, floor_q10=332), ONE_POINT,
                "a candidate suppressed by a non-winner (itself suppressed, no peak) of a neighbouring bin whose winner lies outside the window",
                check, sp=gc.SP5, plants=("winners_only",))


def _rect_occ():
    occ = np.zeros((96, 96), dtype=np.uint8)
    occ[8, 14:82] = 1; occ[87, 14:82] = 1; occ[8:88, 14] = 1; occ[8:88, 81] = 1
    return occ


def rect_log_odds():
    """-2.0 strictly inside the walls, +2.2 on the occupied cells, 0 elsewhere"""
    lo = np.zeros((96, 96))
    lo[9:87, 15:81] = L_FREE
    lo[_rect_occ() != 0] = L_OCC
    return lo


def room_log_odds():
    """-2.0 on rows 4..90 x columns 3..91, +2.2 on the occupied cells, 0 elsewhere"""
    lo = np.zeros((96, 96))
    lo[4:91, 3:92] = L_FREE
    lo[gc.room("s96")() != 0] = L_OCC
    return lo


RECT_POSE, ROOM_POSE = (0.7, 0.675, -0.425), (0.7, 0.45, -0.3)
GP72 = GP(ang_count=72, ang_step=math.pi / 36)
HP_ISSUE = HP(sep_steps=2)                   # f = 768, sep_cells 8, sep_steps 2


def build():
    out = []
    add = out.append
    top = HP(floor_q10=1024, sep_steps=0)
    # ---- separation edges, ties
    add(_one("sep_tx_in", ((20, 30), (28, 30)), top, [(0, 17, 30)], "two equal maxima exactly sep_cells apart in tx: the lowest index survives",
             plants=("lt_window", "tie_high"), candidates=2))
    add(_one("sep_tx_out", ((20, 30), (28, 30)), top.with_(sep_cells=7), [(0, 17, 30), (0, 25, 30)], "sep_cells + 1 apart in tx: both, lowest first",
             plants=("tie_high",)))
    add(_one("sep_ty_in", ((20, 30), (20, 38)), top, [(0, 17, 30)], "exactly sep_cells apart in ty", plants=("lt_window",)))
    add(_one("sep_ty_out", ((20, 30), (20, 38)), top.with_(sep_cells=7), [(0, 17, 30), (0, 17, 38)], "sep_cells + 1 apart in ty"))
    add(_one("plateau", tuple((20, j) for j in range(10, 41)), top, [(0, 17, 10)], "a plateau of 31 equal scores, longer than a window: one peak",
             plants=("greedy", "tie_high"), candidates=31))
    # ---- headings: the region is the one cell that scores 255 at the headings 0, 4, 8, ...
    cell = ((23, 30),)
    one = dict(region=(20, 30, 20, 30), ang_step=QUARTER)
    add(_one("sep_ia_in", cell, top.with_(sep_steps=4, wrap=0), [(0, 20, 30)], "two maxima exactly sep_steps apart in heading", gp=GP(ang_count=8, **one),
             plants=("lt_window",), candidates=2))
    add(_one("sep_ia_out", cell, top.with_(sep_steps=3, wrap=0), [(0, 20, 30), (4, 20, 30)], "sep_steps + 1 apart in heading", gp=GP(ang_count=8, **one)))
    add(_one("wrap_on", cell, top.with_(sep_steps=2), [(0, 20, 30)], "headings 0 and 4 of 6: two steps apart across the wrap", gp=GP(ang_count=6, **one),
             plants=("nowrap",), candidates=2))
    add(_one("wrap_off", cell, top.with_(sep_steps=2, wrap=0), [(0, 20, 30), (4, 20, 30)], "the same with wrap = 0: both survive", gp=GP(ang_count=6, **one)))
    add(_one("wrap_ragged_bin", cell, top.with_(sep_steps=3), [(0, 20, 30)],
             "NA = 6 is no multiple of sep_steps + 1 = 4: the pair across the wrap, the second in the ragged last angular bin; NA <= 2 * sep_steps + 1",
             gp=GP(ang_count=6, **one), plants=("nowrap", "bin_angle"), candidates=2))
    add(_one("wrap_whole_turn", cell, top.with_(sep_steps=2), [(0, 20, 30)], "NA = 5 = 2 * sep_steps + 1: a window is the whole turn",
             gp=GP(ang_count=5, **one), plants=("nowrap",), candidates=2))
    add(_one("plateau_heading", cell, top.with_(sep_steps=1, wrap=0), [(0, 20, 30)], "a plateau along the heading (ang_step = 0: 12 equal headings)",
             gp=GP(ang_count=12, region=(20, 30, 20, 30), ang_step=0.0), plants=("greedy",), candidates=12))
    # ---- winners against winners
    add(_winners_case())
    # ---- the floor: best = 255; f = 900 gives t = 225, f = 904 gives t = 226 and 255 * 904 >> 10 = 225
    rival = ((40, 30), (2, 12))              # (2, 12) would score 255 at tx = -1, outside the map: 225 at (0, 12), and that block's bound is 225
    add(_one("floor_equal", rival, HP(floor_q10=900, sep_steps=0), [(0, 37, 30), (0, 0, 12)],
             "a rival with score == t, in a block whose bound == t, at the map's edge where the window is cut", sp=gc.SP5, plants=("skip_eq",),
             floor_score=225))
    add(_one("floor_below", rival, HP(floor_q10=904, sep_steps=0), [(0, 37, 30)], "a rival with score == t - 1; the floor rounds up", sp=gc.SP5,
             plants=("floor_down",), floor_score=226))
    add(_one("floor_1024", rival, HP(floor_q10=1024, sep_steps=0), [(0, 37, 30)], "f = 1024: t = best", sp=gc.SP5, floor_score=255, candidates=1))
    add(Case("floor_1", "s64", gc.cells("s64", rival), GP(ang_count=1), HP(floor_q10=1, sep_steps=0, sep_cells=64), ONE_POINT,
             "f = 1: t = 1, every candidate that scores; a window as wide as the map",
             lambda c, r, g: r.info["floor_score"] == 1 and r.info["candidates"] == int((g.scores > 0).sum()) and _at(r) == [(0, 37, 30)], sp=gc.SP5))
    # ---- K, and no separation at all
    blob = ((30, 30), (30, 44))
    n_blob = 2 * 49
    for k, name in ((1, "k_1"), (5, "k_below_peaks"), (64, "k_64")):
        add(Case(name, "s64", gc.cells("s64", blob), GP(ang_count=1), HP(max_hyp=k, floor_q10=1, sep_cells=0, sep_steps=0), ONE_POINT,
                 f"K = {k} of {n_blob} peaks; sep_cells = sep_steps = 0: every candidate at the floor is a peak",
                 lambda c, r, g, k=k: r.info["n"] == k == len(r.hyps) and r.info["n_peaks"] == r.info["candidates"] == n_blob and bool(r.peak.all())
                 and _at(r)[0] == (0, 27, 30), sp=gc.SP5))
    # ---- regions, ragged blocks, empties
    add(Case("region_ragged", "s44", gc.room("s44"), GP(ang_count=4, ang_step=QUARTER, region=(3, 5, 37, 40)), HP(floor_q10=600, sep_cells=5, sep_steps=0),
             gc.scan_in(gc.room("s44")(), gc.geom("s44"), (0.0, 0.1, -0.2), keep=gc.spread(90)),
             "a region with an odd origin, ragged blocks and ragged bins, windows cut by its edge",
             lambda c, r, g: r.status == "ok" and r.info["n_peaks"] >= 2 and g.bounds.shape == (4, 5, 5) and 35 % 8 != 0 and 35 % 6 != 0))
    add(Case("no_valid_beam", "s64", gc.room("s64"), GP(ang_count=4), HP(), np.full(360, 0.05, dtype=np.float32), "no valid point: empty, no error",
             lambda c, r, g: r.status == "ok" and r.hyps == [] and r.info["points"] == 0 and r.info["n"] == r.info["n_peaks"] == r.info["candidates"] == 0))
    add(Case("empty_map", "s64", gc.cells("s64", ()), GP(ang_count=4), HP(), gc.scan_in(gc.room("s64")(), gc.geom("s64"), (0.0, 0.0, 0.0), keep=gc.spread(90)),
             "an empty map: empty, no error", lambda c, r, g: r.status == "ok" and r.hyps == [] and r.info["occupied"] == 0 and r.info["points"] == 90))
    # ---- the two maps this entry was asked for
    add(Case("rectangle", "s96", _rect_occ, GP72, HP_ISSUE, gc.scan_in(_rect_occ(), gc.geom("s96"), RECT_POSE),
             "a point-symmetric rectangle: two hypotheses of the same score, the truth and its mirror image, the lower index first",
             lambda c, r, g: _at(r) == [(8, 61, 39), (44, 34, 56)] and [y.score for y in r.hyps] == [90780, 90780] and r.info["n_peaks"] == 2,
             plants=("tie_high",)))
    add(Case("room", "s96", gc.room("s96"), GP72, HP_ISSUE, gc.scan_in(gc.room("s96")(), gc.geom("s96"), ROOM_POSE),
             "a room with no symmetry: the truth and the rectangle's three other rotations, in that order",
             lambda c, r, g: _at(r)[0] == (8, 57, 42) and [y.score for y in r.hyps] == [84661, 71468, 68630, 66225] and r.info["n_peaks"] == 4
             and all(y.accepted for y in r.hyps)))
    return out


CASES = build()
CASE = {c.name: c for c in CASES}
assert all(len(c.cloud) <= 360 and c.geom.side <= 96 and c.gp.ang_count <= 72 for c in CASES)


@functools.lru_cache(maxsize=None)
def volumes(name) -> G.Result:
    """the global search's restated volumes of a case: computed once, shared, never changed"""
    c = CASE[name]
    res = G.localize(c.occ(), c.geom, c.cloud, c.search, c.gp)
    for a in (res.lik, res.pool, res.bounds, res.scores):
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def expected(name) -> H.Result:
    c = CASE[name]
    return H.hypotheses(volumes(name), c.geom, c.gp, c.hp)


# ---- the refusals of H1 and H6 --------------------------------------------------------------------------------------------------------
G200 = G.Geom(-5.0, -5.0, 0.05, 200)
FULL_200 = functools.lru_cache(maxsize=None)(lambda: np.ones((200, 200), dtype=np.uint8))
BAD_PARAMS = (dict(max_hyp=0), dict(max_hyp=65), dict(floor_q10=0), dict(floor_q10=1025), dict(sep_cells=-1), dict(sep_cells=65), dict(sep_steps=-1),
              dict(sep_steps=721), dict(wrap=2), dict(wrap=-1), dict(reserved=1))
# a fully occupied 200 x 200 map, one point, 72 headings: 720 000 blocks at q = 1, all with bound 255 = t; at q = 5, 3528 blocks and
# 2.88e6 candidates
REFUSED = (("floor_blocks", GP(ang_count=72, ang_step=math.pi / 36, pool_log2=1), HP()),
           ("candidates", GP(ang_count=72, ang_step=math.pi / 36, pool_log2=5), HP()))
# bins: 72 headings x 200 x 200 cells with no separation at all are 2.88e6 bins <= 2^22; a 96-cell map cannot reach the limit, so the
# limit is met on the 200-cell map with 720 headings
BINS_GP, BINS_HP = GP(ang_count=720, ang_step=math.pi / 360, pool_log2=5), HP(sep_cells=0, sep_steps=0)


# ---- behaviour: the restated chain -------------------------------------------------------------------------------------------------------
def chain(lo, occ, geom, scan, gp, hp, even_if_rejected=False, align=A.Params(), verify=V.Params(), sp=gc.SP5):
    """relocalizeMapHypotheses restated: this restatement, icp_align_map_restatement.align and icp_verify_map_restatement.verify"""
    cloud, beam = R.cloud(scan, LASER)
    res = H.localize_hyp(occ, geom, cloud, sp, gp, hp)
    classes = V.Classes.from_log_odds(lo, occ)
    out = []
    for y in res.hyps:
        rec = dict(found=y, fine=None, check=None, T=y.T, verified=False)
        if y.accepted or even_if_rejected:
            fine = A.align(occ, geom, cloud, beam, len(scan), y.T, align)
            rec["fine"] = fine
            rec["T"] = tuple(fine.T) if fine.ok else y.T
            chk = V.verify(classes, geom, cloud, beam, len(scan), rec["T"], verify)
            rec["check"] = chk.info
            rec["verified"] = bool(chk.info["accepted"])
        out.append(rec)
    ver = [i for i, o in enumerate(out) if o["verified"]]
    best = ver[0] if ver else -1
    T = out[best]["T"] if ver else (out[0]["T"] if out else None)
    return dict(hypotheses=out, info=res.info, verified_count=len(ver), best=best, ambiguous=len(ver) > 1, T=T)


@functools.lru_cache(maxsize=None)
def behaviour(which):
    """-> (log-odds, occupancy, scan, the restated chain's result) of "rectangle" or "room", under the defaults with f = 768, sep_steps 2"""
    c = CASE[which]
    lo = rect_log_odds() if which == "rectangle" else room_log_odds()
    occ = c.occ()
    return lo, occ, c.scan, chain(lo, occ, c.geom, c.scan, c.gp, c.hp)
