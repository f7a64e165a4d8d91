"""numpy restatement of the hypotheses of the global search (include/tbnav_icp.h, HYPOTHESES, items H1-H10), written from the header
alone, by brute force over icp_global_restatement's score and bound volumes: nothing is pruned and there are no bins.  A candidate is a
peak when the sliding maximum of the keys over its window (H3: a box in tx and ty, H3's distance in the heading) is its own key.
Everything is an integer: the kernels reproduce it exactly.

`plant` names a deliberate error (tests/test_icp_hyp_cases.py shows that each changes at least one case): "winners_only" (bins of
(sep_steps + 1) x (sep_cells + 1)^2 candidates, and a bin's winner suppressed only by other bins' winners), "greedy" (candidates taken in
key order, only the peaks already picked suppress), "lt_window" ('<' for '<=' in the window), "nowrap" (wrap ignored), "floor_down" (the
floor rounded down), "tie_high" (ties to the highest index), "skip_eq" (blocks whose bound == t skipped), "bin_angle" (the heading
distance wrapped at the bins' padded heading count instead of NA)."""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

import icp_global_restatement as G
import icp_search_restatement as S

HYP_MAX, MAX_BINS, MAX_REFINE, MAX_CANDIDATES = 64, 1 << 22, 1 << 18, 1 << 20
PLANTS = ("winners_only", "greedy", "lt_window", "nowrap", "floor_down", "tie_high", "skip_eq", "bin_angle")


@dataclass(frozen=True)
class HypParams:
    """tbnav_icp_hyp_params (H1)"""
    max_hyp: int = 8
    floor_q10: int = 768
    sep_cells: int = 8
    sep_steps: int = 10
    wrap: int = 1
    reserved: int = 0

    def with_(self, **kw):
        return replace(self, **kw)


def valid(hp: HypParams) -> bool:
    return (1 <= hp.max_hyp <= HYP_MAX and 1 <= hp.floor_q10 <= 1024 and 0 <= hp.sep_cells <= 64 and 0 <= hp.sep_steps <= G.MAX_ANG
            and hp.wrap in (0, 1) and hp.reserved == 0)


def bins(gp: G.Params, side: int, hp: HypParams) -> int:
    """H1's bin count"""
    _, _, w, h = G.region(gp, side)
    ba, b = hp.sep_steps + 1, hp.sep_cells + 1
    return -(-gp.ang_count // ba) * -(-w // b) * -(-h // b)


def floor_of(best: int, f: int, plant=None) -> int:
    return (best * f) >> 10 if plant == "floor_down" else (best * f + 1023) >> 10


def heading_distance(ia, ib, na: int, hp: HypParams, plant=None):
    d = np.abs(np.asarray(ia) - np.asarray(ib))
    if hp.wrap and plant != "nowrap":
        turn = -(-na // (hp.sep_steps + 1)) * (hp.sep_steps + 1) if plant == "bin_angle" else na
        d = np.minimum(d, turn - d)
    return d


@dataclass
class Hyp:
    """tbnav_icp_hypothesis (H5)"""
    T: tuple
    quality: float
    score: int
    ia: int
    tx: int
    ty: int
    accepted: int


@dataclass
class Result:
    status: str                 # "ok" | "unsupported"
    hyps: list
    info: dict                  # H7 but for refined_blocks and rounds, which are the implementation's
    index: np.ndarray           # the hook's three arrays, ascending index
    score: np.ndarray
    peak: np.ndarray


def _shift_max(vol: np.ndarray, axis: int, sep: int) -> np.ndarray:
    """the maximum over -sep .. sep along a spatial axis, nothing beyond the region"""
    out = vol.copy()
    n = vol.shape[axis]
    for d in range(1, min(sep, n - 1) + 1):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, n - d), slice(d, n)
        lo, hi = tuple(lo), tuple(hi)
        out[lo] = np.maximum(out[lo], vol[hi])
        out[hi] = np.maximum(out[hi], vol[lo])
    return out


def _window_max(keys: np.ndarray, hp: HypParams, plant=None) -> np.ndarray:
    sc, sa = hp.sep_cells, hp.sep_steps
    if plant == "lt_window":
        sc, sa = max(sc - 1, 0), max(sa - 1, 0)
    m = _shift_max(_shift_max(keys, 1, sc), 2, sc)
    na = keys.shape[0]
    out = m.copy()
    for ia in range(na):
        near = np.flatnonzero(heading_distance(ia, np.arange(na), na, hp, plant) <= sa)
        out[ia] = m[near].max(axis=0)
    return out


def _peaks_winners_only(keys, idx, hp: HypParams, na: int):
    """the plant: bins, and winners against winners"""
    ba, b = hp.sep_steps + 1, hp.sep_cells + 1
    win = {}
    for n, (ia, a, c) in enumerate(idx):
        k = (ia // ba, a // b, c // b)
        if k not in win or keys[n] > keys[win[k]]:
            win[k] = n
    w = np.array(sorted(win.values()), dtype=np.int64)
    peak = np.zeros(len(idx), dtype=bool)
    for n in w:
        o = w[w != n]
        inside = ((np.abs(idx[o, 1] - idx[n, 1]) <= hp.sep_cells) & (np.abs(idx[o, 2] - idx[n, 2]) <= hp.sep_cells)
                  & (heading_distance(idx[o, 0], idx[n, 0], na, hp) <= hp.sep_steps))
        peak[n] = not (inside & (keys[o] > keys[n])).any()
    return peak


def _peaks_greedy(keys, idx, hp: HypParams, na: int):
    """the plant: in key order, only what was picked suppresses"""
    peak = np.zeros(len(idx), dtype=bool)
    picked = np.zeros((0, 3), dtype=np.int64)
    for n in np.argsort(keys)[::-1]:
        inside = ((np.abs(picked[:, 1] - idx[n, 1]) <= hp.sep_cells) & (np.abs(picked[:, 2] - idx[n, 2]) <= hp.sep_cells)
                  & (heading_distance(picked[:, 0], idx[n, 0], na, hp) <= hp.sep_steps))
        if not inside.any():
            peak[n] = True
            picked = np.vstack([picked, idx[n:n + 1]])
    return peak


def hypotheses(res: G.Result, geom: G.Geom, gp: G.Params, hp: HypParams = HypParams(), plant=None) -> Result:
    """tbnav_icp_localize_map_hyp and its hook from the global search's restated volumes"""
    assert valid(hp) and G.valid(gp, geom.side)
    side = geom.side
    tx0, ty0, w, h = G.region(gp, side)
    s, nbx, nby, blocks = G.block_grid(gp, side)
    na = gp.ang_count
    scores = res.scores.astype(np.uint64)
    best = int(scores.max())
    info = dict(searched=1, n=0, n_peaks=0, best_score=best, floor_score=0, points=res.info.points, occupied=res.info.occupied,
                blocks=blocks, floor_blocks=0, candidates=0)
    empty = (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint8))
    if bins(gp, side, hp) > MAX_BINS:
        return Result("unsupported", [], {}, *empty)
    if best == 0:
        return Result("ok", [], info, *empty)
    t = floor_of(best, hp.floor_q10, plant)
    floor_blocks = int((res.bounds.astype(np.uint64) >= t).sum())
    exists = scores >= max(t, 1)
    if plant == "skip_eq":
        keep = np.repeat(np.repeat(res.bounds.astype(np.uint64) != t, s, axis=1), s, axis=2)[:, :w, :h]
        exists &= keep
    candidates = int(exists.sum())
    if floor_blocks > MAX_REFINE or candidates > MAX_CANDIDATES:
        return Result("unsupported", [], {}, *empty)
    ia_, a_, b_ = np.meshgrid(np.arange(na), np.arange(w), np.arange(h), indexing="ij")
    index = ((ia_ * side + (tx0 + a_)) * side + (ty0 + b_)).astype(np.uint64)
    low = index if plant == "tie_high" else (~index & np.uint64(0xffffffff))
    keys = np.where(exists, (scores << np.uint64(32)) | low, np.uint64(0))
    if plant in ("winners_only", "greedy"):
        idx = np.argwhere(exists)
        flat = keys[exists]
        pk = (_peaks_winners_only if plant == "winners_only" else _peaks_greedy)(flat, idx, hp, na)
        peak = np.zeros(keys.shape, dtype=bool)
        peak[exists] = pk
    else:
        peak = exists & (_window_max(keys, hp, plant) == keys)
    order = np.argsort(keys[peak])[::-1]
    pidx = np.argwhere(peak)[order]
    hyps = []
    points, occupied = res.info.points, res.info.occupied
    for ia, a, b in pidx[:hp.max_hyp]:
        ia, tx, ty = int(ia), tx0 + int(a), ty0 + int(b)
        sc = int(scores[ia, a, b])
        q = float(sc) / (255.0 * float(points)) if points > 0 else 0.0
        T = (float(ia) * gp.ang_step, geom.xmin + (float(tx) + 0.5) * geom.resolution, geom.ymin + (float(ty) + 0.5) * geom.resolution)
        hyps.append(Hyp(T, q, sc, ia, tx, ty, int(q >= gp.min_quality and points > 0 and occupied > 0)))
    info.update(n=len(hyps), n_peaks=int(peak.sum()), floor_score=t, floor_blocks=floor_blocks, candidates=candidates)
    return Result("ok", hyps, info, index[exists].astype(np.uint32), scores[exists].astype(np.uint32), peak[exists].astype(np.uint8))


def localize_hyp(occ, geom: G.Geom, src, sp: S.Params = S.Params(), gp: G.Params = G.Params(), hp: HypParams = HypParams(), plant=None) -> Result:
    return hypotheses(G.localize(occ, geom, src, sp, gp), geom, gp, hp, plant)
