"""numpy restatement of the wide second stage of the correlative search (include/tbnav_icp.h, CORRELATIVE SEARCH, items W1-W8) on top
of icp_search_restatement and icp_search_shape_restatement: an addition with no counterpart in the reference, so the header's
items are its whole specification and this file spells them out.

The wide stage is S5, S6 and S7 with wl := W and wa := A: icp_search_restatement scores any window (only its valid() knows the
first stage's limits), so the wide stage here is that file's scores_of_clouds / search_clouds with
Params.with_(lin_cells=W, ang_steps=A).  There is no tolerance.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import icp_restatement as R
import icp_search_restatement as S
import icp_search_shape_restatement as F

MAX_LIN, MAX_ANG, MAX_TABLE = 64, 180, 176
ON_REJECT, ON_REJECT_OR_EDGE, ALWAYS = 0, 1, 2


@dataclass(frozen=True)
class WideParams:
    """tbnav_icp_search_wide_params with tbnav_icp_default_search_wide_params' values"""
    lin_cells: int = 48
    ang_steps: int = 45
    when: int = ON_REJECT

    def with_(self, **kw):
        return replace(self, **kw)


def valid(wp: WideParams, p: S.Params = S.Params()) -> bool:
    """W1's limits and its three conditions against the search parameters p"""
    if not (1 <= wp.lin_cells <= MAX_LIN and 0 <= wp.ang_steps <= MAX_ANG and wp.when in (ON_REJECT, ON_REJECT_OR_EDGE, ALWAYS)):
        return False
    return wp.lin_cells >= p.lin_cells and wp.ang_steps >= p.ang_steps and S.side(p) <= MAX_TABLE


def window(p: S.Params, wp: WideParams) -> S.Params:
    """the first stage's parameters with wl := W, wa := A (W4)"""
    return p.with_(lin_cells=wp.lin_cells, ang_steps=wp.ang_steps)


NOT_SEARCHED = S.Info((0.0, 0.0, 0.0), 0.0, 0, 0, 0, 0, 0, 0, 0, 0, searched=0)


def runs(first: S.Info, when: int) -> bool:
    """W3"""
    return when == ALWAYS or not first.accepted or (when == ON_REJECT_OR_EDGE and bool(first.at_edge))


@dataclass
class Outcome:
    """W5: what tbnav_icp_last_search (info), tbnav_icp_last_search_shape (shape, None: none was formed) and
    tbnav_icp_last_search_wide (first, ran) return"""
    info: S.Info
    first: S.Info
    ran: int
    shape: object = None


def _stage(tgt, src, T_init, p: S.Params, shape_params, scores=None):
    if scores is None:
        scores = S.scores_of_clouds(tgt, src, T_init, p)
    info = S.search_clouds(tgt, src, T_init, p, scores=scores)
    if shape_params is None:
        return info, None
    sh = F.shape(scores, info, p, shape_params)                # W6: F1-F6 with this stage's wl
    return F.shaped(info, sh, T_init, p), sh


def search_clouds(tgt, src, T_init, p: S.Params, wp: WideParams, shape_params=None, first_scores=None, wide_scores=None) -> Outcome:
    """W2-W6 on explicit clouds; first_scores / wide_scores: the stages' volumes, when the caller has them already"""
    assert valid(wp, p), (wp, p)
    if wp.when == ALWAYS:
        first, shape = NOT_SEARCHED, None
    else:
        first, shape = _stage(tgt, src, T_init, p, shape_params, first_scores)
    if not runs(first, wp.when):
        return Outcome(first, first, 0, shape)
    info, shape = _stage(tgt, src, T_init, window(p, wp), shape_params, wide_scores)
    return Outcome(info, first, 1, shape)


def search(target_scan, source_scan, laser: R.Laser, T_init, p: S.Params = S.Params(), wp: WideParams = WideParams(),
           Trs=(0.0, 0.0, 0.0), shape_params=None, **kw) -> Outcome:
    """tbnav_icp_search on a handle with the wide stage on"""
    tgt, _ = R.cloud(target_scan, laser, Trs)
    src, _ = R.cloud(source_scan, laser, Trs)
    return search_clouds(tgt, src, T_init, p, wp, shape_params, **kw)


def wide_scores(target_scan, source_scan, laser: R.Laser, T_init, p: S.Params = S.Params(), wp: WideParams = WideParams(),
                Trs=(0.0, 0.0, 0.0)):
    """W8: tbnav_icp_search_wide_scores -> (Info, the volume uint32 [2A+1][2W+1][2W+1])"""
    pw = window(p, wp)
    sc = S.scores(target_scan, source_scan, laser, T_init, pw, Trs)
    return S.search(target_scan, source_scan, laser, T_init, pw, Trs, scores=sc), sc


def match(target_scan, source_scan, laser: R.Laser, T_init, p: S.Params = S.Params(), wp: WideParams = WideParams(),
          Trs=(0.0, 0.0, 0.0), icp=R.match, shape_params=None, outcome=None, **kw):
    """S8 with "the outcome" for "the search" (W5): the ICP from the outcome's T when it is accepted and from T_init unchanged
    otherwise -> (the ICP's Result, Outcome)"""
    if outcome is None:
        outcome = search(target_scan, source_scan, laser, T_init, p, wp, Trs, shape_params)
    start = outcome.info.T if outcome.info.accepted else tuple(float(v) for v in T_init)
    return icp(target_scan, source_scan, laser, start, Trs=Trs, **kw), outcome
