"""Thirty seeded random cases of the shape of the correlative search's score volume (csrc/icp_search_shape.hip) against its
restatement (tests/icp_search_shape_restatement.py) with ==, drawn by tools/fuzz_icp.py --shape's generator (draw_shape): rooms
and corridors at random headings and widths, the robot's step, the guess's error, the window, slack_q10, drop_q10 and
flat_cells2.  The draw itself is held, on the CPU, to reach every kind: at least 8 cases of kind 1, 1 of kind 2 and 8 of kind 0
among the thirty.  That is a condition on the inputs, not on the code."""
import os
import sys

import pytest

import icp_line_restatement as LR
import icp_restatement as R
import icp_search_shape_restatement as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CASES, SEED = 30, 2031
INFO = ("T", "quality", "score", "points", "candidates", "ia", "iy", "ix", "at_edge", "accepted", "searched")
SHAPE = ("S0", "Sx", "Sy", "Sxx", "Sxy", "Syy", "l1", "l2", "ex", "ey", "T_raw", "cells", "kind", "computed")

sys.path.insert(0, os.path.join(ROOT, "tools"))

_cases = []


def cases():
    """the thirty draws with their restated results, formed once"""
    if not _cases:
        import fuzz_icp
        L = R.lds01()
        for i in range(N_CASES):
            tgt, src, sp, fp, guess, scene = fuzz_icp.draw_shape(i, SEED)
            _cases.append((tgt, src, sp, fp, guess, scene) + F.search(tgt, src, L, guess, sp, fp))
    return _cases


def test_the_draw_reaches_every_kind():
    kinds = [c[7].kind for c in cases()]
    assert len(kinds) == N_CASES
    assert kinds.count(1) >= 8 and kinds.count(2) >= 1 and kinds.count(0) >= 8, kinds
    assert {c[5] for c in cases()} == {"room", "corridor"}


@pytest.mark.gpu
def test_thirty_random_cases_equal_the_restatement(gpu_pkg):
    from rtn_amd import icp
    import fuzz_icp
    L = R.lds01()
    for i, (tgt, src, sp, fp, guess, scene, want, wsh) in enumerate(cases()):
        a = icp.ScanAlignment(icp.default_params(), metric="line", search={f: getattr(sp, f) for f in fuzz_icp.SHAPE_FIELDS},
                              shape=dict(drop_q10=fp.drop_q10, flat_cells2=fp.flat_cells2))
        acc, T, info, sh = a.searchWithShape(guess, tgt, src)
        for f in INFO:
            assert info[f] == getattr(want, f), (i, f, info, want, sp, fp)
        for f in SHAPE:
            assert sh[f] == getattr(wsh, f), (i, f, sh, wsh, sp, fp)
        assert acc == bool(want.accepted) and T == want.T, i
        if i % 3 == 0:                                           # and through the pipeline, with the line metric
            res, _, _ = F.match(tgt, src, L, guess, sp, fp, icp=LR.match, found=(want, wsh))
            ok, Tm, im = a.pclICP(guess, tgt, src)
            assert (ok, tuple(Tm), im["iterations"], im["criterion"]) == (res.ok, tuple(res.T), res.iterations, res.criterion), (i, res)
            assert a.lastSearchShape() == sh, i
        a.close()
