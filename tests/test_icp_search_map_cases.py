"""CPU proof that the map search's case table (tests/icp_search_map_cases.py) reaches what it names, on the restatement
(tests/icp_search_map_restatement.py): every case's own check; the property the kernel's nearest-cell form stands on (S3's stamp is a
function of d2 that never rises) for every parameter set used and over a sweep; each planted error changes at least one case; the
sizes, origins and parameters the table is meant to cover are in it; and the behaviour cases on maps drawn by the oracle's
GridMapper.  The GPU then only has to equal the restatement (tests/test_icp_search_map_gpu.py)."""
import numpy as np
import pytest

import icp_search_map_cases as mc
import icp_search_map_restatement as M
import icp_search_restatement as S


@pytest.mark.parametrize("name", [c.name for c in mc.CASES])
def test_each_case_reaches_what_it_names(name):
    c = mc.CASE[name]
    assert S.valid(c.p) and M.stamp_is_a_non_increasing_function_of_d2(c.p)
    res = mc.expected(name)
    assert c.check(c, res), (name, c.reaches)


def test_the_stamp_is_a_non_increasing_function_of_d2_over_a_sweep():
    for res in (0.01, 0.025, 0.05, 0.0625, 0.1, 0.5):
        for sigma in (0.005, 0.02, 0.05, 0.1, 0.3, 1.0):
            for k in range(1, 9):
                assert M.stamp_is_a_non_increasing_function_of_d2(S.Params(resolution=res, sigma=sigma, stamp_cells=k)), (res, sigma, k)


def _differs(a: M.Result, b: M.Result) -> bool:
    if not np.array_equal(a.table, b.table) or a.tgt_points != b.tgt_points or a.outcome != b.outcome:
        return True
    return any(x is not None and not np.array_equal(x, y) for x, y in ((a.scores, b.scores), (a.wide_scores, b.wide_scores)))


@pytest.mark.parametrize("plant", mc.PLANTS)
def test_each_planted_error_changes_a_case(plant):
    named = [c for c in mc.CASES if plant in c.plants]
    assert named, plant
    for c in named:
        wrong = M.search(c.occ(), c.geom, c.scan_cloud, c.T, c.p, c.wp, c.shape, plant=plant)
        assert _differs(wrong, mc.expected(c.name)), (plant, c.name)


def test_the_table_covers_the_sizes_origins_and_parameters():
    cs = mc.CASES
    assert {c.geom.side for c in cs} >= {64, 80, 96, 24}
    assert {S.side(c.p) for c in cs} >= {32, 34, 48, 160}
    frames = [M.frame(c.geom, c.T, c.p) for c in cs]
    assert {(f.cx - f.h2) % 32 for f in frames} >= {0, 1, 31} and {(f.cy - f.h2) % 32 for f in frames} >= {0, 1, 31}
    assert any(f.cx - f.h2 == 32 for f in frames) and any(f.cx - f.h2 < 0 for f in frames) and any(f.cx + f.h2 > c.geom.side for f, c in zip(frames, cs))
    assert {c.p.stamp_cells for c in cs} >= {1, 3, 8} and {c.p.lin_cells for c in cs} >= {0, 6, 16} and {c.p.ang_steps for c in cs} >= {0, 20}
    assert any(c.p.slack_q10 > 0 for c in cs) and {c.scan.size for c in cs} >= {1, 7, 360}
    assert all(f.E != c.p.half_extent for f, c in zip(frames, cs) if S.side(c.p) < 160)      # M3's E' is not S1's E
    assert any(c.wp is not None for c in cs) and any(c.shape is not None for c in cs)


@pytest.mark.parametrize("name", [b.name for b in mc.BEHAVIOURS])
def test_behaviour_on_maps_drawn_by_the_oracle(name):
    b = {x.name: x for x in mc.BEHAVIOURS}[name]
    res = mc.behaviour_result(name)
    info = res.outcome.info
    print(name, "tgt_points", res.tgt_points, "quality", info.quality, "accepted", info.accepted, "at_edge", info.at_edge, "T", info.T)
    assert round(info.quality, 3) == mc.BEHAVIOUR_RECORD[name]
    if b.accepted is None:
        return                                     # the wide window against the wrong room: recorded, it is NOT rejected (M9)
    assert info.accepted == b.accepted
    if (b.accepted or b.to_cell) and b.map == b.room:
        assert (info.quality >= b.p.min_quality) == bool(b.accepted)
        assert abs(info.T[0] - b.truth[0]) <= b.p.ang_step * (1 + 1e-9)
        assert abs(info.T[1] - b.truth[1]) <= b.p.resolution * (1 + 1e-9) and abs(info.T[2] - b.truth[2]) <= b.p.resolution * (1 + 1e-9)
    elif b.map == b.room:
        assert info.at_edge == 1                   # the truth is outside the window: rejected at its edge
