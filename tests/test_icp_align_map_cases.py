"""The proof of the map alignment's case table (tests/icp_align_map_cases.py), on the CPU, on the restatement
(tests/icp_align_map_restatement.py; include/tbnav_icp.h MAP ALIGNMENT A1-A11): every case reaches what it names, every planted
error changes the result bits of a case, and the BEHAVIOUR of the method on maps the oracle's GridMapper drew."""
import math

import numpy as np
import pytest

import icp_align_map_cases as ac
import icp_align_map_restatement as A
import icp_restatement as R


@pytest.mark.parametrize("name", [c.name for c in ac.CASES])
def test_every_case_reaches_what_it_names(name):
    c = ac.CASE[name]
    assert A.valid(c.p) and 24 <= c.geom.side <= 96
    res = ac.expected(name)
    assert c.check(c, res), (name, c.reaches, res.criterion, res.iterations, res.correspondences)
    assert res.ok == R.converged(res.criterion)
    if not res.ok:
        assert res.T == tuple(float(v) for v in c.T)          # A7: the guess, unchanged


def test_the_table_names_every_size_window_beam_count_and_stop_rule():
    cs = ac.CASES
    assert {c.size_id for c in cs} == {"s64", "s80", "s96", "r20"}
    assert {8, 16, 32} <= {c.p.half_cells for c in cs} and {1, 2, 3, 4} == {c.p.feature_cells for c in cs}
    assert {1, 3, 255, 256, 257, 1080, ac.MAX_BEAMS} <= {c.scan.size for c in cs}
    assert {-(-c.scan.size // 256) for c in cs} >= {1, 2, 4, 5, 8, 16}          # every instantiation of the kernel's ladder
    crits = {ac.expected(c.name).criterion for c in cs}
    assert crits == {R.ITERATIONS, R.TRANSFORM, R.ABS_MSE, R.REL_MSE, R.NO_CORRESPONDENCES, R.DEGENERATE}
    assert {1, 2} <= {c.icp["max_iter"] for c in cs}


@pytest.mark.parametrize("plant", ac.PLANTS)
def test_every_planted_error_changes_a_case(plant):
    named = [c for c in ac.CASES if plant in c.plants]
    assert named, plant
    for c in named:
        assert ac.digest(ac.run(c, plant=plant)) != ac.digest(ac.expected(c.name)), (plant, c.name)


def test_a_guess_that_is_not_finite_or_outside_the_map_is_out_of_world():
    c = ac.CASE["room_defaults"]
    for T in ac.NON_FINITE_GUESSES + ((0.1, 2.0, 0.0), (0.1, 0.0, -2.0001), (0.1, 1e300, 0.0)):
        assert ac.run(c, T=T) is None, T
    assert ac.run(c, T=(0.1, -2.0, 1.9999)) is not None


def test_bad_parameters_are_named_as_such():
    for kw in (dict(half_cells=7), dict(half_cells=257), dict(gate_cells=0), dict(gate_cells=17), dict(feature_cells=0), dict(feature_cells=5),
               dict(max_flatness=1.0), dict(max_flatness=-0.01), dict(max_flatness=math.nan), dict(max_flatness=math.inf), dict(reserved=1)):
        assert not A.valid(A.Params(**kw)), kw
    assert A.valid(A.Params()) and A.valid(A.Params(8, 1, 1, 0.0)) and A.valid(A.Params(256, 16, 4, 0.999))


def test_behaviour_on_maps_the_grid_mapper_drew():
    """mean translation and angle error after the alignment are below the starts'; the figures themselves are printed and recorded in
    icp_align_map_cases.BEHAVIOUR_RECORD, not asserted: nobody has measured them on other maps"""
    for room in ac.BEHAVIOUR_ROOMS:
        rows = ac.behaviour(room)
        s_t, s_a = np.array([r[0][0] for r in rows]), np.array([r[0][1] for r in rows])
        e_t, e_a = np.array([r[1][0] for r in rows]), np.array([r[1][1] for r in rows])
        it = [r[2] for r in rows]
        mm = lambda v: (round(float(1e3 * v.mean()), 1), round(float(1e3 * v.max()), 1))          # (mean, max)
        rec = dict(start_mm=mm(s_t), end_mm=mm(e_t), start_mrad=mm(s_a), end_mrad=mm(e_a),
                   iterations=(round(float(np.mean(it)), 1), int(max(it))), ok=int(sum(r[3] for r in rows)))
        print(room, rec)
        assert e_t.mean() < s_t.mean() and e_a.mean() < s_a.mean(), (room, rec)
