"""The cost grid from a filter's map (include/tbnav_nav.h G7-G8) on the CPU: tbnav_nav_inflation_tables against the restatement with
==, every rejection of G7, the case table (tests/nav_from_map_cases.py) against the host route over the exact EDT, what each case
names, a wrong merge told apart, and the library's exports."""
import ctypes as C
import functools

import numpy as np
import pytest

import nav_from_map_cases as fc
import nav_from_map_restatement as fr
import oracle_api as orc
from mppi_field_restatement import cost_field_from_distance
from nav_restatement import nav_cost_from_distance

NEW_SYMBOLS = ("tbnav_nav_inflation_tables", "tbnav_nav_set_cost_from_rbpf", "tbnav_nav_get_cost", "tbnav_mppi_set_cost_field_from_rbpf",
               "tbnav_nav_last_cost_kernel", "tbnav_nav_profile_cost_from_rbpf")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tables(pkg, res, r_robot, r_inflate, k, cap=None):
    """(status, cost, field, n, reach) through ctypes; cap: the room offered (None: what the length query asks for)."""
    L = pkg.capi.lib()
    n, reach = C.c_int32(-7), C.c_int32(-7)
    rc = L.tbnav_nav_inflation_tables(res, r_robot, r_inflate, k, None, None, 0, C.byref(n), C.byref(reach))
    if rc != pkg.capi.OK:
        return rc, None, None, n.value, reach.value
    room = n.value + 1 if cap is None else cap
    cost, field = np.full(max(room, 1), 255, dtype=np.uint8), np.full(max(room, 1), -1.0, dtype=np.float32)
    rc = L.tbnav_nav_inflation_tables(res, r_robot, r_inflate, k, cost.ctypes.data, field.ctypes.data, room, C.byref(n), C.byref(reach))
    return rc, cost, field, n.value, reach.value


def test_the_library_exports_every_new_symbol(pkg):
    L = pkg.capi.lib()
    for name in NEW_SYMBOLS:
        assert name in pkg.capi.declared_symbols() and hasattr(L, name), name
    assert (pkg.capi.NAV_MAX_REACH, pkg.capi.NAV_BEST_PARTICLE) == (fr.MAX_REACH, -1)


@pytest.mark.parametrize("prm", fc.TABLE_PARAMS, ids=[str(i) for i in range(len(fc.TABLE_PARAMS))])
def test_inflation_tables_equal_the_restatement(pkg, prm):
    """Cost bytes, field bits, n and reach, with ==; the Python wrapper gives the same arrays."""
    cost, field, R = fr.tables(*prm)
    rc, got_cost, got_field, n, reach = _tables(pkg, *prm)
    assert rc == pkg.capi.OK and (n, reach) == (R * R + 1, R) and len(cost) == n + 1
    assert np.array_equal(got_cost, cost) and np.array_equal(_bits(got_field), _bits(field))
    assert (cost[-1], field[-1]) == (1, 0.0)                       # the open value
    assert cost[0] == 0 and field[0] == 1.0                        # an occupied cell itself
    from rtn_amd.nav import inflation_tables
    w_cost, w_field, w_reach = inflation_tables(*prm)
    assert np.array_equal(w_cost, cost) and np.array_equal(_bits(w_field), _bits(field)) and w_reach == R


def test_inflation_tables_past_the_reach_are_open(pkg):
    """What makes the table form equal to the host route: at c = R*R the formulas have reached the open value already."""
    for prm in fc.TABLE_PARAMS:
        cost, field, R = fr.tables(*prm)
        assert np.sqrt(float(R * R)) * prm[0] >= prm[2] and (cost[R * R], field[R * R]) == (cost[-1], field[-1]), prm


def test_inflation_tables_rejections(pkg):
    c = pkg.capi
    L = c.lib()
    nan, inf = float("nan"), float("inf")
    bad = [(0.0, 0.1, 0.45, 8.0), (-0.05, 0.1, 0.45, 8.0), (nan, 0.1, 0.45, 8.0), (inf, 0.1, 0.45, 8.0),
           (0.05, -0.01, 0.45, 8.0), (0.05, nan, 0.45, 8.0), (0.05, 0.45, 0.45, 8.0), (0.05, 0.5, 0.45, 8.0),
           (0.5, 0.1, float(np.nextafter(10.0, 11.0)), 8.0), (0.5, 0.1, nan, 8.0), (0.5, 0.1, inf, 8.0),
           (0.05, 0.1, 0.45, -0.5), (0.05, 0.1, 0.45, 63.5), (0.05, 0.1, 0.45, nan), (0.05, 0.1, 0.45, inf)]
    for prm in bad:
        assert fr.check_args(*prm) == "INVALID_ARG", prm
        rc, _, _, n, reach = _tables(pkg, *prm)
        assert rc == c.ERR_INVALID_ARG and (n, reach) == (-7, -7), prm
    # R = 32 is accepted, R = 33 is not; r_inflate = 10.0 is accepted where the cells are large enough
    assert fr.reach(0.05, 1.55) == 32 and fr.reach(0.05, 1.6) == 33 and fr.check_args(0.05, 0.1, 1.6, 8.0) == "UNSUPPORTED"
    assert _tables(pkg, 0.05, 0.1, 1.55, 8.0)[0] == c.OK
    rc, _, _, n, reach = _tables(pkg, 0.05, 0.1, 1.6, 8.0)
    assert rc == c.ERR_UNSUPPORTED and (n, reach) == (-7, -7)
    assert _tables(pkg, 1e-300, 0.1, 0.45, 8.0)[0] == c.ERR_UNSUPPORTED
    assert _tables(pkg, 0.5, 0.1, 10.0, 8.0)[0] == c.OK and fr.reach(0.5, 10.0) == 21
    # a buffer too small: INVALID_ARG with n set and nothing written; either table may be null
    rc, cost, field, n, reach = _tables(pkg, 0.05, 0.10, 0.45, 8.0, cap=101)
    assert rc == c.ERR_INVALID_ARG and (n, reach) == (101, 10) and (cost == 255).all() and (field == -1.0).all()
    want_cost, want_field, _ = fr.tables(0.05, 0.10, 0.45, 8.0)
    only = np.full(102, 255, dtype=np.uint8)
    assert L.tbnav_nav_inflation_tables(0.05, 0.10, 0.45, 8.0, only.ctypes.data, None, 102, None, None) == c.OK
    assert np.array_equal(only, want_cost)
    onlyf = np.full(102, -1.0, dtype=np.float32)
    assert L.tbnav_nav_inflation_tables(0.05, 0.10, 0.45, 8.0, None, onlyf.ctypes.data, 102, None, None) == c.OK
    assert np.array_equal(_bits(onlyf), _bits(want_field))


def test_the_other_entry_points_without_a_handle(pkg):
    c = pkg.capi
    L = c.lib()
    buf = C.create_string_buffer(8)
    assert L.tbnav_nav_set_cost_from_rbpf(None, None, -1, 0.10, 0.45, 8.0) == c.ERR_INVALID_ARG
    assert L.tbnav_mppi_set_cost_field_from_rbpf(None, None, -1, 0.10, 0.45, 1.0) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_get_cost(None, None) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_last_cost_kernel(None, buf, 8) == c.ERR_INVALID_ARG


# ---- the case table ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(size_id):
    """name -> (occupancy, c over the widest window any parameter set of the size asks for, metres of the exact EDT)."""
    size = fc.SIZE[size_id]
    r_max = max(fr.reach(size.res, p[1]) for p in fc.params(size).values())
    out = {}
    for name, occ in fc.patterns(size).items():
        codes = orc.exact_edt_codes(occ, size.radius, np.full(occ.shape, 0xFFFF, dtype=np.uint16))
        metres = np.where(codes == 0xFFFF, fr.MAX_OCC_DIST, np.sqrt(codes.astype(np.float64)) * size.res)    # tbnav_rbpf_get_occ_dist
        out[name] = (occ, fr.nearest_c(occ, r_max), metres)
    return out


@pytest.mark.parametrize("size_id", [s.id for s in fc.SIZES])
def test_the_table_form_equals_the_host_route_over_the_exact_edt(size_id):
    """For every pattern and parameter set: table[c] == nav_cost_from_distance / cost_field_from_distance of sqrt(code) * res."""
    size = fc.SIZE[size_id]
    for name, (occ, c, metres) in _case(size_id).items():
        for pname, (r_robot, r_inflate, k) in fc.params(size).items():
            R = fr.reach(size.res, r_inflate)
            cost = fr.cost_from_occ(occ, size.res, r_robot, r_inflate, k, c=c)
            field = fr.field_from_occ(occ, size.res, r_robot, r_inflate, c=c)
            assert np.array_equal(cost, nav_cost_from_distance(metres, r_robot, r_inflate, k)), (name, pname)
            assert np.array_equal(_bits(field), _bits(cost_field_from_distance(metres, r_robot, r_inflate))), (name, pname)
            if name in ("ties", "reach"):       # (the window of the parameter set itself gives the same grid as the widest one)
                assert np.array_equal(fr.cost_from_occ(occ, size.res, r_robot, r_inflate, k), cost), (name, pname, R)


def test_the_sizes_and_patterns_are_what_they_name():
    assert [(s.xsize, -(-s.xsize // 32), s.xsize % 32) for s in fc.SIZES] == [(64, 2, 0), (96, 3, 0), (80, 3, 16), (24, 1, 24)]
    for size in fc.SIZES:
        assert int(np.ceil((2 * size.half) / size.res)) == size.xsize and int(np.ceil(10.0 / size.res)) == size.radius
        pats = fc.patterns(size)
        xs = size.xsize
        assert not pats["empty"].any() and pats["full_map"].all() and pats["corners"].sum() == 4
        assert pats["full_row"].sum() == xs == pats["full_col"].sum() and 0 < pats["random"].sum() < 0.02 * xs * xs
        if xs > 32:
            tiles = {(i // 32, j // 32) for i, j in np.argwhere(pats["one_tile"])}
            assert tiles == {(1, 1)} and pats["one_tile"].sum() > 5
            assert {tuple(np.argwhere(pats[f"four_corner_{n}"])[0]) for n in range(4)} == {(31, 31), (31, 32), (32, 31), (32, 32)}
    assert {fr.reach(0.05, p[1]) for p in fc.PARAMS_5CM.values()} == {10, 32}
    assert [fr.reach(0.5, p[1]) for p in fc.PARAMS_50CM.values()] == [2, 10, 21]


@pytest.mark.parametrize("size_id", [s.id for s in fc.SIZES])
def test_the_reach_pattern_has_an_obstacle_at_the_tables_last_entry_and_one_past_it(size_id):
    size = fc.SIZE[size_id]
    occ = fc.patterns(size)["reach"]
    for pname, (r_robot, r_inflate, k) in fc.params(size).items():
        cost_tab, field_tab, R = fr.tables(size.res, r_robot, r_inflate, k)
        c = fr.nearest_c(occ, R)
        cost = fr.lookup(c, cost_tab, R)
        probes = fc.reach_probes(size, R)
        cs = [want for _, want in probes]
        assert R * R in cs and R * R + 1 in cs and (R + 1) * (R + 1) in cs, (pname, probes)
        for (cell, want), on_axis_past in zip(probes, (False, True, False, False, False)):
            if want <= R * R:
                assert c[cell] == want and cost[cell] == cost_tab[want], (pname, cell)
            else:       # past the table: reads open, whether the window sees the obstacle (c = R*R + 1, the diagonal) or not (R + 1 rows away)
                assert cost[cell] == cost_tab[-1] == 1 and c[cell] == (fr.NONE if on_axis_past else want), (pname, cell)


def test_a_merge_that_lets_the_first_row_decide_gives_another_answer():
    size = fc.SIZE["r20"]
    occ = fc.patterns(size)["ties"]
    R = fr.reach(size.res, fc.PARAMS_50CM["r_robot_0_k_63"][1])
    right, wrong = fr.nearest_c(occ, R), fr.first_row_c(occ, R)
    assert right[fc.TIE_TARGET] == fc.TIE_C == wrong[fc.TIE_TARGET]          # two rows at the same distance: no way to get it wrong
    assert right[fc.MERGE_TARGET] == fc.MERGE_C and wrong[fc.MERGE_TARGET] == fc.MERGE_WRONG_C
    cost_tab = fr.tables(size.res, *fc.PARAMS_50CM["r_robot_0_k_63"])[0]
    assert not np.array_equal(fr.lookup(right, cost_tab, R), fr.lookup(wrong, cost_tab, R))
