"""The goal field's other layers (include/tbnav_nav.h): the compile-only node file, what of the C-ABI answers without a GPU, the
Python and C++ helpers that derive a cost grid from distances (bit for bit), and planner::GoalField through its test hook on the
7 x 5 case (GPU)."""
import ctypes as C
import os

import numpy as np
import pytest

import nav_cases as nc
import nav_restatement as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "obj")
HOST_LIB = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "libtbnav_host.so")

APPLY_TO = b"_ZN7planner9GoalField7applyToERN10controller4MPPIEdd"     # planner::GoalField::applyTo(controller::MPPI&, double, double)
SOLVE = b"_ZN7planner9GoalField5solveEdd"                              # planner::GoalField::solve(double, double)


def test_node_with_a_goal_field_compiles_and_the_plain_node_does_not_name_it():
    def read(name):
        path = os.path.join(OBJ, name)
        assert os.path.exists(path), "run __graft_entry__.build()"
        with open(path, "rb") as fh:
            return fh.read()
    nav = read("node_calls_nav.o")
    assert APPLY_TO in nav and SOLVE in nav and b"navCostFromDistance" in nav
    assert b"GoalField" not in read("node_calls.o")


def test_the_c_abi_without_a_handle_or_a_device(pkg):
    """Bad arguments return before any device call; without a GPU create fails with TBNAV_ERR_NO_DEVICE, as everywhere else."""
    c = pkg.capi
    L = c.lib()
    for name in ("tbnav_nav_create", "tbnav_nav_destroy", "tbnav_nav_set_cost", "tbnav_nav_solve", "tbnav_nav_cell_of", "tbnav_nav_get_cost_to_go",
                 "tbnav_nav_get_field", "tbnav_nav_path", "tbnav_nav_last_solve", "tbnav_nav_apply_to_mppi", "tbnav_nav_apply_to_mppi_group"):
        assert name in c.declared_symbols() and hasattr(L, name), name
    h = C.c_void_p()
    buf = np.zeros(35, dtype=np.uint32)
    n, ix, iy = C.c_int32(-7), C.c_int32(), C.c_int32()
    assert L.tbnav_nav_create(None, C.byref(h)) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_create(C.byref(c.NavParams(7, 5, 0.0, 0.0, 0.05, -1, 0)), None) == c.ERR_INVALID_ARG
    for bad in (c.NavParams(1, 5, 0.0, 0.0, 0.05, -1, 0), c.NavParams(7, c.NAV_MAX_SIDE + 1, 0.0, 0.0, 0.05, -1, 0),
                c.NavParams(7, 5, 0.0, 0.0, 0.0, -1, 0), c.NavParams(7, 5, float("nan"), 0.0, 0.05, -1, 0)):
        assert L.tbnav_nav_create(C.byref(bad), C.byref(h)) == c.ERR_INVALID_ARG and not h.value
    L.tbnav_nav_destroy(None)
    assert L.tbnav_nav_set_cost(None, buf.ctypes.data) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_solve(None, 0, 0) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_cell_of(None, 0.0, 0.0, C.byref(ix), C.byref(iy)) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_get_cost_to_go(None, buf.ctypes.data) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_get_field(None, 10.0, buf.ctypes.data) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_path(None, 0, 0, buf.ctypes.data, 4, C.byref(n)) == c.ERR_INVALID_ARG and n.value == -7
    assert L.tbnav_nav_last_solve(None, None, None, 0) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_apply_to_mppi(None, None, 10.0, 1.0) == c.ERR_INVALID_ARG
    assert L.tbnav_nav_apply_to_mppi_group(None, None, 10.0, 1.0) == c.ERR_INVALID_ARG
    assert (c.NAV_MAX_SIDE, c.NAV_MAX_COST, c.NAV_UNREACHED) == (nr.MAX_SIDE, nr.MAX_COST, nr.UNREACHED)
    if L.tbnav_device_count() == 0:
        from rtn_amd.nav import GoalField
        with pytest.raises(c.TbnavError) as ei:
            GoalField(7, 5, **nc.GEOM)
        assert ei.value.status == c.ERR_NO_DEVICE


@pytest.fixture(scope="module")
def host(pkg):
    pkg.capi.lib()  # loads torch's HIP runtime first, then libtbnav_hip.so
    L = C.CDLL(HOST_LIB)
    L.hst_nav_cost_from_distance.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p]
    L.hst_nav_solve.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_int, C.POINTER(C.c_int)]
    L.hst_nav_last_error.restype = C.c_char_p
    return L


def _cpp_cost(host, dist, r_robot, r_inflate, k):
    d = np.ascontiguousarray(dist, dtype=np.float64)
    out = np.full(d.shape, 255, dtype=np.uint8)
    return host.hst_nav_cost_from_distance(d.ctypes.data, d.shape[0], d.shape[1], r_robot, r_inflate, k, out.ctypes.data), out


def test_nav_cost_from_distance_python_equals_cpp_bit_for_bit(pkg, host):
    from rtn_amd.nav import nav_cost_from_distance
    r_robot, r_inflate = 0.10, 0.45
    rng = np.random.default_rng(2)
    edge = np.array([0.0, r_robot, np.nextafter(r_robot, 1), np.nextafter(r_robot, 0), r_inflate, np.nextafter(r_inflate, 0),
                     np.nextafter(r_inflate, 1), 10.0, 0.05, 0.2, 0.3, 0.449])
    # distances at which k * t * t is half-way between two integers for k = 8 (t * t = 1/16, 3/16: rint goes to the even one)
    halves = r_inflate - np.sqrt(np.array([1.0, 3.0, 5.0, 7.0]) / 16.0) * (r_inflate - r_robot)
    dist = np.concatenate([edge, halves, rng.uniform(0.0, 0.6, 20)]).reshape(6, 6)
    for d, k in ((dist, 8.0), (dist, 63.0), (dist, 0.0), (dist, 2.5), (nr.scenario_u_distance(), nr.U_K)):
        py = nav_cost_from_distance(d, r_robot, r_inflate, k)
        rc, cpp = _cpp_cost(host, d, r_robot, r_inflate, k)
        assert rc == 0, host.hst_nav_last_error()
        assert py.dtype == np.uint8 and py.shape == d.shape
        assert np.array_equal(py, cpp) and np.array_equal(py, nr.nav_cost_from_distance(d, r_robot, r_inflate, k))
        assert int(py.max()) <= 1 + k and np.array_equal(py == 0, d <= r_robot) and (py[d >= r_inflate] == 1).all()
    py = nav_cost_from_distance(dist, r_robot, r_inflate, 8.0)
    assert py[0, 0] == 0 and py[0, 1] == 0 and py[0, 2] == 9 and py[0, 4] == 1 and py[1, 1] == 1
    for bad in ((0.45, 0.45, 8.0), (0.5, 0.45, 8.0), (-0.1, 0.45, 8.0), (0.1, 0.45, 63.5), (0.1, 0.45, -1.0)):
        with pytest.raises(ValueError):
            nav_cost_from_distance(dist, *bad)
        assert _cpp_cost(host, dist, *bad)[0] == 1


@pytest.mark.gpu
def test_cpp_class_gives_the_restatements_cost_to_go_field_and_path(gpu_pkg, host):
    """planner::GoalField through its hook on the 7 x 5 case: setCost, solve and path in WORLD coordinates, costToGo, field."""
    case = nc.CASES["drawn_7x5"]
    cost, goal = case["cost"], case["goal"]
    want = nc.expected("drawn_7x5")
    geom = np.array([nc.GEOM["xmin"], nc.GEOM["ymin"], nc.GEOM["resolution"]])
    X, Y = nr.cell_centres(7, 5, **nc.GEOM)
    start = nc.starts("drawn_7x5")[0]
    goal_xy, start_xy = np.array([X[goal], Y[goal]]), np.array([X[start], Y[start]])
    assert nr.cell_of(7, 5, **nc.GEOM, x=goal_xy[0], y=goal_xy[1]) == goal
    d, f, cells, n = np.zeros((7, 5), np.uint32), np.zeros((7, 5), np.float32), np.full((35, 2), -1, np.int32), C.c_int(0)
    args = (7, 5, geom.ctypes.data, cost.ctypes.data)
    outs = (10.0, d.ctypes.data, f.ctypes.data, cells.ctypes.data, 35, C.byref(n))
    rounds = host.hst_nav_solve(*args, goal_xy.ctypes.data, start_xy.ctypes.data, *outs)
    assert rounds >= 1, host.hst_nav_last_error()
    assert np.array_equal(d, want)
    assert np.array_equal(f.view(np.uint32), nr.field(want, nc.GEOM["resolution"], 10.0).view(np.uint32))
    p, _ = nr.path(cost, want, start)
    assert n.value == len(p) and np.array_equal(cells[:n.value], p)
    # a goal outside the world, and a cost above 64, are std::invalid_argument
    outside = np.array([nc.GEOM["xmin"] - 0.01, goal_xy[1]])
    assert host.hst_nav_solve(*args, outside.ctypes.data, start_xy.ctypes.data, *outs) == -2
    assert b"NOT in the bounds of the world" in host.hst_nav_last_error()
    bad = cost.copy(); bad[0, 0] = 65
    assert host.hst_nav_solve(7, 5, geom.ctypes.data, bad.ctypes.data, goal_xy.ctypes.data, start_xy.ctypes.data, *outs) == -2
