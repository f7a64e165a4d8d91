"""CPU tests of the MPPI cost field (include/tbnav_mppi.h, section COST FIELD): the numpy restatement
(tests/mppi_field_restatement.py) against the field-less restatements, the lookup's properties F2 promises, the behaviour
scenario S, and what of the new surface can be checked without a GPU (null handles, the compile-only node file, the host
function that derives a field from distances)."""
import ctypes as C
import os

import numpy as np
import pytest

import mppi_field_restatement as fr
import oracle_api as orc
import second_restatement as sr
from cases import WAYPOINTS, mppi_cfg, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "obj")
HOST_LIB = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "libtbnav_host.so")
EPS = 2.0 ** -53


def _noise(seed, K, T, var=0.9):
    return orc.normal_stream(seed, K * T * 2, 0.0, np.sqrt(var)).reshape(K, T, 2)


# ---- 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,horizon,ticks", [(64, 0.25, 3), (37, 0.29, 2)])
def test_zero_weight_and_zero_field_are_the_fieldless_tick(K, horizon, ticks):
    """weight = 0 (on random values) and an all-zero field (at weight 1e4): the same bits as second_restatement's tick, which
    in turn meets the oracle at tests/test_second_restatement.py's figures."""
    d = mppi_cfg(K, horizon)
    T = sr.mppi_steps(horizon, d["dt"])
    f0 = dict(fr.random_field_7x5(), weight=0.0)
    fz = dict(fr.random_field_7x5(), values=np.zeros((7, 5), dtype=np.float32))
    u = np.zeros((2, T)); u_o = np.zeros((2, T))
    x0 = (0.5, 0.2, 1.0)
    for t in range(ticks):
        nz = _noise(42 + t, K, T)
        base = sr.mppi_new_controls(d, u, (0.3, -0.2), WAYPOINTS[2], x0, nz)
        for f in (f0, fz, None):
            got = fr.mppi_new_controls_field(d, u, (0.3, -0.2), WAYPOINTS[2], x0, nz, field=f)
            for key in ("loss", "J", "u", "out"):
                assert np.array_equal(got[key], base[key]), (key, f is None)
        a = orc.mppi_new_controls(d, u_o, (0.3, -0.2), WAYPOINTS[2], x0, nz)
        assert rel_err(base["loss"], a["loss"]) < 1e-12 and rel_err(base["J"], a["J"]) < 1e-12
        assert np.allclose(base["u"], a["u"], rtol=1e-11, atol=1e-13) and np.allclose(base["out"], a["out"], rtol=1e-11, atol=1e-13)
        u, u_o = base["u"], a["u"]
        x0 = (x0[0] + 0.01, x0[1] + 0.004, x0[2] + 0.02)


def test_restated_arc_step_meets_the_oracles_arc_tick():
    """The oracle does not expose the per-step state of its exact-arc dynamics, so the step is restated (from the comment block of
    csrc/mppi_device.hpp) and held here against the oracle's field-less arc tick: a turning warm start, a heading that crosses the
    +-pi cut, three ticks."""
    d = mppi_cfg(65, 1.0)
    T = sr.mppi_steps(1.0, d["dt"])
    u = np.zeros((2, T)); u[0] = 2.0; u[1] = 3.5
    u_o = u.copy()
    x0 = (0.0, 0.0, 3.1)
    for t in range(3):
        nz = _noise(7 + t, 65, T)
        a = orc.mppi_new_controls(d, u_o, (2.0, 3.5), WAYPOINTS[2], x0, nz, dyn=1)
        b = fr.mppi_new_controls_field(d, u, (2.0, 3.5), WAYPOINTS[2], x0, nz, field=None, dyn=1)
        assert rel_err(b["loss"], a["loss"]) < 1e-12 and rel_err(b["J"], a["J"]) < 1e-12
        assert np.allclose(b["u"], a["u"], rtol=1e-11, atol=1e-13)
        u, u_o = b["u"], a["u"]
        x0 = (x0[0] + 0.002, x0[1] - 0.001, x0[2] + 0.003)


def test_the_field_carries_a_real_share_of_the_parity_setting():
    """The setting of the device parity test (tests/test_mppi_field_gpu.py): the rollouts start beside the 7 x 5 field, cross it and
    leave it, and its share of J(0) is tens of per cent — a device that dropped the term could not pass."""
    d = mppi_cfg(256, 0.5)
    f = fr.random_field_7x5()
    u = np.zeros((2, 50)); u[0] = 5.0; u[1] = 6.0
    r = fr.mppi_new_controls_field(d, u, (5.0, 6.0), WAYPOINTS[2], (0.5, 0.2, 1.0), _noise(1, 256, 50), field=f)
    share = r["field_share"].sum(axis=0) / r["J"][0]
    print("field share of J(0): median", np.median(share), "min", share.min(), "max", share.max())
    assert 0.2 < np.median(share) < 0.8


# ---- 2-5: the lookup -------------------------------------------------------------------------------------------------------
# resolution 0.25 from (-0.5, 1.0): every cell centre and every product of F2 is exact in fp64, so "== at a centre" tests the
# indexing and the lerps and nothing else
GEOM = dict(xmin=-0.5, ymin=1.0, resolution=0.25)


def _v75():
    return np.random.default_rng(5).random((7, 5), dtype=np.float32)   # k * 2^-24: differences of two values are exact in fp64


def test_lookup_returns_the_stored_value_at_every_cell_centre():
    v = _v75()
    X, Y = fr.cell_centres(7, 5, GEOM["xmin"], GEOM["ymin"], GEOM["resolution"])
    assert np.array_equal(fr.lookup(v, **GEOM, x=X, y=Y), v.astype(np.float64))


def test_lookup_is_constant_beyond_the_outermost_centres():
    v = _v75().astype(np.float64)
    lo_x, hi_x = GEOM["xmin"] + 0.125, GEOM["xmin"] + 6.5 * 0.25
    lo_y, hi_y = GEOM["ymin"] + 0.125, GEOM["ymin"] + 4.5 * 0.25
    ys = GEOM["ymin"] + (np.arange(5) + 0.5) * 0.25
    xs = GEOM["xmin"] + (np.arange(7) + 0.5) * 0.25
    for far in (1e-3, 0.124, 0.126, 3.0, 1e6, 1e300):
        assert np.array_equal(fr.lookup(v, **GEOM, x=np.full(5, lo_x - far), y=ys), v[0])
        assert np.array_equal(fr.lookup(v, **GEOM, x=np.full(5, hi_x + far), y=ys), v[6])
        assert np.array_equal(fr.lookup(v, **GEOM, x=xs, y=np.full(7, lo_y - far)), v[:, 0])
        assert np.array_equal(fr.lookup(v, **GEOM, x=xs, y=np.full(7, hi_y + far)), v[:, 4])
        corners = fr.lookup(v, **GEOM, x=[lo_x - far, lo_x - far, hi_x + far, hi_x + far], y=[lo_y - far, hi_y + far, lo_y - far, hi_y + far])
        assert np.array_equal(corners, [v[0, 0], v[0, 4], v[6, 0], v[6, 4]])


def test_lookup_of_non_finite_coordinates():
    """F2: a NaN goes to grid coordinate 0, +inf to the last centre, -inf to the first."""
    v = _v75().astype(np.float64)
    yc = GEOM["ymin"] + 2.5 * 0.25   # centre of column 2
    xc = GEOM["xmin"] + 3.5 * 0.25   # centre of row 3
    got = fr.lookup(v, **GEOM, x=[np.nan, np.inf, -np.inf, xc, xc, xc, np.nan], y=[yc, yc, yc, np.nan, np.inf, -np.inf, np.nan])
    assert np.array_equal(got, [v[0, 2], v[6, 2], v[0, 2], v[3, 0], v[3, 4], v[3, 0], v[0, 0]])


def test_lookup_is_continuous_across_cell_borders():
    """Along a slanted line through several cell borders in steps of 1e-9 m (windows round each border the line crosses, on both
    axes): |c(p + d) - c(p)| <= d * (max - min) / resolution * 2 + 8 * 2^-53 * max|v|."""
    f = fr.random_field_7x5()
    v = f["values"]
    res, d = f["resolution"], 1e-9
    bound = d * float(v.max() - v.min()) / res * 2 + 8 * EPS * float(np.abs(v).max())
    direction = np.array([np.cos(0.3), np.sin(0.3)])
    start = np.array([f["xmin"] + 0.03, f["ymin"] + 0.04])
    worst = 0.0
    for axis in (0, 1):
        origin = (f["xmin"], f["ymin"])[axis]
        for border in range(1, 5):   # the cell borders and the lines through the centres, where the lookup changes cells
            for line in (origin + border * res, origin + (border + 0.5) * res):
                s0 = (line - start[axis]) / direction[axis]
                s = s0 + np.arange(-2000, 2001) * d
                p = start[None, :] + s[:, None] * direction[None, :]
                c = fr.lookup(v, f["xmin"], f["ymin"], res, p[:, 0], p[:, 1])
                worst = max(worst, float(np.abs(np.diff(c)).max()))
    assert 0 < worst <= bound, (worst, bound)


# ---- 6: scenario S ------------------------------------------------------------------------------------------------------
def _restated_controller(field):
    prm = fr.S_PRM
    T = sr.mppi_steps(prm["horizon"], prm["dt"])
    state = {"u": np.zeros((2, T))}

    def tick(x, noise):
        r = fr.mppi_new_controls_field(prm, state["u"], (0.0, 0.0), fr.S_GOAL, tuple(x), noise, field=field)
        state["u"] = r["u"]
        return r["out"]
    return tick


def test_scenario_s_with_the_field_the_robot_goes_round():
    """Seed 3, with the field: arrival within 1200 ticks, never closer to the disc than r_robot = 0.10 m (design conditions; the
    restatement meets them at 694-824 ticks and 0.326-0.349 m over seeds 3, 4, 5, 7)."""
    ticks, clearance = fr.scenario_run(_restated_controller(fr.scenario_field()), seed=3)
    print("scenario S with field: ticks", ticks, "least clearance", clearance)
    assert ticks is not None and ticks <= fr.S_MAX_TICKS
    assert clearance >= fr.S_R_ROBOT


def test_scenario_s_without_the_field_the_robot_drives_through():
    """Seed 3, without: the least clearance is negative — the straight line to the waypoint passes through the disc."""
    ticks, clearance = fr.scenario_run(_restated_controller(None), seed=3)
    print("scenario S without field: ticks", ticks, "least clearance", clearance)
    assert clearance < 0


# ---- 7: the C-ABI without a GPU ------------------------------------------------------------------------------------------
def test_null_handles_are_invalid_arguments(pkg):
    c = pkg.capi
    L = c.lib()
    g = c.MppiCostField(7, 5, 0.0, 0.0, 0.05, 1.0)
    v = np.zeros(35, dtype=np.float32)
    xy = np.zeros(2); out = np.zeros(1)
    assert L.tbnav_mppi_set_cost_field(None, C.byref(g), v.ctypes.data) == c.ERR_INVALID_ARG
    assert L.tbnav_mppi_set_cost_field(None, None, None) == c.ERR_INVALID_ARG
    assert L.tbnav_mppi_get_cost_field(None, None, None) == c.ERR_INVALID_ARG
    assert L.tbnav_mppi_cost_field_lookup(None, xy.ctypes.data, 1, out.ctypes.data) == c.ERR_INVALID_ARG
    assert L.tbnav_mppi_group_set_cost_field(None, C.byref(g), v.ctypes.data) == c.ERR_INVALID_ARG
    assert c.MPPI_FIELD_MAX_SIDE == 4096


# ---- 8: the compile-only node file -----------------------------------------------------------------------------------------
SET_COST_FIELD = b"_ZN10controller4MPPI12setCostFieldERKNS_9CostFieldE"   # controller::MPPI::setCostField(controller::CostField const&)


def test_node_with_a_cost_field_compiles_and_the_plain_node_does_not_name_it():
    def read(name):
        path = os.path.join(OBJ, name)
        assert os.path.exists(path), "run __graft_entry__.build()"
        with open(path, "rb") as fh:
            return fh.read()
    assert SET_COST_FIELD in read("node_calls_mppi_field.o")
    assert b"CostField" not in read("node_calls.o")


# ---- 9: the two functions that derive a field from distances ---------------------------------------------------------------
@pytest.fixture(scope="module")
def host(pkg):
    pkg.capi.lib()  # loads torch's HIP runtime first, then libtbnav_hip.so
    L = C.CDLL(HOST_LIB)
    L.hst_cost_field_from_distance.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p]
    L.hst_field_last_error.restype = C.c_char_p
    return L


def _cpp_field(host, dist, r_robot, r_inflate):
    d = np.ascontiguousarray(dist, dtype=np.float64)
    out = np.empty(d.shape, dtype=np.float32)
    rc = host.hst_cost_field_from_distance(d.ctypes.data, d.shape[0], d.shape[1], r_robot, r_inflate, out.ctypes.data)
    return rc, out


def test_cost_field_from_distance_python_equals_cpp_bit_for_bit(pkg, host):
    from rtn_amd.mppi import cost_field_from_distance
    r_robot, r_inflate = 0.10, 0.45
    rng = np.random.default_rng(2)
    edge = np.array([0.0, r_robot, np.nextafter(r_robot, 1), np.nextafter(r_robot, 0), r_inflate, np.nextafter(r_inflate, 0),
                     np.nextafter(r_inflate, 1), 10.0, 0.05, 0.2, 0.3, 0.449])
    dist = np.concatenate([edge, rng.uniform(0.0, 0.6, 24)]).reshape(6, 6)
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_gridmapper.npz"))
    occ = z["g80_s1_occ_dist"].reshape(80, 80)
    i, j = np.unravel_index(np.argmin(np.abs(occ - 0.3)), occ.shape)   # a window that straddles the inflation band
    i, j = min(max(i - 3, 0), 74), min(max(j - 3, 0), 74)
    window = np.ascontiguousarray(occ[i:i + 6, j:j + 6])
    assert window.min() < r_inflate
    for d in (dist, window):
        py = cost_field_from_distance(d, r_robot, r_inflate)
        rc, cpp = _cpp_field(host, d, r_robot, r_inflate)
        assert rc == 0, host.hst_field_last_error()
        assert py.dtype == np.float32 and py.shape == d.shape
        assert np.array_equal(py.view(np.uint32), cpp.view(np.uint32))
        assert np.array_equal(py, fr.cost_field_from_distance(d, r_robot, r_inflate))
    py = cost_field_from_distance(dist, r_robot, r_inflate)
    assert py[0, 0] == 1.0 and py[0, 1] == 1.0 and py[0, 4] == 0.0 and py[1, 1] == 0.0 and 0.0 < py[1, 4] < 1.0
    for bad in ((0.45, 0.45), (0.5, 0.45), (-0.1, 0.45)):
        with pytest.raises(ValueError):
            cost_field_from_distance(dist, *bad)
        assert _cpp_field(host, dist, *bad)[0] == 1
