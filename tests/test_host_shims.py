"""The C++ class shims (ros-turtlebot-navigation_amd/host/, libtbnav_host.so): the rigid2d layer is
bit-exact against the oracle (itself pinned to the reference build); the controller::MPPI and
bmapping::ParticleFilter surfaces are driven exactly the way the ROS nodes call them."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_api as orc
import rbpf_cases as rc
from cases import MPPI_BASE, WAYPOINTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "libtbnav_host.so")


@pytest.fixture(scope="module")
def host(pkg):
    pkg.capi.lib()  # loads torch's HIP runtime first, then libtbnav_hip.so
    L = C.CDLL(HOST_LIB)
    L.hst_normalize_angle_PI.restype = C.c_double
    L.hst_normalize_angle_PI.argtypes = [C.c_double]
    L.hst_dd_create.restype = C.c_void_p
    L.hst_dd_create.argtypes = [C.c_void_p, C.c_double, C.c_double]
    L.hst_dd_update_odometry.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_void_p]
    L.hst_last_error.restype = C.c_char_p
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _arr(v):
    return np.array(v, dtype=np.float64)


def test_rigid2d_shim_bit_exact_vs_oracle(host):
    r = orc.RigidAPI("orc")
    rng = np.random.default_rng(4)
    for x in np.concatenate([rng.uniform(-40, 40, 500), [0.0, np.pi, -np.pi]]):
        assert host.hst_normalize_angle_PI(x) == r.normalize_angle_PI(x)
    for _ in range(200):
        a, b, v, tw = rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3), rng.uniform(-4, 4, 2), rng.uniform(-2, 2, 3)
        out = np.empty(5)
        host.hst_transform_compose(_p(a), _p(b), _p(out)); assert np.array_equal(out[:3], r.compose(a, b)[:3])
        host.hst_transform_inv(_p(a), _p(out)); assert np.array_equal(out[:3], r.inv(a)[:3])
        host.hst_transform_integrate_twist(_p(a), _p(tw), _p(out)); assert np.array_equal(out[:3], r.integrate_twist(a, tw)[:3])
        o2 = np.empty(2); host.hst_transform_apply(_p(a), _p(v), _p(o2)); assert np.array_equal(o2, r.apply(a, v))
    buf = C.create_string_buffer(128)
    host.hst_transform_print(_p(_arr([np.pi / 2, 3.0, 5.0])), buf, 128)
    assert buf.value.decode() == "theta (degrees): 90 x: 3 y: 5\n"   # operator<<, rigid2d.cpp:307-311


def test_diff_drive_shim_bit_exact_vs_oracle(host):
    r = orc.RigidAPI("orc")
    rng = np.random.default_rng(6)
    pose = _arr([0.1, -0.2, 0.3])
    dh = C.c_void_p(host.hst_dd_create(_p(pose), 0.16, 0.033)); do = r.dd_create(pose, 0.16, 0.033)
    enc = np.zeros(2); st = np.empty(7); out2 = np.empty(2)
    for step in range(300):
        if step % 2:
            tw = _arr([rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), 0.0])
            assert host.hst_dd_feedforward(dh, _p(tw)) == r.dd_feedforward(do, tw) == 0
        else:
            enc = enc + rng.uniform(-0.5, 0.7, 2)
            host.hst_dd_update_odometry(dh, enc[0], enc[1], _p(out2))
            assert np.array_equal(out2, r.dd_update_odometry(do, *enc))
        host.hst_dd_state(dh, _p(st))
        assert np.array_equal(st, r.dd_state(do))
    assert host.hst_dd_twist_to_wheels(dh, _p(_arr([0, 1, 0.5])), _p(out2)) == 1
    assert host.hst_last_error() == b"Twist cannot have y velocity component"   # diff_drive.cpp:72
    host.hst_dd_destroy(dh); r.dd_destroy(do)


def test_host_twister_draws_like_the_reference_sampler(host):
    a = np.empty(1000)
    host.hst_twister_stream(C.c_uint64(42), C.c_int64(1000), C.c_double(0.0), C.c_double(np.sqrt(0.9)), _p(a))
    assert np.array_equal(a, orc.normal_stream(42, 1000, 0.0, np.sqrt(0.9)))


def _mppi_params(d):
    return _arr([d["wheel_radius"], d["wheel_base"], d["lam"], d["max_wheel_vel"], d["ul_var"], d["ur_var"], d["horizon"],
                 d["dt"]] + d["Q"] + d["R"] + d["P1"])


@pytest.mark.gpu
def test_mppi_class_surface_matches_oracle_with_seeded_twister(host, gpu_pkg):
    """controller::MPPI::newControls draws its own noise from rigid2d::getTwister(): with the twister
    seeded, three ticks equal three oracle ticks fed the same stream (control vector <= 1e-9)."""
    d = dict(MPPI_BASE, rollouts=64)
    T, K, n_ticks = 25, 64, 3
    out = np.empty(2 * n_ticks); u_dev = np.empty((2, T))
    got_T = host.hst_mppi_tick(_p(_mppi_params(d)), K, C.c_uint64(7), _p(_arr(WAYPOINTS[1])), _p(_arr([0.0, 0.0, 0.0])),
                               n_ticks, _p(out), _p(u_dev))
    assert got_T == T, host.hst_last_error()
    stream = orc.normal_stream(7, n_ticks * K * T * 2, 0.0, np.sqrt(0.9)).reshape(n_ticks, K, T, 2)
    u = np.zeros((2, T))
    for t in range(n_ticks):
        ref = orc.mppi_new_controls(d, u, (0, 0), WAYPOINTS[1], (0, 0, 0), stream[t])
        u = ref["u"]
        assert np.allclose(out[2 * t:2 * t + 2], ref["out"], rtol=1e-9, atol=1e-12)
    assert np.allclose(u_dev, u, rtol=1e-9, atol=1e-12)


@pytest.mark.gpu
def test_mppi_class_with_n_gpus_matches_the_oracle(host, gpu_pkg):
    """controller::MPPI(..., rollouts, n_gpus = 4) (not in the reference): the ensemble's 256 rollouts split over
    four members — all on device 0 here, so the records travel by in-process copies; on four devices the same calls go through
    one grouped ncclAllGather — host twister seeded: three ticks equal the oracle fed the same stream, as with one GPU."""
    d = dict(MPPI_BASE, rollouts=256)
    T, K, n_ticks = 25, 256, 3
    out = np.empty(2 * n_ticks); u_dev = np.empty((2, T))
    host.hst_mppi_gpus(4)
    try:
        got_T = host.hst_mppi_tick(_p(_mppi_params(d)), K, C.c_uint64(9), _p(_arr(WAYPOINTS[1])), _p(_arr([0.0, 0.0, 0.0])),
                                   n_ticks, _p(out), _p(u_dev))
    finally:
        host.hst_mppi_gpus(1)
    assert got_T == T, host.hst_last_error()
    stream = orc.normal_stream(9, n_ticks * K * T * 2, 0.0, np.sqrt(0.9)).reshape(n_ticks, K, T, 2)
    u = np.zeros((2, T))
    for t in range(n_ticks):
        ref = orc.mppi_new_controls(d, u, (0, 0), WAYPOINTS[1], (0, 0, 0), stream[t])
        u = ref["u"]
        assert np.allclose(out[2 * t:2 * t + 2], ref["out"], rtol=1e-9, atol=1e-12)
    assert np.allclose(u_dev, u, rtol=1e-9, atol=1e-12)


def _closed_loop(host, d, K, max_ticks, seed=3, odometry_mode=0):
    wp = _arr(WAYPOINTS).copy()
    traj = np.zeros((max_ticks, 5)); reached = C.c_int(); dev = C.c_double()
    ticks = host.hst_mppi_closed_loop(_p(_mppi_params(d)), K, C.c_uint64(seed), _p(wp), 5, C.c_double(0.05), C.c_double(60.0),
                                      max_ticks, _p(traj), C.byref(reached), C.c_int(odometry_mode), C.byref(dev))
    assert ticks > 0, host.hst_last_error()
    _closed_loop.last_dev = dev.value
    return traj[:ticks], reached.value


@pytest.mark.gpu
def test_cfg1_closed_loop_plumbing(host, gpu_pkg):
    """BASELINE configs[0] (K=64, T=25, diff-drive kinematics, 5-waypoint path): the whole chain
    newControls -> DiffDrive::wheelsToTwist -> plant feedforward(twist/60) -> pose -> waypoint switch
    (mppi_waypoints_node.cpp:226-305, fake_diff_encoders_node.cpp:105-113) runs and drives toward the
    goal.  With a 0.25 s horizon this controller only creeps up to a waypoint (measured: it needs
    > 40 000 ticks for the second one), so the plumbing check is progress, not lap completion."""
    d = dict(MPPI_BASE, rollouts=64)
    traj, reached = _closed_loop(host, d, 64, 3000)
    dist = np.hypot(traj[:, 0] - WAYPOINTS[1][0], traj[:, 1] - WAYPOINTS[1][1])
    print(f"\n[cfg1 closed loop] ticks {len(traj)}, waypoints reached {reached}, distance to waypoint 1: {dist[0]:.3f} -> {dist[-1]:.3f} m")
    assert dist[-1] < 0.15 and dist[-1] < 0.2 * dist[0]
    assert np.all(np.abs(traj[:, 3:]) <= d["max_wheel_vel"] + 1e-12)


@pytest.mark.gpu
def test_cfg2_closed_loop_completes_the_pentagon(host, gpu_pkg):
    """K=1024, T=50 (BASELINE configs[1]) through the class surface: one full lap of the five waypoints
    of nuturtle_robot/config/real_waypoints.yaml (measured on MI355X: ~2000 ticks at 60 Hz)."""
    d = dict(MPPI_BASE, rollouts=1024, horizon=0.5)
    traj, reached = _closed_loop(host, d, 1024, 6000)
    print(f"\n[cfg2 closed loop] ticks {len(traj)}, waypoints reached {reached}")
    assert reached == 5


@pytest.mark.gpu
def test_closed_loop_through_wrapped_encoders_and_odometry(host, gpu_pkg):
    """MPPI -> wheelsToTwist -> plant feedforward(twist/60) -> encoders wrapped to [-pi, pi)
    -> updateOdometry -> pose -> MPPI, on the HIP path, over a full lap (thousands of ticks, many encoder
    wraps).  The odometry pose the controller steers by must stay on the plant's true pose."""
    d = dict(MPPI_BASE, rollouts=1024, horizon=0.5)
    traj, reached = _closed_loop(host, d, 1024, 6000, odometry_mode=1)
    print(f"\n[closed loop via encoders] ticks {len(traj)}, waypoints reached {reached}")
    assert reached == 5
    # the odometry the controller steers by (integrated from WRAPPED encoder angles) stays on the plant's pose
    print(f"   max |odometry pose - plant pose| over the lap: {_closed_loop.last_dev:.3e}")
    assert _closed_loop.last_dev < 1e-9
    assert np.all(np.abs(traj[:, 3:]) <= d["max_wheel_vel"] + 1e-12)


@pytest.mark.gpu
def test_closed_loop_with_exact_arc_rollouts(host, gpu_pkg):
    """SURVEY.md 8-f N4 in the loop: the controller integrates its rollouts with the plant's own arc step
    (controller::MPPI::useExactArcDynamics) and still laps the pentagon through the wrapped-encoder odometry chain."""
    d = dict(MPPI_BASE, rollouts=1024, horizon=0.5)
    traj, reached = _closed_loop(host, d, 1024, 6000, odometry_mode=3)
    assert reached == 5, f"only {reached} of 5 waypoints in {len(traj)} ticks"
    assert _closed_loop.last_dev < 1e-9
    print(f"   arc-dynamics lap: {len(traj)} ticks")


@pytest.mark.gpu
@pytest.mark.parametrize("reference_field", [0, 1])
def test_particle_filter_class_surface_end_to_end(host, gpu_pkg, reference_field):
    """bmapping::ParticleFilter driven like turtle_mapping_node.cpp:459-494 (SLAM, getRobotState,
    newMap).  No distance-field injection.  By DEFAULT (round 3: the reference's own distance field up to 4096 particles)
    the class IS the reference filter: best pose to 1e-9, Neff and the exported map identical.  After
    ParticleFilter::useExactDistanceField() (the fast mode): best pose within 1 mm, exported maps agree on >= 99 % of cells."""
    N, k, n_scans = 40, 50, 5
    host.hst_pf_reference_field(reference_field)   # 1: the class's DEFAULT (the reference's field); 0: useExactDistanceField()
    steps, poses = rc.trajectory(n_scans, inc=(0.04, 0.03, 0.02))
    rng = np.random.default_rng(3)
    scans = np.stack([orc.room_scan(poses[s], walls=rc.ROOM_SMALL, rng=rng) for s in range(n_scans)])
    odom = np.stack([steps[0][0]] + [st[1] for st in steps])
    out_pose = np.empty((n_scans, 3)); out_neff = np.empty(n_scans, dtype=np.int32); m = np.empty(80 * 80, dtype=np.int8)
    xs = host.hst_pf_run(N, k, C.c_double(2.0), C.c_uint64(11), _p(scans), 360, n_scans, _p(odom), _p(out_pose), _p(out_neff), _p(m))
    host.hst_pf_reference_field(1)
    assert xs == 80, host.hst_last_error()
    # the same run through the oracle filter: same twister stream, same ICP convention
    pf = orc.PfAPI(orc.pf_params(N=N, k=k, pose0=tuple(odom[0])))
    stream = orc.normal_stream(11, n_scans * (N * (3 * k + 3) + 1), 0.0, 1.0)
    off = 0
    for s in range(n_scans):
        prev, cur = odom[s], odom[s + 1]
        t_icp = (0.0, 0.0, 0.0) if s == 0 else rc.compose(rc.inverse(prev), cur)  # first call: identity (cloud_alignment.cpp:43-50)
        nz = stream[off:off + N * (3 * k + 3) + 1]
        tr = pf.slam(scans[s], (0, 0, 0), cur, prev, True, t_icp, nz)
        off += tr["normals_used"]
        assert tr["rc"] == 0
        po, _, _ = pf.particles()
        assert np.allclose(out_pose[s], po[pf.best()], atol=1e-9 if reference_field else 1e-3)
        if reference_field:
            assert out_neff[s] == tr["neff"]
    agree = np.mean(m == pf.grid(pf.best()).grid_map())
    print(f"\n[pf class surface, reference_field={reference_field}] Neff {out_neff.tolist()}, exported map agreement {agree*100:.2f} %")
    assert agree == 1.0 if reference_field else agree >= 0.99


@pytest.mark.gpu
def test_particle_filter_class_with_n_gpus_equals_one_gpu(host, gpu_pkg):
    """bmapping::ParticleFilter(..., n_gpus = 4) (not in the reference): the 40 particles of the launch
    configuration over four members (device 0 four times on this box: copy transport; on four devices RCCL), the filter's
    twister seeded — best pose per scan, Neff and the exported map identical to the same class on one GPU in the same
    (exact) distance-field mode: sharding changes nothing but where a particle lives."""
    N, k, n_scans = 40, 50, 6
    steps, poses = rc.trajectory(n_scans, inc=(0.04, 0.03, 0.02))
    rng = np.random.default_rng(3)
    scans = np.stack([orc.room_scan(poses[s], walls=rc.ROOM_SMALL, rng=rng) for s in range(n_scans)])
    odom = np.stack([steps[0][0]] + [st[1] for st in steps])
    res = []
    for gpus in (1, 4):
        out_pose = np.empty((n_scans, 3)); out_neff = np.empty(n_scans, dtype=np.int32); m = np.empty(80 * 80, dtype=np.int8)
        host.hst_pf_reference_field(0); host.hst_pf_gpus(gpus)
        try:
            xs = host.hst_pf_run(N, k, C.c_double(2.0), C.c_uint64(11), _p(scans), 360, n_scans, _p(odom), _p(out_pose), _p(out_neff), _p(m))
        finally:
            host.hst_pf_reference_field(1); host.hst_pf_gpus(1)
        assert xs == 80, host.hst_last_error()
        res.append((out_pose, out_neff, m))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


def test_node_call_sites_compile_against_these_headers():
    """host/test/node_calls.cpp spells every call turtle_mapping_node.cpp / mppi_waypoints_node.cpp make on the hot-path
    classes; build() compiles it (host/Makefile), so the object must be there and newer than the headers' users."""
    obj = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "obj", "node_calls.o")
    assert os.path.exists(obj), "run __graft_entry__.build()"


@pytest.mark.gpu
@pytest.mark.parametrize("reference_field", [0, 1])
def test_grid_mapper_class_surface_against_the_oracle(host, gpu_pkg, reference_field):
    """bmapping::GridMapper as a class of its own (grid_mapper.hpp:128-140): integrateScan / likelihoodFieldModel /
    gridMap / laserEndPoints / value copies, against the oracle's GridMapper (pinned to the compiled reference).
    With useReferenceDistanceField() the likelihood is the reference's to 1e-9; by default (exact field) it is close."""
    host.hst_gm_create.restype = C.c_void_p
    host.hst_gm_clone.restype = C.c_void_p
    grid = _arr([0.05, -2.0, 2.0, -2.0, 2.0]); laser = orc.lds01_laser(); trs = _arr([0.0, 0.0, 0.0])
    g = C.c_void_p(host.hst_gm_create(_p(grid), _p(laser), _p(orc.MIX), _p(trs), reference_field))
    assert g.value, host.hst_last_error()
    o = orc.GridAPI("orc", grid=tuple(grid))
    steps, poses = rc.trajectory(4, inc=(0.04, 0.03, 0.02))
    rng = np.random.default_rng(4)
    lik = C.c_double()
    for s in range(4):
        scan = orc.room_scan(poses[s], walls=rc.ROOM_SMALL, rng=rng)
        pose = _arr(poses[s])
        probe = _arr(poses[s] + np.array([0.01, 0.02, -0.015]))
        assert host.hst_gm_likelihood(g, _p(scan), 360, _p(probe), C.byref(lik)) == 0, host.hst_last_error()
        want, err = o.likelihood(scan, probe)
        assert err == 0
        if reference_field or s == 0:
            assert abs(lik.value - want) <= 1e-9 * abs(want), (s, lik.value, want)
        else:
            assert abs(lik.value - want) <= 0.05 * abs(want), (s, lik.value, want)
        xy = np.empty((360, 2))
        n = host.hst_gm_end_points(g, _p(scan), 360, _p(pose), _p(xy))
        assert n == 360 and np.array_equal(xy[:n], o.end_points(scan, pose))          # LaserScanner::laserEndPoints, bit-exact
        assert host.hst_gm_integrate_scan(g, _p(scan), 360, _p(pose)) == 0, host.hst_last_error()
        o.integrate_scan(scan, pose)
        m = np.empty(80 * 80, dtype=np.int8)
        assert host.hst_gm_grid_map(g, _p(m), m.size) == m.size
        assert np.array_equal(m, o.grid_map())                                        # gridMap, bit-exact
    # value semantics: a copy maps on its own
    g2 = C.c_void_p(host.hst_gm_clone(g)); o2 = o.clone()
    scan = orc.room_scan(poses[3], walls=rc.ROOM_SMALL, rng=rng)
    assert host.hst_gm_integrate_scan(g2, _p(scan), 360, _p(_arr(poses[3]))) == 0
    o2.integrate_scan(scan, poses[3])
    m2 = np.empty(80 * 80, dtype=np.int8); m1 = np.empty(80 * 80, dtype=np.int8)
    host.hst_gm_grid_map(g2, _p(m2), m2.size); host.hst_gm_grid_map(g, _p(m1), m1.size)
    assert np.array_equal(m2, o2.grid_map()) and np.array_equal(m1, o.grid_map()) and not np.array_equal(m1, m2)
    if reference_field:
        assert host.hst_gm_likelihood(g2, _p(scan), 360, _p(_arr(poses[3])), C.byref(lik)) == 0
        want, _ = o2.likelihood(scan, poses[3])
        assert abs(lik.value - want) <= 1e-9 * abs(want)
    # the reference's exception, as an exception
    far = np.full(360, 3.0, dtype=np.float32)
    assert host.hst_gm_integrate_scan(g, _p(far), 360, _p(_arr([0.0, 1.5, 1.5]))) == 1
    assert b"NOT in the bounds of the world" in host.hst_last_error()
    host.hst_gm_destroy(g); host.hst_gm_destroy(g2); o.close(); o2.close()


@pytest.mark.gpu
def test_grid_mapper_default_field_likelihood_is_the_exact_field_s(host, gpu_pkg):
    """GridMapper::likelihoodFieldModel in the DEFAULT mode (rbpf_likelihood_one with query-mode lookups: no LDS slice, the row
    walks on the global bitmap, inlined) at 1e-9 against the oracle's GridMapper over the exact field — the brute-force transform
    of the oracle's own occupied cells, injected through set_occ_dist (tests/test_oracle_exact_field.py pins that to the oracle's
    exact_field switch, bit for bit).  Shipped 80 x 80 map, ROOM_SMALL, three scans integrated on both sides, the fourth scan
    scored at: its own pose; two poses a few centimetres off; a pose far enough out that most beams end well away from every
    occupied cell (the walks go rows deep); a pose from which beams leave the world (both sides report it).
    The "unreached" fallback itself cannot occur on this map: cell_radius is 200 cells (max_occ_dist 10 m at 0.05 m) and no two
    cells of an 80 x 80 map are more than 112 apart, so once a cell is occupied every cell has an obstacle within reach (asserted
    below).  The far pose asks for what the map does allow: beams whose nearest obstacle is beyond the three cells a 7 x 7
    look would settle, up to ten cells away."""
    host.hst_gm_create.restype = C.c_void_p
    grid = _arr([0.05, -2.0, 2.0, -2.0, 2.0]); laser = orc.lds01_laser(); trs = _arr([0.0, 0.0, 0.0])
    g = C.c_void_p(host.hst_gm_create(_p(grid), _p(laser), _p(orc.MIX), _p(trs), 0))
    assert g.value, host.hst_last_error()
    o = orc.GridAPI("orc", grid=tuple(grid))
    _, poses = rc.trajectory(4, inc=(0.04, 0.03, 0.02))
    rng = np.random.default_rng(4)
    scans = [orc.room_scan(poses[s], walls=rc.ROOM_SMALL, rng=rng) for s in range(4)]
    for s in range(3):
        assert host.hst_gm_integrate_scan(g, _p(scans[s]), 360, _p(_arr(poses[s]))) == 0, host.hst_last_error()
        assert o.integrate_scan(scans[s], poses[s]) == 0
    occ = np.zeros(o.G, dtype=np.uint8)
    occ[o.occ_cells()] = 1
    radius = int(o.constants()[3])
    codes = orc.exact_edt_codes(occ.reshape(o.xsize, o.ysize), radius, np.full((o.xsize, o.ysize), 0xFFFF, np.uint16))
    assert radius == 200 and occ.any() and codes.max() < 0xFFFF       # (no cell out of reach: see above)
    o.set_occ_dist((np.sqrt(codes.astype(np.float64)) * 0.05).ravel())
    scan, own = scans[3], np.array(poses[3])

    def end_codes(q):
        xy = o.end_points(scan, q)
        return codes[np.floor((xy[:, 0] + 2.0) / 0.05).astype(int), np.floor((xy[:, 1] + 2.0) / 0.05).astype(int)]

    far = own + np.array([0.1, 0.35, -0.25])
    assert end_codes(own).max() <= 9 and (end_codes(far) > 9).sum() > 180 and end_codes(far).max() > 81
    lik = C.c_double()
    for q in (own, own + np.array([0.01, 0.02, -0.015]), own + np.array([-0.02, -0.03, 0.04]), far):
        want, err = o.likelihood(scan, q)
        assert err == 0 and want > 0.0
        assert host.hst_gm_likelihood(g, _p(scan), 360, _p(_arr(q)), C.byref(lik)) == 0, host.hst_last_error()
        print("likelihood at", q, ":", lik.value, "oracle", want, "rel", abs(lik.value - want) / want)
        assert abs(lik.value - want) <= 1e-9 * abs(want), (q, lik.value, want)
    out = own + np.array([0.0, 0.6, 0.0])
    assert o.likelihood(scan, out)[1] != 0
    assert host.hst_gm_likelihood(g, _p(scan), 360, _p(_arr(out)), C.byref(lik)) == 1
    assert b"NOT in the bounds of the world" in host.hst_last_error()
    host.hst_gm_destroy(g); o.close()


@pytest.mark.gpu
@pytest.mark.parametrize("odometry_mode", [0, 1])
def test_closed_loop_tick_sequence_equals_the_oracle_loop(host, gpu_pkg, odometry_mode):
    """SURVEY.md 8-f N3 as PARITY, not only as a property: the first 200 ticks of the closed loop
    (mppi_waypoints_node.cpp:226-305: waypoint switch -> newControls -> wheelsToTwist -> plant feedforward(twist / 60)
    [-> wrapped encoders -> updateOdometry]) on the HIP path, against the same loop run with the oracle (MPPI restatement
    + the DiffDrive restatement that is pinned bit-exact to the reference build), both consuming the same seeded
    mt19937_64 stream.  Controls and poses tick by tick within 1e-9."""
    d = dict(MPPI_BASE, rollouts=64)  # BASELINE configs[0]: K=64, T=25
    K, T, n_ticks, seed, rate, goal = 64, 25, 200, 3, 60.0, 0.05
    wp = _arr(WAYPOINTS).copy()
    traj = np.zeros((n_ticks, 5)); reached = C.c_int(); dev = C.c_double()
    ticks = host.hst_mppi_closed_loop(_p(_mppi_params(d)), K, C.c_uint64(seed), _p(wp), 5, C.c_double(goal), C.c_double(rate),
                                      n_ticks, _p(traj), C.byref(reached), C.c_int(odometry_mode), C.byref(dev))
    assert ticks == n_ticks, host.hst_last_error()
    # ---- the oracle's loop
    r = orc.RigidAPI("orc")
    start = [wp[0][2], wp[0][0], wp[0][1]]  # (theta, x, y)
    plant, odometer, model = (r.dd_create(start, d["wheel_base"], d["wheel_radius"]) for _ in range(3))
    stream = orc.normal_stream(seed, n_ticks * K * T * 2, 0.0, np.sqrt(d["ul_var"])).reshape(n_ticks, K, T, 2)
    u = np.zeros((2, T))
    target, n_reached = 1, 0
    worst_u = worst_pose = 0.0
    for t in range(n_ticks):
        st = r.dd_state(odometer if odometry_mode else plant)
        th, x, y = st[0], st[1], st[2]
        if np.sqrt((x - wp[target][0]) ** 2 + (y - wp[target][1]) ** 2) < goal:
            n_reached += 1
            target = (target + 1) % 5
        ref = orc.mppi_new_controls(d, u, (0.0, 0.0), tuple(wp[target]), (x, y, th), stream[t])
        u = ref["u"]
        cmd = r.dd_wheels_to_twist(model, ref["out"])
        assert r.dd_feedforward(plant, [cmd[0] / rate, cmd[1] / rate, 0.0]) == 0
        ps = r.dd_state(plant)
        if odometry_mode:
            r.dd_update_odometry(odometer, ps[3], ps[4])
        worst_u = max(worst_u, float(np.max(np.abs(traj[t, 3:5] - ref["out"]) / np.maximum(np.abs(ref["out"]), 1e-3))))
        worst_pose = max(worst_pose, float(np.max(np.abs(traj[t, :3] - np.array([ps[1], ps[2], ps[0]])))))
    print(f"\n[closed loop vs oracle, odometry_mode={odometry_mode}] {n_ticks} ticks: max rel. control diff {worst_u:.2e}, max pose diff {worst_pose:.2e}")
    assert worst_u <= 1e-9 and worst_pose <= 1e-9
    assert n_reached == reached.value
    for dd in (plant, odometer, model):
        r.dd_destroy(dd)
