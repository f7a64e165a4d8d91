"""The device ICP's point-to-line metric (include/tbnav_icp.h POINT-TO-LINE METRIC, csrc/icp.hip icp_align<LineMetric>) against the
numpy restatement of that contract (tests/icp_line_restatement.py), bit for bit, through every layer: the C-ABI (set_metric /
get_metric / normals / match / step / step_batch), the Python mirror (rtn_amd.icp.ScanAlignment(metric="line")) and the C++
ScanAlignment::useDeviceICP(device, ICPMetric::PointToLine) inside bmapping::ParticleFilter.  The metric has no counterpart in
the reference."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import icp_line_restatement as LR
import icp_restatement as R
import oracle_api as orc
import rbpf_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "libtbnav_host.so")
CORRIDOR = (-50, 50, -1, 1)

pytestmark = pytest.mark.gpu


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _laser(params):
    return R.Laser(params.beam_min, params.beam_max, params.beam_delta, params.range_min, params.range_max)


def _aligner(gpu_pkg, metric="line", normal_window=0, normal_max_gap=0.0, **kw):
    from rtn_amd import icp
    p = icp.default_params(**kw)
    return icp.ScanAlignment(p, metric=metric, normal_window=normal_window, normal_max_gap=normal_max_gap), p


def _same(got, want: R.Result, where=""):
    ok, T, info = got
    assert ok == want.ok, (where, got, want)
    assert (info["iterations"], info["criterion"], info["correspondences"]) == (want.iterations, want.criterion, want.correspondences), (where, info, want)
    assert info["mse"] == want.mse, (where, info["mse"], want.mse)
    assert tuple(T) == tuple(want.T), (where, T, want.T)


def _run(room, inc, n, seed, n_beams=360, beam_delta_deg=1.0):
    steps, poses = rc.trajectory(n, inc=inc)
    rng = np.random.default_rng(seed)
    scans = np.stack([orc.room_scan(p, n_beams=n_beams, beam_delta_deg=beam_delta_deg, walls=room, rng=rng) for p in poses])
    return steps, poses, scans


def test_normals_are_the_restatements(gpu_pkg):
    rng = np.random.default_rng(5)
    scan = orc.room_scan((0.3, 0.1, -0.2), walls=rc.ROOM_SURVEY, rng=rng)
    scan[[0, 7, 100, 101, 103]] = [np.nan, np.inf, -np.inf, np.float32(0.05), np.float32(0.12)]
    scan[200] = np.float32(0.5)     # a lone point in front of its wall
    scan[359] = np.float32(3.5)     # range_max: out
    big = orc.room_scan((0.0, 0.2, 0.1), n_beams=1080, beam_delta_deg=1.0 / 3.0, walls=rc.ROOM_BENCH, rng=rng)
    big[::97] = np.nan
    big[500:520] = np.inf
    cases = [(dict(), scan), (dict(Trs=(0.4, -0.07, 0.05)), scan), (dict(beam_delta_deg=1.0 / 3.0, Trs=(-0.2, 0.03, 0.0)), big)]
    for kw, sc in cases:
        for window, gap in ((1, 0.0), (9, 0.0), (9, 0.1), (16, 1.0)):
            a, p = _aligner(gpu_pkg, normal_window=window, normal_max_gap=gap, **kw)
            nxy, has = a.normals(sc)
            want_n, want_h = LR.normals(sc, _laser(p), tuple(p.Trs), window=window, max_gap=gap if gap else LR.NORMAL_MAX_GAP)
            assert np.array_equal(has, want_h), (kw, window, gap)
            assert np.array_equal(nxy.view(np.uint32), want_n.view(np.uint32)), (kw, window, gap)
            assert 0 < has.sum() < sc.size
            a.close()


@pytest.mark.parametrize("room,inc", [(rc.ROOM_BENCH, rc.TRAJ_BENCH), (rc.ROOM_SURVEY, rc.TRAJ_SURVEY)])
def test_match_is_the_restatement_bit_for_bit(gpu_pkg, room, inc):
    from rtn_amd import icp
    a, p = _aligner(gpu_pkg)
    L = _laser(p)
    steps, poses, scans = _run(room, inc, 6, 11)
    for s in range(1, 6):
        g = icp.init_guess(poses[s], poses[s - 1])
        for guess in (g, (g[0] + math.radians(3.0), g[1] + 0.05, g[2] - 0.05)):
            want = LR.match(scans[s - 1], scans[s], L, guess)
            assert want.ok
            _same(a.pclICP(guess, scans[s - 1], scans[s]), want, (room, s, guess))
    a.close()


def test_match_1080_beams_a_laser_offset_and_window_9(gpu_pkg):
    from rtn_amd import icp
    a, p = _aligner(gpu_pkg, normal_window=9, beam_delta_deg=1.0 / 3.0, Trs=(0.1, -0.05, 0.02))
    L = _laser(p)
    steps, poses, scans = _run(rc.ROOM_BENCH, rc.TRAJ_BENCH, 4, 3, n_beams=1080, beam_delta_deg=1.0 / 3.0)
    for s in range(1, 4):
        g = icp.init_guess(poses[s], poses[s - 1])
        want = LR.match(scans[s - 1], scans[s], L, g, Trs=tuple(p.Trs), window=9)
        assert want.ok
        _same(a.pclICP(g, scans[s - 1], scans[s]), want, s)
        a.setMetric("line", 1)
        _same(a.pclICP(g, scans[s - 1], scans[s]), LR.match(scans[s - 1], scans[s], L, g, Trs=tuple(p.Trs), window=1), (s, 1))
        a.setMetric("line", 9)
    a.close()


def test_failures_and_max_iter(gpu_pkg):
    a, p = _aligner(gpu_pkg)
    L = _laser(p)
    scan = orc.room_scan((0.0, 0.0, 0.0), walls=rc.ROOM_BENCH)
    bad = np.full(360, np.nan, dtype=np.float32)
    for tgt, src in ((scan, bad), (bad, scan)):
        want = LR.match(tgt, src, L, (0, 0, 0))
        assert want.criterion == R.NO_CORRESPONDENCES
        _same(a.pclICP((0, 0, 0), tgt, src), want)
    small = orc.room_scan((0.0, 0.0, 0.0), walls=(-0.6, 0.6, -0.6, 0.6))
    want = LR.match(small, small, L, (0.0, 2.0, 0.0))
    assert want.criterion == R.NO_CORRESPONDENCES
    _same(a.pclICP((0.0, 2.0, 0.0), small, small), want)
    # a target whose points all stand alone: valid points, no normal, nothing paired
    sparse = np.full(360, np.nan, dtype=np.float32)
    sparse[::4] = scan[::4]
    want = LR.match(sparse, scan, L, (0, 0, 0))
    assert want.criterion == R.NO_CORRESPONDENCES and want.correspondences == 0
    _same(a.pclICP((0, 0, 0), sparse, scan), want)
    # the noise-free corridor: DEGENERATE; with noise it converges and keeps the guess along the corridor
    c0 = orc.room_scan((0.0, 0.0, 0.0), walls=CORRIDOR)
    c1 = orc.room_scan((0.0, 0.05, 0.0), walls=CORRIDOR)
    want = LR.match(c0, c1, L, (0.0, 0.05, 0.0))
    assert want.criterion == R.DEGENERATE and not want.ok and want.T == (0.0, 0.0, 0.0)
    got = a.pclICP((0.0, 0.05, 0.0), c0, c1)
    assert got[2]["criterion"] == gpu_pkg.capi.ICP_DEGENERATE
    _same(got, want)
    rng = np.random.default_rng(2)
    n0 = orc.room_scan((0.0, 0.0, 0.0), walls=CORRIDOR, rng=rng)
    n1 = orc.room_scan((0.0, 0.05, 0.0), walls=CORRIDOR, rng=rng)
    want = LR.match(n0, n1, L, (0.0, 0.05, 0.0))
    assert want.ok and abs(want.T[1] - 0.05) < 0.005
    _same(a.pclICP((0.0, 0.05, 0.0), n0, n1), want)
    a.close()
    one, p1 = _aligner(gpu_pkg, max_iter=1)
    b = orc.room_scan((0.05, 0.07, 0.02), walls=rc.ROOM_BENCH)
    got = one.pclICP((0, 0, 0), scan, b)
    assert got[0] and got[2]["criterion"] == gpu_pkg.capi.ICP_ITERATIONS and got[2]["iterations"] == 1
    _same(got, LR.match(scan, b, L, (0, 0, 0), max_iter=1))
    one.close()


def test_step_failure_and_set_metric_keep_the_stored_scan(gpu_pkg):
    a, p = _aligner(gpu_pkg)
    L = _laser(p)
    s0 = orc.room_scan((0.0, 0.0, 0.0), walls=rc.ROOM_BENCH, rng=np.random.default_rng(1))
    s1 = orc.room_scan((0.03, 0.05, 0.01), walls=rc.ROOM_BENCH, rng=np.random.default_rng(2))
    s2 = orc.room_scan((0.05, 0.09, 0.03), walls=rc.ROOM_BENCH, rng=np.random.default_rng(3))
    bad = np.full(360, np.inf, dtype=np.float32)
    ok, T, info = a.pclICPWrapper((0.5, 0.5, 0.5), s0)
    assert ok and T == (0.0, 0.0, 0.0) and info["criterion"] == gpu_pkg.capi.ICP_NOT_RUN
    ok, T, info = a.pclICPWrapper((0.0, 0.0, 0.0), bad)
    assert not ok and info["criterion"] == gpu_pkg.capi.ICP_NO_CORRESPONDENCES
    _same(a.pclICPWrapper((0.0, 0.05, 0.01), s1), LR.match(s0, s1, L, (0.0, 0.05, 0.01)))   # aligned against s0, not bad
    a.setMetric("point")
    _same(a.pclICPWrapper((0.0, 0.04, 0.02), s2), R.match(s1, s2, L, (0.0, 0.04, 0.02)))     # the stored scan survived: s1
    a.setMetric("line", 3, 0.2)
    _same(a.pclICPWrapper((0.0, -0.09, -0.03), s0), LR.match(s2, s0, L, (0.0, -0.09, -0.03), window=3, max_gap=0.2))
    a.reset()
    assert a.pclICPWrapper((0.0, 0.0, 0.0), s1)[2]["criterion"] == gpu_pkg.capi.ICP_NOT_RUN
    assert a.metric() == ("line", 3, 0.2)    # reset forgets the scan, not the metric
    a.close()


def _planted_run(n=200):
    from rtn_amd import icp
    steps, poses, scans = _run(rc.ROOM_BENCH, (0.01, 0.006, 0.003), n, 17)
    bad = [37, 90, 91, 150, 199]   # one alone, two in a row, the last
    for s in bad:
        scans[s] = np.float32(np.nan) if s % 2 else np.float32(np.inf)
    T_init = np.array([icp.init_guess(poses[s], poses[s - 1] if s else poses[0]) for s in range(n)])
    return scans, T_init, bad


def test_step_batch_is_n_steps_and_the_restatement(gpu_pkg):
    scans, T_init, bad = _planted_run()
    n = len(scans)
    a, p = _aligner(gpu_pkg)
    one = [a.pclICPWrapper(T_init[s], scans[s]) for s in range(n)]
    b, _ = _aligner(gpu_pkg)
    ok, T, info = b.wrapperBatch(T_init, scans)
    launches = b.lastBatchLaunches()
    for s in range(n):
        assert bool(ok[s]) == one[s][0] and tuple(T[s]) == one[s][1] and info[s] == one[s][2], s
    w = LR.Wrapper(_laser(p))
    for s in range(n):
        _same((bool(ok[s]), tuple(T[s]), info[s]), w.step(scans[s], T_init[s]), s)
    failed = [s for s in range(n) if not ok[s]]
    assert failed == bad, failed
    assert launches > 1, "a failure must realign the pairs that depended on it"
    # the point metric on the same run gives other numbers: the batch did run the line metric, in every launch
    c, _ = _aligner(gpu_pkg, metric="point")
    okp, Tp, infop = c.wrapperBatch(T_init, scans)
    assert np.array_equal(okp, ok) and not np.array_equal(Tp, T)
    assert all(infop[s]["mse"] != info[s]["mse"] for s in range(1, n) if ok[s])
    # two repeats are bit-identical
    b.reset()
    ok2, T2, info2 = b.wrapperBatch(T_init, scans)
    assert np.array_equal(ok, ok2) and np.array_equal(T.view(np.uint64), T2.view(np.uint64)) and info == info2
    a.close(); b.close(); c.close()


def test_line_then_point_reproduces_the_point_restatement(gpu_pkg):
    """The two kernels do not leak into each other: after set_metric(LINE) and a line alignment, set_metric(POINT) gives
    exactly what icp_restatement.match gives (and what a handle that never left the point metric gives)."""
    from rtn_amd import icp
    a, p = _aligner(gpu_pkg, metric="point")
    fresh, _ = _aligner(gpu_pkg, metric="point")
    L = _laser(p)
    steps, poses, scans = _run(rc.ROOM_SURVEY, rc.TRAJ_SURVEY, 4, 23)
    for s in range(1, 4):
        g = icp.init_guess(poses[s], poses[s - 1])
        a.setMetric("line", 5, 0.3)
        _same(a.pclICP(g, scans[s - 1], scans[s]), LR.match(scans[s - 1], scans[s], L, g, window=5, max_gap=0.3), ("line", s))
        a.setMetric("point")
        got = a.pclICP(g, scans[s - 1], scans[s])
        _same(got, R.match(scans[s - 1], scans[s], L, g), ("point", s))
        assert got == fresh.pclICP(g, scans[s - 1], scans[s])
    a.close(); fresh.close()


def test_set_metric_checks_its_arguments_and_get_metric_returns_them(gpu_pkg):
    from rtn_amd import icp
    capi = gpu_pkg.capi
    a, p = _aligner(gpu_pkg, metric="point")
    assert a.metric() == ("point", 1, 0.25)                       # a new handle
    a.setMetric("line", 7, 0.4)
    assert a.metric() == ("line", 7, 0.4)
    L = capi.lib()
    for metric, window in ((2, 1), (-1, 1), (capi.ICP_METRIC_LINE, 17), (capi.ICP_METRIC_POINT, 17)):
        assert L.tbnav_icp_set_metric(a._h, metric, window, 0.1) == capi.ERR_INVALID_ARG, (metric, window)
        assert a.metric() == ("line", 7, 0.4)                     # a refused call changes nothing
    assert L.tbnav_icp_set_metric(None, 0, 1, 0.1) == capi.ERR_INVALID_ARG
    a.setMetric("line", 0, -1.0)                                  # <= 0: the defaults
    assert a.metric() == ("line", 1, 0.25)
    a.setMetric("line", 16, 0.0)
    assert a.metric() == ("line", 16, 0.25)
    a.setMetric("point", 4, 0.5)                                  # stored with either metric
    assert a.metric() == ("point", 4, 0.5)
    with pytest.raises(ValueError):
        a.setMetric("plane")
    with pytest.raises(ValueError):
        icp.ScanAlignment(p, metric="plane")
    # the line metric's beam limit: 2048 beams align, more are refused; the point metric takes them
    a.setMetric("line")
    wide = np.full(capi.ICP_LINE_MAX_BEAMS + 4, 1.0, dtype=np.float32)
    with pytest.raises(capi.TbnavError):
        a.pclICP((0, 0, 0), wide, wide)
    with pytest.raises(capi.TbnavError):
        a.normals(wide)
    a.setMetric("point")
    assert a.pclICP((0, 0, 0), wide, wide)[0]
    a.pclICPWrapper((0, 0, 0), wide)                              # stored with 2052 beams
    assert L.tbnav_icp_set_metric(a._h, capi.ICP_METRIC_LINE, 0, 0.0) == capi.ERR_INVALID_ARG
    assert a.metric()[0] == "point"
    a.close()


def test_2048_beams_run_with_the_line_metric(gpu_pkg):
    """The limit itself: 2048 beams (32 KB of cloud and normals beside the tree's LDS), bit for bit."""
    n = 2048
    a, p = _aligner(gpu_pkg, normal_window=4, beam_delta_deg=360.0 / n)
    L = _laser(p)
    rng = np.random.default_rng(31)
    s0 = orc.room_scan((0.0, 0.0, 0.0), n_beams=n, beam_delta_deg=360.0 / n, walls=rc.ROOM_BENCH, rng=rng)
    s1 = orc.room_scan((0.02, 0.04, 0.01), n_beams=n, beam_delta_deg=360.0 / n, walls=rc.ROOM_BENCH, rng=rng)
    want = LR.match(s0, s1, L, (0.0, 0.0, 0.0), window=4)
    assert want.ok
    _same(a.pclICP((0.0, 0.0, 0.0), s0, s1), want)
    a.close()


@pytest.fixture(scope="module")
def host(pkg):
    pkg.capi.lib()
    L = C.CDLL(HOST_LIB)
    L.hst_icp_last_error.restype = C.c_char_p
    L.hst_icp_pf_run_metric.restype = C.c_int
    L.hst_icp_pf_run_metric.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_uint64] + [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
    return L


def test_particle_filter_class_with_the_line_metric(host, gpu_pkg):
    """bmapping::ScanAlignment::useDeviceICP(-1, ICPMetric::PointToLine) inside bmapping::ParticleFilter: the (ok, T) the
    class's matcher returns per scan equals the restatement's wrapper (and the Python mirror's), and the best pose / Neff equal
    the oracle filter fed those same (ok, T) — the tolerances of test_particle_filter_class_with_device_icp."""
    from rtn_amd import icp
    N, k, n_scans = 40, 50, 6
    steps, poses = rc.trajectory(n_scans, inc=(0.04, 0.03, 0.02))
    rng = np.random.default_rng(3)
    scans = np.stack([orc.room_scan(poses[s], walls=rc.ROOM_SMALL, rng=rng) for s in range(n_scans)])
    odom = np.stack([steps[0][0]] + [st[1] for st in steps])
    u = np.array([st[3] for st in steps], dtype=np.float64)
    ok = np.zeros(n_scans, dtype=np.int32); T = np.zeros((n_scans, 3)); pose = np.zeros((n_scans, 3))
    neff = np.zeros(n_scans, dtype=np.int32)
    rcode = host.hst_icp_pf_run_metric(1, N, k, 2.0, 11, _p(scans), 360, n_scans, _p(odom), _p(u), _p(ok), _p(T), _p(pose), _p(neff))
    assert rcode == 0, host.hst_icp_last_error()
    mirror, p = _aligner(gpu_pkg)
    w = LR.Wrapper(_laser(p))
    okp = np.zeros(n_scans, dtype=np.int32); Tp = np.zeros((n_scans, 3)); posep = np.zeros((n_scans, 3))
    neffp = np.zeros(n_scans, dtype=np.int32)
    for s in range(n_scans):
        g = icp.init_guess(odom[s + 1], odom[s])
        m = mirror.pclICPWrapper(g, scans[s])
        want = w.step(scans[s], g)
        assert bool(ok[s]) == m[0] == want.ok and tuple(T[s]) == m[1] == tuple(want.T), s
    mirror.close()
    assert ok.all()
    # not the point metric's answers
    rcode = host.hst_icp_pf_run_metric(0, N, k, 2.0, 11, _p(scans), 360, n_scans, _p(odom), _p(u), _p(okp), _p(Tp), _p(posep), _p(neffp))
    assert rcode == 0, host.hst_icp_last_error()
    assert not np.array_equal(T[1:], Tp[1:])
    pf = orc.PfAPI(orc.pf_params(N=N, k=k, pose0=tuple(odom[0])))
    stream = orc.normal_stream(11, n_scans * (N * (3 * k + 3) + 1), 0.0, 1.0)
    off = 0
    for s in range(n_scans):
        nz = stream[off:off + N * (3 * k + 3) + 1]
        tr = pf.slam(scans[s], u[s], odom[s + 1], odom[s], bool(ok[s]), T[s], nz)
        off += tr["normals_used"]
        assert tr["rc"] == 0
        po, _, _ = pf.particles()
        assert np.allclose(pose[s], po[pf.best()], atol=1e-9, rtol=0), s
        assert neff[s] == tr["neff"], s
