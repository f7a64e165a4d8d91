"""The numpy restatement of the device ICP's contract (tests/icp_restatement.py, include/tbnav_icp.h) on its own (CPU):
it recovers known motions, fails where the reference's ICP fails, stops where PCL's criteria stop it, and keeps
pclICPWrapper's bookkeeping.  The GPU tests hold the kernel to this restatement bit for bit."""
import math

import numpy as np

import icp_restatement as R
import oracle_api as orc
import rbpf_cases as rc

L = R.lds01()


def _apply(T, pts):
    c, s = math.cos(T[0]), math.sin(T[0])
    return np.stack([c * pts[:, 0] - s * pts[:, 1] + T[1], s * pts[:, 0] + c * pts[:, 1] + T[2]], axis=1)


def test_noise_free_rigid_motion_is_recovered():
    """target = T * source exactly (a star-shaped closed curve, no noise): ICP from the identity recovers T to 1e-6."""
    ang = np.arange(0, 2 * np.pi, np.pi / 90)
    rad = 1.5 + 0.5 * np.cos(3 * ang)
    src = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1).astype(np.float32)
    for T in ((0.03, 0.02, -0.015), (-0.05, -0.04, 0.03)):
        tgt = _apply(T, src.astype(np.float64)).astype(np.float32)
        got = R.match_clouds(tgt, src, np.arange(len(src)), len(src), (0.0, 0.0, 0.0))
        assert got.ok, got
        assert np.allclose(got.T, T, atol=1e-6, rtol=0), (got.T, T)


def test_all_invalid_scan_and_far_guess_fail_with_no_correspondences():
    scan = orc.room_scan((0.0, 0.0, 0.0), walls=rc.ROOM_BENCH)
    bad = np.full(360, np.nan, dtype=np.float32)
    r = R.match(scan, bad, L, (0.0, 0.0, 0.0))
    assert not r.ok and r.criterion == R.NO_CORRESPONDENCES and r.iterations == 1 and r.T == (0.0, 0.0, 0.0)
    r = R.match(bad, scan, L, (0.0, 0.0, 0.0))
    assert not r.ok and r.criterion == R.NO_CORRESPONDENCES
    small = orc.room_scan((0.0, 0.0, 0.0), walls=(-0.6, 0.6, -0.6, 0.6))
    r = R.match(small, small, L, (0.0, 2.0, 0.0))   # 2 m off: no pair within 0.5 m
    assert not r.ok and r.criterion == R.NO_CORRESPONDENCES


def test_max_iter_one_stops_with_iterations():
    a = orc.room_scan((0.0, 0.0, 0.0), walls=rc.ROOM_BENCH)
    b = orc.room_scan((0.05, 0.07, 0.02), walls=rc.ROOM_BENCH)
    r = R.match(a, b, L, (0.0, 0.0, 0.0), max_iter=1)
    assert r.ok and r.criterion == R.ITERATIONS and r.iterations == 1


def test_wrapper_bookkeeping():
    a = orc.room_scan((0.0, 0.0, 0.0), walls=rc.ROOM_BENCH)
    b = orc.room_scan((0.02, 0.05, 0.0), walls=rc.ROOM_BENCH)
    bad = np.full(360, np.inf, dtype=np.float32)
    w = R.Wrapper(L)
    first = w.step(a, (0.3, 0.3, 0.3))
    assert first.ok and first.T == (0.0, 0.0, 0.0) and first.criterion == R.NOT_RUN
    assert np.array_equal(w.stored, a)
    f = w.step(bad, (0.0, 0.0, 0.0))
    assert not f.ok and np.array_equal(w.stored, a)        # a failure keeps the stored scan
    g = w.step(b, (0.0, 0.0, 0.0))
    assert g.ok and np.array_equal(w.stored, b)            # a success replaces it
    assert g.T == R.match(a, b, L, (0.0, 0.0, 0.0)).T


def test_summation_order_is_a_parameter():
    """B changes only the last bits (the order of the fp64 sums), never the outcome on a room."""
    a = orc.room_scan((0.0, 0.0, 0.0), walls=rc.ROOM_BENCH, rng=np.random.default_rng(2))
    b = orc.room_scan((0.05, 0.06, 0.01), walls=rc.ROOM_BENCH, rng=np.random.default_rng(3))
    r1, r2 = R.match(a, b, L, (0.0, 0.0, 0.0), B=256), R.match(a, b, L, (0.0, 0.0, 0.0), B=64)
    assert r1.ok and r2.ok
    assert np.allclose(r1.T, r2.T, atol=1e-9)


def test_rooms_with_the_icp_init_guess_land_within_2cm_and_5mrad():
    for room, inc in ((rc.ROOM_BENCH, rc.TRAJ_BENCH), (rc.ROOM_SURVEY, rc.TRAJ_SURVEY)):
        steps, poses = rc.trajectory(8, inc=inc)
        rng = np.random.default_rng(1)
        scans = [orc.room_scan(p, walls=room, rng=rng) for p in poses]
        for s in range(1, 8):
            prev, cur = poses[s - 1], poses[s]
            r = R.match(scans[s - 1], scans[s], L, R.init_guess(cur, prev))
            truth = rc.compose(rc.inverse(prev), cur)
            assert r.ok and r.correspondences >= 250, (room, s, r)
            err = np.array(r.T) - truth
            assert abs(err[0]) < 0.005 and np.hypot(err[1], err[2]) < 0.02, (room, s, err)


def test_init_guess_is_the_world_frame_difference():
    g = R.init_guess((3.0, 1.0, 2.0), (-3.0, 0.5, 1.0))
    assert g[1] == 0.5 and g[2] == 1.0
    assert abs(g[0] - (6.0 - 2 * math.pi)) < 1e-12   # normalize(normalize(3) - normalize(-3))
