"""The numpy restatement of the device ICP's point-to-line metric (tests/icp_line_restatement.py, include/tbnav_icp.h
POINT-TO-LINE METRIC) on its own (CPU): what the metric is for, held as tests — it needs fewer iterations than the point
metric and lands closer on the project's rooms, it leaves the direction a corridor hides at the guess where the point metric
erases the motion, it refuses (DEGENERATE) where the scan holds no information at all — and the normals' rules.  The metric has
no counterpart in the reference; the GPU tests hold the kernel to this restatement bit for bit.

Measured with this restatement (360 beams, the 14 pairs below): bench room 3.57 iterations on average (point metric 9.0),
translation error mean 1.27 / max 3.32 mm (10.05 / 10.76), rotation error max 0.90 mrad; survey room 3.71 (8.29), 1.26 /
2.88 mm (4.65 / 6.77), 1.50 mrad; at least 260 pairs."""
import math

import numpy as np

import icp_line_restatement as LR
import icp_restatement as R
import oracle_api as orc
import rbpf_cases as rc

L = R.lds01()
CORRIDOR = (-50, 50, -1, 1)


def _apply(T, pts):
    c, s = math.cos(T[0]), math.sin(T[0])
    return np.stack([c * pts[:, 0] - s * pts[:, 1] + T[1], s * pts[:, 0] + c * pts[:, 1] + T[2]], axis=1)


def test_noise_free_room_motion_is_recovered_in_fewer_iterations_than_the_point_metric():
    p0, p1 = (0.1, 0.2, -0.1), (0.15, 0.27, -0.06)
    a = orc.room_scan(p0, walls=rc.ROOM_SURVEY)
    b = orc.room_scan(p1, walls=rc.ROOM_SURVEY)
    truth = np.array(rc.compose(rc.inverse(p0), p1))
    line, point = LR.match(a, b, L, (0.0, 0.0, 0.0)), R.match(a, b, L, (0.0, 0.0, 0.0))
    err = np.abs(np.array(line.T) - truth)
    print("line", line, err, "point", point)
    assert line.ok and point.ok
    assert np.all(err < 1e-5), err
    assert line.iterations <= point.iterations, (line.iterations, point.iterations)


def test_noise_free_rigid_motion_of_a_curve_is_recovered():
    """test_icp_restatement's star-shaped closed curve (target = T * source exactly), through match_clouds, to 1e-6."""
    ang = np.arange(0, 2 * np.pi, np.pi / 90)
    rad = 1.5 + 0.5 * np.cos(3 * ang)
    src = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1).astype(np.float32)
    beams = np.arange(len(src))
    for T in ((0.03, 0.02, -0.015), (-0.05, -0.04, 0.03)):
        tgt = _apply(T, src.astype(np.float64)).astype(np.float32)
        got = LR.match_clouds(tgt, beams, src, beams, len(src), (0.0, 0.0, 0.0))
        print(T, got)
        assert got.ok, got
        assert np.allclose(got.T, T, atol=1e-6, rtol=0), (got.T, T)


def test_rooms_land_closer_and_sooner_than_the_point_metric():
    """The 14 pairs of test_rooms_with_the_icp_init_guess_land_within_2cm_and_5mrad."""
    for room, inc in ((rc.ROOM_BENCH, rc.TRAJ_BENCH), (rc.ROOM_SURVEY, rc.TRAJ_SURVEY)):
        steps, poses = rc.trajectory(8, inc=inc)
        rng = np.random.default_rng(1)
        scans = [orc.room_scan(p, walls=room, rng=rng) for p in poses]
        terr = {"line": [], "point": []}
        iters = {"line": 0, "point": 0}
        for s in range(1, 8):
            prev, cur = poses[s - 1], poses[s]
            g = R.init_guess(cur, prev)
            truth = np.array(rc.compose(rc.inverse(prev), cur))
            line = LR.match(scans[s - 1], scans[s], L, g)
            point = R.match(scans[s - 1], scans[s], L, g)
            assert line.ok and line.correspondences >= 240, (room, s, line)
            assert point.ok
            err = np.array(line.T) - truth
            perr = np.array(point.T) - truth
            print(room, s, "line", line.iterations, line.correspondences, err, "point", point.iterations, perr)
            assert abs(err[0]) < 0.003 and np.hypot(err[1], err[2]) < 0.005, (room, s, err)
            terr["line"].append(np.hypot(err[1], err[2]))
            terr["point"].append(np.hypot(perr[1], perr[2]))
            iters["line"] += line.iterations
            iters["point"] += point.iterations
        print(room, "mean translation error", np.mean(terr["line"]), np.mean(terr["point"]), "iterations", iters)
        assert np.mean(terr["line"]) <= 0.5 * np.mean(terr["point"]), (room, terr)
        assert iters["line"] <= 0.6 * iters["point"], (room, iters)


def _corridor(rng):
    a = orc.room_scan((0.0, 0.0, 0.0), walls=CORRIDOR, rng=rng)
    b = orc.room_scan((0.0, 0.05, 0.0), walls=CORRIDOR, rng=rng)   # 5 cm along the corridor
    return a, b


def test_noisy_corridor_keeps_the_guess_along_it_where_the_point_metric_erases_the_motion():
    a, b = _corridor(np.random.default_rng(2))
    guess = (0.0, 0.05, 0.0)
    line, point = LR.match(a, b, L, guess), R.match(a, b, L, guess)
    print("line", line, "point", point)
    assert line.ok and point.ok
    assert abs(line.T[1] - guess[1]) < 0.005, line
    assert abs(point.T[1] - guess[1]) > 0.030, point


def test_noise_free_corridor_is_degenerate():
    a, b = _corridor(None)
    r = LR.match(a, b, L, (0.0, 0.05, 0.0))
    assert not r.ok and r.criterion == R.DEGENERATE and r.T == (0.0, 0.0, 0.0), r


def test_depth_jump_wider_than_the_gap_gives_one_sided_normals():
    """A wall at x = 1 up to beam 19 and at x = 2 from beam 20 (beams 340..359 and 0..39 only): no normal is drawn across
    the 1 m jump, the beams on either side of it take their one neighbour on their own side."""
    n = 360
    ang = np.deg2rad(np.arange(n, dtype=np.float64))
    scan = np.full(n, np.inf, dtype=np.float32)
    near, far = np.arange(0, 20), np.arange(20, 40)
    scan[near] = (1.0 / np.cos(ang[near])).astype(np.float32)
    scan[far] = (2.0 / np.cos(ang[far])).astype(np.float32)
    nxy, has = LR.normals(scan, L)
    assert has[:40].all() and not has[40:].any()
    pts, beam = R.cloud(scan, L)
    for i, lo, hi in ((19, 18, 19), (20, 20, 21), (0, 0, 1), (39, 38, 39), (10, 9, 11)):   # 0 and 39: the window's ends
        t = pts[hi].astype(np.float64) - pts[lo].astype(np.float64)
        l = math.sqrt(t[0] * t[0] + t[1] * t[1])
        assert tuple(nxy[i]) == (np.float32(-t[1] / l), np.float32(t[0] / l)), i
    assert np.allclose(np.abs(nxy[:40, 0]), 1.0, atol=1e-3)   # walls x = const: normals along x
    # with a gap that spans the jump the two sides are joined
    wide, _ = LR.normals(scan, L, max_gap=1.5)
    assert abs(wide[19, 0]) < 0.9 and abs(wide[20, 0]) < 0.9


def test_a_point_without_a_neighbour_has_no_normal_and_is_never_paired():
    a = orc.room_scan((0.0, 0.0, 0.0), walls=rc.ROOM_BENCH, rng=np.random.default_rng(4))
    b = orc.room_scan((0.01, 0.03, 0.01), walls=rc.ROOM_BENCH, rng=np.random.default_rng(5))
    lone = a.copy()
    lone[[99, 101]] = np.nan                 # beam 100 has no valid neighbour inside window 1
    lone[200] = np.float32(0.5)              # beam 200 stands 1.5 m in front of its wall: its neighbours are beyond the gap
    nxy, has = LR.normals(lone, L)
    assert not has[100] and not has[200] and not has[99] and has[98] and has[102]
    assert has[199] and has[201]             # one-sided
    assert tuple(nxy[100]) == (0.0, 0.0)
    full = LR.match(a, b, L, (0.0, 0.0, 0.0))
    r = LR.match(lone, b, L, (0.0, 0.0, 0.0))
    assert full.ok and r.ok
    # the sources whose nearest target is beam 100 or 200 are dropped, not handed to the next nearest target
    assert r.correspondences < 360 and full.correspondences == 360, (r, full)
    # a target of lone points only: every point is valid, none has a normal, nothing is paired
    sparse = np.full(360, np.nan, dtype=np.float32)
    sparse[::4] = a[::4]
    assert not LR.normals(sparse, L)[1].any()
    r = LR.match(sparse, b, L, (0.0, 0.0, 0.0))
    assert not r.ok and r.criterion == R.NO_CORRESPONDENCES and r.correspondences == 0 and r.iterations == 1


def test_invalid_beams_inside_the_window_are_skipped():
    a = orc.room_scan((0.0, 0.0, 0.0), walls=rc.ROOM_BENCH, rng=np.random.default_rng(4))
    holes = a.copy()
    holes[[99, 101, 102]] = [np.nan, np.inf, np.float32(0.05)]      # NaN, inf, below range_min
    pts, beam = R.cloud(holes, L)
    at = {int(b): k for k, b in enumerate(beam)}
    nxy, has = LR.normals(holes, L, window=3)
    assert has[100]
    t = pts[at[103]].astype(np.float64) - pts[at[97]].astype(np.float64)   # lowest / highest valid beam inside window 3
    l = math.sqrt(t[0] * t[0] + t[1] * t[1])
    assert tuple(nxy[100]) == (np.float32(-t[1] / l), np.float32(t[0] / l))
    assert not LR.normals(holes, L, window=1)[1][100]


def test_window_1_against_window_9_on_1080_beams():
    """At 1/3 degree the 1 cm range noise tilts a window-1 tangent (two points 1-2 cm apart) by tens of degrees; window 9
    spans ten times the baseline.  Both align; the wide window's normals are the straighter ones."""
    L3 = R.lds01(1.0 / 3.0)
    rng = np.random.default_rng(7)
    p0, p1 = (0.0, 0.0, 0.0), (0.02, 0.05, 0.01)
    a = orc.room_scan(p0, n_beams=1080, beam_delta_deg=1.0 / 3.0, walls=rc.ROOM_BENCH, rng=rng)
    b = orc.room_scan(p1, n_beams=1080, beam_delta_deg=1.0 / 3.0, walls=rc.ROOM_BENCH, rng=rng)
    n1, h1 = LR.normals(a, L3, window=1)
    n9, h9 = LR.normals(a, L3, window=9)
    assert h1.all() and h9.all()
    assert not np.array_equal(n1, n9)
    # a wall's normal is an axis: the smaller component is the tilt
    tilt1 = np.minimum(np.abs(n1[:, 0]), np.abs(n1[:, 1]))
    tilt9 = np.minimum(np.abs(n9[:, 0]), np.abs(n9[:, 1]))
    print("median tilt", np.median(tilt1), np.median(tilt9))
    assert np.median(tilt9) < 0.5 * np.median(tilt1)
    truth = np.array(rc.compose(rc.inverse(p0), p1))
    for w in (1, 9):
        r = LR.match(a, b, L3, R.init_guess(p1, p0), window=w)
        err = np.array(r.T) - truth
        print(w, r, err)
        assert r.ok and abs(err[0]) < 0.003 and np.hypot(err[1], err[2]) < 0.005, (w, r, err)


def test_wrapper_keeps_the_stored_scan_on_a_degenerate_scan():
    a, b = _corridor(None)
    w = LR.Wrapper(L)
    first = w.step(a, (0.3, 0.3, 0.3))
    assert first.ok and first.T == (0.0, 0.0, 0.0) and first.criterion == R.NOT_RUN
    f = w.step(b, (0.0, 0.05, 0.0))
    assert not f.ok and f.criterion == R.DEGENERATE and np.array_equal(w.stored, a)
    # a noise-free corridor as the target is degenerate whatever the source: the point metric takes over (set_metric between
    # steps keeps the stored scan) and aligns against a, the scan that was kept
    w.metric = "point"
    g = w.step(b, (0.0, 0.05, 0.0))
    assert g.ok and np.array_equal(w.stored, b)
    assert g.T == R.match(a, b, L, (0.0, 0.05, 0.0)).T
    w.metric = "line"
    noisy = orc.room_scan((0.0, 0.1, 0.0), walls=CORRIDOR, rng=np.random.default_rng(2))
    h = w.step(noisy, (0.0, 0.05, 0.0))
    assert not h.ok and h.criterion == R.DEGENERATE and np.array_equal(w.stored, b)
