"""The device ICP's correlative search (include/tbnav_icp.h CORRELATIVE SEARCH, csrc/icp_search.hip) against the numpy restatement
of that contract (tests/icp_search_restatement.py) with ==: the table, the whole score volume, the chosen indices, T, score,
quality, candidates, at_edge and accepted; then the search in front of the ICP (match / step / step_batch, both metrics) against
the restated search feeding the restated ICP, bit for bit; that off means off; the argument limits; and the Python and C++
layers.  Scores are integers: there is no tolerance anywhere."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import icp_line_restatement as LR
import icp_restatement as R
import icp_search_restatement as S
import oracle_api as orc
import rbpf_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "libtbnav_host.so")
FIELDS = ("resolution", "half_extent", "sigma", "ang_step", "min_quality", "stamp_cells", "lin_cells", "ang_steps", "slack_q10")
NEAR_ROOM = (-0.9, 0.8, -0.7, 1.4)    # walls on both sides of a +-1 m table's edge

pytestmark = pytest.mark.gpu


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _laser(params):
    return R.Laser(params.beam_min, params.beam_max, params.beam_delta, params.range_min, params.range_max)


def _aligner(gpu_pkg, search=None, metric="point", **kw):
    from rtn_amd import icp
    p = icp.default_params(**kw)
    return icp.ScanAlignment(p, metric=metric, search=search), p


def _kw(p: S.Params):
    return {f: getattr(p, f) for f in FIELDS}


def _same_info(got: dict, want: S.Info, where=""):
    for f in ("T", "quality", "score", "points", "candidates", "ia", "iy", "ix", "at_edge", "accepted", "searched"):
        assert got[f] == getattr(want, f), (where, f, got, want)


def _same(got, want: R.Result, where=""):
    ok, T, info = got
    assert ok == want.ok, (where, got, want)
    assert (info["iterations"], info["criterion"], info["correspondences"]) == (want.iterations, want.criterion, want.correspondences), (where, info, want)
    assert info["mse"] == want.mse, (where, info["mse"], want.mse)
    assert tuple(T) == tuple(want.T), (where, T, want.T)


def _pair(room, n_beams=360, seed=1, p1=(0.07, 0.02, 0.01)):
    rng = np.random.default_rng(seed)
    dd = 360.0 / n_beams if n_beams > 1 else 1.0
    s0 = orc.room_scan((0.0, 0.0, 0.0), n_beams=n_beams, beam_delta_deg=dd, walls=room, rng=rng)
    s1 = orc.room_scan(p1, n_beams=n_beams, beam_delta_deg=dd, walls=room, rng=rng)
    return s0, s1, dd, R.init_guess(p1, (0.0, 0.0, 0.0))


def test_tables_are_the_restatements(gpu_pkg):
    rng = np.random.default_rng(5)
    scan = orc.room_scan((0.3, 0.1, -0.2), walls=rc.ROOM_SURVEY, rng=rng)
    scan[[0, 7, 100, 101]] = [np.nan, np.inf, -np.inf, np.float32(0.05)]
    scan[50] = np.float32(0.12)    # range_min: kept, a point 12 cm from the laser
    scan[359] = np.float32(3.5)    # range_max: out
    near = orc.room_scan((0.1, 0.05, 0.0), walls=NEAR_ROOM, rng=rng)
    params = [S.Params(), S.Params(lin_cells=16, ang_steps=0), S.Params(half_extent=1.0), S.Params(resolution=0.04, half_extent=3.0),
              S.Params(stamp_cells=8, sigma=0.2), S.Params(stamp_cells=1, sigma=0.02, lin_cells=0)]
    for kw in (dict(), dict(Trs=(0.4, -0.07, 0.05))):
        for sc in (scan, near):
            for sp in params:
                a, p = _aligner(gpu_pkg, search=_kw(sp), **kw)
                got = a.searchTable(sc)
                want = S.table(sc, _laser(p), sp, tuple(p.Trs))
                assert got.shape == want.shape and np.array_equal(got, want), (kw, sp)
                assert want.any()
                a.close()
    # with the search off the hook builds the default table
    a, p = _aligner(gpu_pkg)
    assert np.array_equal(a.searchTable(scan), S.table(scan, _laser(p)))
    a.close()


def _three(s1):
    three = np.full(s1.size, np.nan, dtype=np.float32)
    three[[10, 130, 250]] = s1[[10, 130, 250]]
    return three


# (name, room, n_beams, search parameters, offset of the guess from the truth, Trs, what to do with the source)
VOLUMES = [
    ("bench", rc.ROOM_BENCH, 360, S.Params(), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), None),
    ("survey", rc.ROOM_SURVEY, 360, S.Params(), (0.05, 0.1, -0.15), (0.0, 0.0, 0.0), None),
    ("window 0 0", rc.ROOM_BENCH, 360, S.Params(lin_cells=0, ang_steps=0), (0.0, 0.02, 0.0), (0.0, 0.0, 0.0), None),
    ("window 14 20", rc.ROOM_BENCH, 360, S.Params(lin_cells=14), (0.0, 0.65, 0.65), (0.0, 0.0, 0.0), None),
    ("window 14 20 survey", rc.ROOM_SURVEY, 360, S.Params(lin_cells=14), (0.0, 0.65, 0.65), (0.0, 0.0, 0.0), None),
    ("window 8 2", rc.ROOM_BENCH, 360, S.Params(lin_cells=8, ang_steps=2), (0.0, -0.2, 0.1), (0.0, 0.0, 0.0), None),
    ("window 16 90, the largest table", rc.ROOM_BENCH, 360, S.Params(lin_cells=16, ang_steps=90, half_extent=4.375), (1.2, -0.5, 0.3), (0.0, 0.0, 0.0), None),
    ("window 13 3", rc.ROOM_SURVEY, 360, S.Params(lin_cells=13, ang_steps=3), (0.0, 0.3, 0.0), (0.0, 0.0, 0.0), None),
    ("1 beam", rc.ROOM_BENCH, 1, S.Params(ang_steps=2), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), None),
    ("255 beams", rc.ROOM_BENCH, 255, S.Params(), (0.02, 0.1, 0.0), (0.0, 0.0, 0.0), None),
    ("257 beams", rc.ROOM_SURVEY, 257, S.Params(), (0.0, 0.0, 0.1), (0.0, 0.0, 0.0), None),
    ("1080 beams", rc.ROOM_BENCH, 1080, S.Params(), (0.1, 0.1, 0.1), (0.1, -0.05, 0.02), None),
    ("4096 beams", rc.ROOM_BENCH, 4096, S.Params(ang_steps=5), (0.0, 0.05, 0.0), (0.0, 0.0, 0.0), None),
    ("half_extent 1", NEAR_ROOM, 360, S.Params(half_extent=1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), None),
    ("half_extent 1, window 16: base cells outside the table", NEAR_ROOM, 360, S.Params(half_extent=1.0, lin_cells=16, ang_steps=4),
     (0.3, 0.4, -0.5), (0.2, 0.1, -0.1), None),
    ("half_extent 1 in a room outside it", rc.ROOM_BENCH, 360, S.Params(half_extent=1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), None),
    ("resolution 0.04", rc.ROOM_BENCH, 360, S.Params(resolution=0.04, half_extent=3.0, sigma=0.04), (0.0, 0.1, -0.1), (0.0, 0.0, 0.0), None),
    ("stamp 8", rc.ROOM_SURVEY, 360, S.Params(stamp_cells=8, sigma=0.2), (0.0, 0.2, 0.2), (0.0, 0.0, 0.0), None),
    ("three beams tie", rc.ROOM_BENCH, 360, S.Params(), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), _three),
    ("slack 64", rc.ROOM_BENCH, 360, S.Params(slack_q10=64), (0.05, 0.1, 0.1), (0.0, 0.0, 0.0), None),
    ("slack 1023, three beams", rc.ROOM_BENCH, 360, S.Params(slack_q10=1023), (0.0, 0.1, 0.0), (0.0, 0.0, 0.0), _three),
    ("invalid beams", rc.ROOM_SURVEY, 360, S.Params(), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0),
     lambda s: np.where(np.arange(s.size) % 7 == 0, np.float32(np.nan), s).astype(np.float32)),
]


@pytest.mark.parametrize("case", VOLUMES, ids=[c[0] for c in VOLUMES])
def test_score_volume_and_result_are_the_restatements(gpu_pkg, case):
    name, room, n_beams, sp, off, Trs, edit = case
    s0, s1, dd, truth = _pair(room, n_beams)
    if edit is not None:
        s1 = edit(s1)
    guess = tuple(t + o for t, o in zip(truth, off))
    a, p = _aligner(gpu_pkg, search=_kw(sp), beam_delta_deg=dd, Trs=Trs)
    L = _laser(p)
    want_sc = S.scores(s0, s1, L, guess, sp, Trs)
    want = S.search(s0, s1, L, guess, sp, Trs, scores=want_sc)
    acc, T, info, sc = a.searchScores(guess, s0, s1)
    assert sc.shape == want_sc.shape and np.array_equal(sc, want_sc), name
    _same_info(info, want, name)
    assert acc == bool(want.accepted) and T == want.T
    acc2, T2, info2 = a.search(guess, s0, s1)                 # the entry without the volume, and a repeat: the same bits
    assert (acc2, T2, info2) == (acc, T, info)
    if name == "three beams tie":
        assert info["score"] == 765 and info["candidates"] == 3
    if "outside the table" in name:
        assert 0 < info["score"]
    a.close()


def test_the_stateless_entry_uses_the_defaults_while_the_search_is_off(gpu_pkg):
    s0, s1, dd, truth = _pair(rc.ROOM_BENCH)
    a, p = _aligner(gpu_pkg)
    assert a.searchParams() == (False, _kw(S.Params()))
    acc, T, info = a.search(truth, s0, s1)
    _same_info(info, S.search(s0, s1, _laser(p), truth))
    assert acc and a.lastSearch()["searched"] == 0           # the stateless entry leaves the pipeline's record alone
    a.close()


PIPE = S.Params(lin_cells=14)
SLIPPED = 2


def _batch_run():
    from rtn_amd import icp
    n = 12
    steps, poses = rc.trajectory(n, inc=rc.TRAJ_BENCH)
    rng = np.random.default_rng(17)
    scans = np.stack([orc.room_scan(q, walls=rc.ROOM_BENCH, rng=rng) for q in poses])
    scans[5] = np.float32(np.inf)                             # fails: the pairs behind it are aligned again
    T_init = np.array([icp.init_guess(poses[s], poses[s - 1] if s else poses[0]) for s in range(n)])
    T_init[SLIPPED, 1:] += 0.65                               # a slip: outside the basin of either metric, inside the window
    return scans, T_init, poses


_searches = {}


def _want_steps(scans, T_init, L, icp_fn):
    """the restated search feeding the restated ICP, with pclICPWrapper's bookkeeping; the searches are shared by the metrics"""
    stored, out = None, []
    for s in range(len(scans)):
        if stored is None:
            stored = s
            out.append((R.Result(True, (0.0, 0.0, 0.0), 0, 0, 0.0, R.NOT_RUN), None))
            continue
        key = (stored, s)
        if key not in _searches:
            _searches[key] = S.search(scans[stored], scans[s], L, tuple(T_init[s]), PIPE)
        res, info = S.match(scans[stored], scans[s], L, tuple(T_init[s]), PIPE, icp=icp_fn, info=_searches[key])
        out.append((res, info))
        if res.ok:
            stored = s
    return out


@pytest.mark.parametrize("metric,icp_fn", [("point", R.match), ("line", LR.match)])
def test_match_step_and_batch_are_the_restated_search_feeding_the_restated_icp(gpu_pkg, metric, icp_fn):
    scans, T_init, poses = _batch_run()
    n = len(scans)
    a, p = _aligner(gpu_pkg, search=_kw(PIPE), metric=metric)
    L = _laser(p)
    want = _want_steps(scans, T_init, L, icp_fn)
    one, rec = [], []
    for s in range(n):
        one.append(a.pclICPWrapper(T_init[s], scans[s]))
        rec.append(a.lastSearch())
    for s in range(n):
        _same(one[s], want[s][0], (metric, s))
        if want[s][1] is None:
            assert rec[s]["searched"] == 0 and rec[s]["T"] == (0.0, 0.0, 0.0)
        else:
            _same_info(rec[s], want[s][1], (metric, s))
    assert [s for s in range(n) if not one[s][0]] == [5]
    q = SLIPPED
    assert rec[q]["accepted"] == 1 and rec[5]["accepted"] == 0
    truth = R.init_guess(poses[q], poses[q - 1])
    assert math.hypot(one[q][1][1] - truth[1], one[q][1][2] - truth[2]) < 0.02
    # the stateless match: the slipped scan against the one before it, found
    m = a.pclICP(T_init[q], scans[q - 1], scans[q])
    _same(m, want[q][0], metric)
    _same_info(a.lastSearch(), want[q][1], metric)
    # the batch: 12 steps, bit for bit, the realignment launches included
    b, _ = _aligner(gpu_pkg, search=_kw(PIPE), metric=metric)
    ok, T, info = b.wrapperBatch(T_init, scans)
    assert b.lastBatchLaunches() > 1
    for s in range(n):
        assert bool(ok[s]) == one[s][0] and tuple(T[s]) == one[s][1] and info[s] == one[s][2], (metric, s)
    assert b.lastSearch() == rec[n - 1]
    # and the rest of a run after a batch goes on from the batch's stored scan
    assert b.pclICPWrapper(T_init[3], scans[3]) == a.pclICPWrapper(T_init[3], scans[3])
    a.setSearch(None)
    off = a.pclICP(T_init[q], scans[q - 1], scans[q])
    assert off[0] and math.hypot(off[1][1] - truth[1], off[1][2] - truth[2]) > 0.5     # the parent's answer: converged, wrong
    a.close(); b.close()


@pytest.mark.parametrize("room,inc", [(rc.ROOM_BENCH, rc.TRAJ_BENCH), (rc.ROOM_SURVEY, rc.TRAJ_SURVEY)])
def test_off_means_off(gpu_pkg, room, inc):
    """the room cases of test_icp_gpu.test_match_is_the_restatement_bit_for_bit: a fresh handle, a handle whose search was
    turned off again, and a handle whose search is on but not accepted all give the parent's contract (icp_restatement.match)"""
    from rtn_amd import icp
    fresh, p = _aligner(gpu_pkg)
    was_on, _ = _aligner(gpu_pkg, search=True)
    on, _ = _aligner(gpu_pkg, search=True)
    L = _laser(p)
    steps, poses = rc.trajectory(6, inc=inc)
    rng = np.random.default_rng(11)
    scans = np.stack([orc.room_scan(q, walls=room, rng=rng) for q in poses])
    was_on.pclICP((0.0, 0.0, 0.0), scans[0], scans[1])
    assert was_on.lastSearch()["searched"] == 1
    was_on.setSearch(None)
    assert was_on.searchParams() == (False, _kw(S.Params()))
    for s in range(1, 6):
        g = icp.init_guess(poses[s], poses[s - 1])
        for guess in (g, (g[0] + math.radians(3.0), g[1] + 0.05, g[2] - 0.05)):
            want = R.match(scans[s - 1], scans[s], L, guess)
            _same(fresh.pclICP(guess, scans[s - 1], scans[s]), want, (room, s, guess))
            _same(was_on.pclICP(guess, scans[s - 1], scans[s]), want, (room, s, guess))
            assert was_on.lastSearch()["searched"] == 0 and fresh.lastSearch()["searched"] == 0
        far = (g[0], g[1] + 0.65, g[2] + 0.65)               # the default window does not reach the truth: not accepted
        got = on.pclICP(far, scans[s - 1], scans[s])
        rec = on.lastSearch()
        assert rec["searched"] == 1 and rec["accepted"] == 0
        assert got == fresh.pclICP(far, scans[s - 1], scans[s])
        _same(got, R.match(scans[s - 1], scans[s], L, far), (room, s, "far"))
    fresh.close(); was_on.close(); on.close()


def test_set_search_checks_its_arguments_and_get_search_returns_them(gpu_pkg):
    capi = gpu_pkg.capi
    Lib = capi.lib()
    a, p = _aligner(gpu_pkg, search=dict(lin_cells=4, slack_q10=7))
    held = (True, _kw(S.Params(lin_cells=4, slack_q10=7)))
    assert a.searchParams() == held
    bad = [dict(stamp_cells=0), dict(stamp_cells=9), dict(lin_cells=-1), dict(lin_cells=17), dict(ang_steps=-1), dict(ang_steps=91),
           dict(slack_q10=-1), dict(slack_q10=1024), dict(resolution=0.0), dict(resolution=-0.05), dict(resolution=float("nan")),
           dict(half_extent=0.0), dict(half_extent=float("inf")), dict(sigma=0.0), dict(sigma=float("nan")), dict(ang_step=float("inf")),
           dict(min_quality=float("nan")), dict(resolution=0.04), dict(half_extent=4.45, lin_cells=16), dict(half_extent=6.0),
           dict(resolution=1e-9)]
    for kw in bad:
        assert not S.valid(S.Params(**kw)), kw
        sp = capi.IcpSearchParams()
        Lib.tbnav_icp_default_search_params(C.byref(sp))
        for f, v in kw.items():
            setattr(sp, f, v)
        assert Lib.tbnav_icp_set_search(a._h, C.byref(sp)) == capi.ERR_INVALID_ARG, kw
        assert a.searchParams() == held, kw                   # a refused call changes nothing
        with pytest.raises(capi.TbnavError):
            a.setSearch(**kw)
    assert Lib.tbnav_icp_set_search(None, None) == capi.ERR_INVALID_ARG
    for kw in (dict(lin_cells=16, ang_steps=90, stamp_cells=8, slack_q10=1023), dict(resolution=0.04, half_extent=3.0),
               dict(half_extent=4.375, lin_cells=16), dict(lin_cells=0, ang_steps=0, stamp_cells=1)):
        assert S.valid(S.Params(**kw)), kw
        a.setSearch(**kw)
        assert a.searchParams() == (True, _kw(S.Params(**kw)))
    with pytest.raises(TypeError):
        a.setSearch(window=3)
    a.setSearch(None)
    assert a.searchParams() == (False, _kw(S.Params()))
    wide = np.full(4097, 1.0, dtype=np.float32)                # TBNAV_ICP_MAX_BEAMS + 1
    with pytest.raises(capi.TbnavError):
        a.search((0, 0, 0), wide, wide)
    with pytest.raises(capi.TbnavError):
        a.searchTable(wide)
    a.close()


@pytest.fixture(scope="module")
def host(pkg):
    pkg.capi.lib()
    Lib = C.CDLL(HOST_LIB)
    Lib.hst_icp_last_error.restype = C.c_char_p
    Lib.hst_icp_pf_run_search.restype = C.c_int
    Lib.hst_icp_pf_run_search.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_uint64] + [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
    return Lib


SLIP = 3


def _slipped_run():
    """six scans of a drive through ROOM_SMALL; at scan SLIP the odometry jumps 0.65 m in x and y that the robot did not move (a
    wheel slip), and stays off by that from then on.  The map is +-4 m: in the shipped +-2 m map the wrong pose of the parent's
    pipeline leaves the map and the filter throws instead of answering."""
    n = 6
    steps, poses = rc.trajectory(n, inc=(0.04, 0.03, 0.02))
    rng = np.random.default_rng(3)
    scans = np.stack([orc.room_scan(poses[s], walls=rc.ROOM_SMALL, rng=rng) for s in range(n)])
    odom = np.stack([steps[0][0]] + [st[1] for st in steps]).astype(np.float64)
    odom[SLIP + 1:, 1:] += 0.65
    u = np.array([st[3] for st in steps], dtype=np.float64)
    return scans, odom, u, np.array(poses)


def test_particle_filter_class_with_the_search(host, gpu_pkg):
    """bmapping::ScanAlignment::useDeviceICP(-1, metric, ICPSearch) inside bmapping::ParticleFilter: the (ok, T) the class's
    matcher returns per scan equals the Python mirror's and the restatement's; after a slipped scan the filter's pose stays
    within 5 cm of the truth, where the parent's pipeline (the same run, the search off) is more than 0.5 m away."""
    from rtn_amd import icp
    N, k = 40, 50
    scans, odom, u, poses = _slipped_run()
    n = len(scans)

    def run(search):
        ok = np.zeros(n, dtype=np.int32); T = np.zeros((n, 3)); pose = np.zeros((n, 3)); neff = np.zeros(n, dtype=np.int32)
        rcode = host.hst_icp_pf_run_search(0, search, 14, N, k, 4.0, 11, _p(scans), 360, n, _p(odom), _p(u), _p(ok), _p(T), _p(pose), _p(neff))
        assert rcode == 0, host.hst_icp_last_error()
        return ok, T, pose

    ok, T, pose = run(1)
    mirror, p = _aligner(gpu_pkg, search=_kw(PIPE))
    L = _laser(p)
    stored = None
    for s in range(n):
        g = icp.init_guess(odom[s + 1], odom[s])
        m = mirror.pclICPWrapper(g, scans[s])
        assert bool(ok[s]) == m[0] and tuple(T[s]) == m[1], s
        if stored is not None:
            want, info = S.match(scans[stored], scans[s], L, g, PIPE)
            assert m[0] == want.ok and m[1] == tuple(want.T), s
            _same_info(mirror.lastSearch(), info, s)
        if m[0]:
            stored = s
    assert mirror.lastSearch()["searched"] == 1
    mirror.close()
    assert ok.all()

    def err(pose):
        # the filter starts one odometry increment behind the first scan's pose (rbpf_cases.trajectory) and the first
        # alignment is the identity, so its frame is shifted by that increment: what is compared is the way travelled
        # since scan 0
        d = (pose[SLIP] - pose[0]) - (poses[SLIP] - poses[0])
        return math.hypot(d[1], d[2])

    d_on = err(pose)
    ok0, T0, pose0 = run(0)
    d_off = err(pose0)
    print("filter pose error at the slipped scan: search on %.4f m, off %.4f m" % (d_on, d_off))
    assert d_on < 0.05, d_on
    assert ok0[SLIP] and d_off > 0.5, d_off
