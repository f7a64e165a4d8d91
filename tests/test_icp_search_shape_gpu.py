"""The shape of the correlative search's score volume on the device (include/tbnav_icp.h, items F1-F6; csrc/icp_search_shape.hip)
against its restatement (tests/icp_search_shape_restatement.py) with ==: the seven integers, kind, cells, and the doubles the
host forms from them with the same arithmetic (l1, l2, e, the shaped T).  Then the search with the shape in front of the ICP
(match / step / step_batch, both metrics) against the restated search -> shape -> ICP chain, bit for bit; that off means off;
the argument limits; and the C++ class inside bmapping::ParticleFilter on a corridor.  There is no tolerance anywhere."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import icp_line_restatement as LR
import icp_restatement as R
import icp_search_restatement as S
import icp_search_shape_restatement as F
import oracle_api as orc
import rbpf_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "lib", "libtbnav_host.so")
FIELDS = ("resolution", "half_extent", "sigma", "ang_step", "min_quality", "stamp_cells", "lin_cells", "ang_steps", "slack_q10")
INFO = ("T", "quality", "score", "points", "candidates", "ia", "iy", "ix", "at_edge", "accepted", "searched")
SHAPE = ("S0", "Sx", "Sy", "Sxx", "Sxy", "Syy", "l1", "l2", "ex", "ey", "T_raw", "cells", "kind", "computed")
CORRIDOR = (-50, 50, -1, 1)

pytestmark = pytest.mark.gpu


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _laser(params):
    return R.Laser(params.beam_min, params.beam_max, params.beam_delta, params.range_min, params.range_max)


def _kw(p: S.Params):
    return {f: getattr(p, f) for f in FIELDS}


def _fkw(fp: F.ShapeParams):
    return dict(drop_q10=fp.drop_q10, flat_cells2=fp.flat_cells2)


def _aligner(gpu_pkg, search=None, shape=None, metric="point", **kw):
    from rtn_amd import icp
    p = icp.default_params(**kw)
    return icp.ScanAlignment(p, metric=metric, search=search, shape=shape), p


def _same_info(got: dict, want: S.Info, where=""):
    for f in INFO:
        assert got[f] == getattr(want, f), (where, f, got, want)


def _same_shape(got: dict, want: F.Shape, where=""):
    for f in SHAPE:
        assert got[f] == getattr(want, f), (where, f, got, want)


def _same(got, want: R.Result, where=""):
    ok, T, info = got
    assert ok == want.ok, (where, got, want)
    assert (info["iterations"], info["criterion"], info["correspondences"]) == (want.iterations, want.criterion, want.correspondences), (where, info, want)
    assert info["mse"] == want.mse, (where, info["mse"], want.mse)
    assert tuple(T) == tuple(want.T), (where, T, want.T)


def _room(room, n_beams=360, seed=1, p1=(0.07, 0.02, 0.01)):
    rng = np.random.default_rng(seed)
    dd = 360.0 / n_beams if n_beams > 1 else 1.0
    s0 = orc.room_scan((0.0, 0.0, 0.0), n_beams=n_beams, beam_delta_deg=dd, walls=room, rng=rng)
    s1 = orc.room_scan(p1, n_beams=n_beams, beam_delta_deg=dd, walls=room, rng=rng)
    return s0, s1, dd, R.init_guess(p1, (0.0, 0.0, 0.0))


def _corridor(seed, p0=(0.0, 0.0, 0.0), p1=(0.0, 0.10, 0.0), n_beams=360):
    rng = np.random.default_rng(seed)
    dd = 360.0 / n_beams
    s0 = orc.room_scan(p0, n_beams=n_beams, beam_delta_deg=dd, walls=CORRIDOR, rng=rng)
    s1 = orc.room_scan(p1, n_beams=n_beams, beam_delta_deg=dd, walls=CORRIDOR, rng=rng)
    return s0, s1, dd, tuple(float(v) for v in rc.compose(rc.inverse(np.array(p0)), np.array(p1)))


def _bench(off=(0.0, 0.0, 0.0), **kw):
    s0, s1, dd, truth = _room(rc.ROOM_BENCH, **kw)
    return s0, s1, dd, tuple(t + o for t, o in zip(truth, off))


def _no_beam():
    s0, s1, dd, g = _bench()
    return s0, np.full(360, np.inf, dtype=np.float32), dd, g


def _cor(seed, guess=None, **kw):
    s0, s1, dd, truth = _corridor(seed, **kw)
    return s0, s1, dd, truth if guess is None else guess


P0, F0 = S.Params(), F.ShapeParams()
# (name, scans and guess, search parameters, shape parameters, the kind it must be or None)
CASES = [
    ("bench room", lambda: _bench(), P0, F0, 0),
    ("survey room", lambda: _room(rc.ROOM_SURVEY, p1=(0.07, 0.10, 0.05)), P0, F0, 0),
    ("corridor seed 3", lambda: _cor(3), P0, F0, 1),
    ("corridor seed 4", lambda: _cor(4), P0, F0, 1),
    ("corridor heading 0.6", lambda: _cor(6, p0=(0.6, 0.0, 0.0), p1=(0.6, 0.10, 0.0)), P0, F0, 1),
    ("corridor, guess off across it", lambda: _cor(3, guess=(0.05, 0.10, 0.15)), P0, F0, 1),
    ("lin_cells 0", lambda: _cor(3), S.Params(lin_cells=0), F0, 0),
    ("lin_cells 1", lambda: _cor(3), S.Params(lin_cells=1), F0, 0),
    ("lin_cells 16: every slot of every thread", lambda: _cor(3), S.Params(lin_cells=16), F0, 1),
    ("lin_cells 16, room", lambda: _bench((0.0, 0.3, -0.2)), S.Params(lin_cells=16, ang_steps=5), F0, 0),
    ("lin_cells 9: two slots, the second partly", lambda: _cor(4), S.Params(lin_cells=9, ang_steps=3), F0, 1),
    ("ang_steps 0", lambda: _cor(4), S.Params(ang_steps=0), F0, 1),
    ("slack 64: the shape follows pass 1's choice", lambda: _cor(3), S.Params(slack_q10=64), F0, 1),
    ("slack 64, room", lambda: _bench((0.05, 0.1, 0.1)), S.Params(slack_q10=64), F0, None),
    ("drop 0", lambda: _cor(3), P0, F.ShapeParams(drop_q10=0), 0),
    ("drop 1", lambda: _cor(3), P0, F.ShapeParams(drop_q10=1), None),
    ("drop 1023", lambda: _cor(3), P0, F.ShapeParams(drop_q10=1023), None),
    ("drop 1023, room: flat in both", lambda: _bench(), P0, F.ShapeParams(drop_q10=1023), 2),
    ("flat_cells2 20: the corridor is compact", lambda: _cor(4), P0, F.ShapeParams(flat_cells2=20.0), 0),
    ("half_extent 2: the slow list", lambda: _bench((0.0, 0.5, 0.0)), S.Params(half_extent=2.0, lin_cells=12), F0, None),
    ("half_extent 2, corridor: the slow list", lambda: _cor(3, guess=(0.0, 0.10, 0.5)), S.Params(half_extent=2.0, lin_cells=12), F0, None),
    ("1 beam", lambda: _bench(n_beams=1), S.Params(ang_steps=2), F0, None),
    ("4096 beams", lambda: _cor(3, n_beams=4096), S.Params(ang_steps=5), F0, 1),
    ("4096 beams, room", lambda: _bench((0.0, 0.05, 0.0), n_beams=4096), S.Params(ang_steps=5), F0, 0),
    ("no valid beam", _no_beam, P0, F0, 0),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_search_with_shape_is_the_restatement(gpu_pkg, case):
    name, make, sp, fp, kind = case
    s0, s1, dd, guess = make()
    a, p = _aligner(gpu_pkg, search=_kw(sp), beam_delta_deg=dd)
    if fp != F0:
        a.setSearchShape(**_fkw(fp))                            # the hook uses the handle's shape parameters
    L = _laser(p)
    sc = S.scores(s0, s1, L, guess, sp)
    plain = S.search(s0, s1, L, guess, sp, scores=sc)
    want, wsh = F.search(s0, s1, L, guess, sp, fp, scores=sc)
    acc, T, info, sh = a.searchWithShape(guess, s0, s1)
    print(name, {f: sh[f] for f in ("S0", "cells", "kind", "l1", "l2")})
    _same_shape(sh, wsh, name)
    _same_info(info, want, name)
    assert acc == bool(want.accepted) and T == want.T and sh["T_raw"] == plain.T
    if kind is not None:
        assert sh["kind"] == kind, (name, sh)
    if "slow list" in name:
        assert sh["S0"] > 0 and info["score"] > 0
    if name == "no valid beam":
        assert (sh["S0"], sh["computed"], sh["kind"], info["points"]) == (0, 1, 0, 0)
    if "every slot" in name:
        assert (2 * sp.lin_cells + 1) ** 2 == 1089
    again = a.searchWithShape(guess, s0, s1)                   # a repeat: the same bits
    assert again == (acc, T, info, sh)
    assert a.lastSearchShape()["computed"] == 0                # the stateless hook leaves the pipeline's record alone
    a.close()


def test_the_hook_forms_the_shape_while_the_handle_has_it_off(gpu_pkg):
    s0, s1, dd, truth = _corridor(3)
    a, p = _aligner(gpu_pkg)                                    # search off, shape off: the defaults of both
    assert a.searchShapeParams() == (False, _fkw(F0))
    L = _laser(p)
    want, wsh = F.search(s0, s1, L, truth)
    acc, T, info, sh = a.searchWithShape(truth, s0, s1)
    _same_shape(sh, wsh)
    _same_info(info, want)
    assert sh["kind"] == 1
    _same_info(a.search(truth, s0, s1)[2], S.search(s0, s1, L, truth))   # tbnav_icp_search with the shape off: S7's T
    a.setSearchShape()
    _same_info(a.search(truth, s0, s1)[2], want)                         # and with it on: the shaped T
    a.close()


PIPE = S.Params()


def _pipeline_run():
    """six scans: two along a corridor, a scan with no valid beam (it fails, so the next pair is aligned again against the scan
    before it), a third along the corridor, then two of a room"""
    rng = np.random.default_rng(3)
    cor = [orc.room_scan((0.0, 0.10 * s, 0.0), walls=CORRIDOR, rng=rng) for s in range(4)]
    room = [orc.room_scan(q, walls=rc.ROOM_BENCH, rng=rng) for q in ((0.0, 0.0, 0.0), (0.07, 0.02, 0.01))]
    scans = np.stack([cor[0], cor[1], np.full(360, np.inf, dtype=np.float32), cor[3], room[0], room[1]])
    T_init = np.array([(0.0, 0.0, 0.0), (0.0, 0.10, 0.0), (0.0, 0.10, 0.0), (0.0, 0.20, 0.0), (0.0, 0.0, 0.0), (0.07, 0.02, 0.01)])
    return scans, T_init


_found = {}


def _want_steps(scans, T_init, L, icp_fn):
    stored, out = None, []
    for s in range(len(scans)):
        if stored is None:
            stored = s
            out.append((R.Result(True, (0.0, 0.0, 0.0), 0, 0, 0.0, R.NOT_RUN), None, None))
            continue
        key = (stored, s)
        if key not in _found:
            _found[key] = F.search(scans[stored], scans[s], L, tuple(T_init[s]), PIPE, F0)
        res, info, sh = F.match(scans[stored], scans[s], L, tuple(T_init[s]), PIPE, F0, icp=icp_fn, found=_found[key])
        out.append((res, info, sh))
        if res.ok:
            stored = s
    return out


@pytest.mark.parametrize("metric,icp_fn", [("point", R.match), ("line", LR.match)])
def test_match_step_and_batch_are_the_restated_chain(gpu_pkg, metric, icp_fn):
    scans, T_init = _pipeline_run()
    n = len(scans)
    a, p = _aligner(gpu_pkg, search=_kw(PIPE), shape=True, metric=metric)
    assert a.searchShapeParams() == (True, _fkw(F0))
    L = _laser(p)
    want = _want_steps(scans, T_init, L, icp_fn)
    one, rec, shp = [], [], []
    for s in range(n):
        one.append(a.pclICPWrapper(T_init[s], scans[s]))
        rec.append(a.lastSearch())
        shp.append(a.lastSearchShape())
    for s in range(n):
        _same(one[s], want[s][0], (metric, s))
        if want[s][1] is None:
            assert rec[s]["searched"] == 0 and shp[s]["computed"] == 0 and shp[s]["S0"] == 0 and shp[s]["T_raw"] == (0.0, 0.0, 0.0)
        else:
            _same_info(rec[s], want[s][1], (metric, s))
            _same_shape(shp[s], want[s][2], (metric, s))
    fails = [s for s in range(n) if not one[s][0]]
    assert fails == [s for s in range(n) if not want[s][0].ok] and 2 in fails and 3 not in fails   # (the room after the corridor
    assert [shp[s]["kind"] for s in (1, 3)] == [1, 1], shp                                         # is the metric's business)
    assert shp[1]["T_raw"] != rec[1]["T"] and rec[2]["accepted"] == 0 and shp[2]["computed"] == 1
    if metric == "point":
        assert shp[5]["kind"] == 0 and shp[5]["T_raw"] == rec[5]["T"]                              # room against room: compact
    # the stateless match
    m = a.pclICP(T_init[1], scans[0], scans[1])
    _same(m, want[1][0], metric)
    _same_info(a.lastSearch(), want[1][1], metric)
    _same_shape(a.lastSearchShape(), want[1][2], metric)
    # the batch: six steps, bit for bit, the realignment launch included; the record is the last scan's
    b, _ = _aligner(gpu_pkg, search=_kw(PIPE), shape=True, metric=metric)
    ok, T, info = b.wrapperBatch(T_init, scans)
    assert b.lastBatchLaunches() > 1
    for s in range(n):
        assert bool(ok[s]) == one[s][0] and tuple(T[s]) == one[s][1] and info[s] == one[s][2], (metric, s)
    assert b.lastSearch() == rec[n - 1] and b.lastSearchShape() == shp[n - 1]
    # a batch that ends in the corridor: the record is that scan's
    b.reset()
    b.wrapperBatch(T_init[:4], scans[:4])
    assert b.lastSearchShape() == shp[3] and b.lastSearch() == rec[3]
    # with the search off the shape is stored but idle
    a.setSearch(None)
    off = a.pclICP(T_init[1], scans[0], scans[1])
    _same(off, icp_fn(scans[0], scans[1], L, tuple(T_init[1])), metric)
    assert a.searchShapeParams()[0] and a.lastSearchShape()["computed"] == 0 and a.lastSearch()["searched"] == 0
    a.close(); b.close()


LONG = S.Params(lin_cells=2, ang_steps=2)
_long = {}


def _long_run():
    """1030 scans of the ellipse drive of tools/icp_time.py::loop_run (ROOM_BENCH, 500 scans a lap, 360 beams at 1 deg,
    default_rng(1)): a fresh aligner forms 1029 pairs of them, scans 1..1024 in the search's first chunk and 1025..1029 in its
    second"""
    if not _long:
        from rtn_amd import icp
        n = 1030
        phi = 2 * math.pi * np.arange(n) / 500.0
        poses = np.stack([phi + math.pi / 2, 1.0 * np.cos(phi), 0.8 * np.sin(phi)], axis=1)
        rng = np.random.default_rng(1)
        _long["scans"] = np.stack([orc.room_scan(q, n_beams=360, beam_delta_deg=1.0, walls=rc.ROOM_BENCH, rng=rng) for q in poses])
        _long["T_init"] = np.array([icp.init_guess(poses[s], poses[s - 1] if s else poses[0]) for s in range(n)])
    return _long["scans"], _long["T_init"]


@pytest.mark.parametrize("shape", [False, True], ids=["off", "on"])
def test_a_batch_longer_than_one_chunk_is_the_restated_chain(gpu_pkg, shape):
    """one wrapperBatch of 1029 pairs: more than the 1024 a launch of the search takes, so the second chunk's pairs, guesses
    and records sit at first + i.  Every pair converges (a condition on this input, checked with the restatement on the CPU:
    all 1029 pairs accepted, converged, kind 0), so scan s is aligned against scan s - 1 and the pairs either side of the
    chunk's edge are restated one by one."""
    scans, T_init = _long_run()
    a, p = _aligner(gpu_pkg, search=_kw(LONG), shape=True if shape else None)
    L = _laser(p)
    ok, T, info = a.wrapperBatch(T_init, scans)
    assert ok[1:].all(), np.flatnonzero(ok == 0)
    want = None
    for s in (1, 1023, 1024, 1025, 1026, 1029):
        g = tuple(T_init[s])
        want = F.match(scans[s - 1], scans[s], L, g, LONG, F0) if shape else S.match(scans[s - 1], scans[s], L, g, LONG)
        _same((ok[s], T[s], info[s]), want[0], s)
    _same_info(a.lastSearch(), want[1], "last")
    if shape:
        _same_shape(a.lastSearchShape(), want[2], "last")
    a.close()


def test_off_means_off(gpu_pkg):
    cases = [_corridor(3), _room(rc.ROOM_BENCH), _corridor(6, (0.6, 0.0, 0.0), (0.6, 0.10, 0.0))]
    a, p = _aligner(gpu_pkg, search=True, metric="line")
    before = []
    for s0, s1, dd, g in cases:
        r = a.searchScores(g, s0, s1)
        before.append((r[:3], r[3].copy(), a.search(g, s0, s1), a.pclICP(g, s0, s1), a.lastSearch()))
        assert a.lastSearchShape()["computed"] == 0
    a.setSearchShape(drop_q10=300, flat_cells2=1.5)
    assert a.searchShapeParams() == (True, dict(drop_q10=300, flat_cells2=1.5))
    changed = 0
    for (s0, s1, dd, g), b in zip(cases, before):
        changed += a.pclICP(g, s0, s1) != b[3]
        assert a.lastSearchShape()["computed"] == 1
    assert changed == 2                                        # the two corridors; the room is compact
    a.setSearchShape(None)
    assert a.searchShapeParams() == (False, _fkw(F0))
    for (s0, s1, dd, g), b in zip(cases, before):
        r = a.searchScores(g, s0, s1)
        assert r[:3] == b[0] and np.array_equal(r[3], b[1])
        assert a.search(g, s0, s1) == b[2]
        assert a.pclICP(g, s0, s1) == b[3] and a.lastSearch() == b[4]
        assert a.lastSearchShape()["computed"] == 0 and a.lastSearchShape()["T_raw"] == (0.0, 0.0, 0.0)
    a.close()


def test_set_search_shape_checks_its_arguments(gpu_pkg):
    capi = gpu_pkg.capi
    Lib = capi.lib()
    a, p = _aligner(gpu_pkg, search=True, shape=dict(drop_q10=100, flat_cells2=3.0))
    held = (True, dict(drop_q10=100, flat_cells2=3.0))
    assert a.searchShapeParams() == held
    d = capi.IcpSearchShapeParams()
    Lib.tbnav_icp_default_search_shape_params(C.byref(d))
    assert (d.drop_q10, d.reserved, d.flat_cells2) == (256, 0, 2.0)
    for kw in (dict(drop_q10=-1), dict(drop_q10=1024), dict(flat_cells2=0.0), dict(flat_cells2=-1.0), dict(flat_cells2=float("nan")),
               dict(flat_cells2=float("inf"))):
        assert not F.valid(F.ShapeParams(**kw)), kw
        fp = capi.IcpSearchShapeParams(256, 0, 2.0)
        for f, v in kw.items():
            setattr(fp, f, v)
        assert Lib.tbnav_icp_set_search_shape(a._h, C.byref(fp)) == capi.ERR_INVALID_ARG, kw
        assert a.searchShapeParams() == held, kw
        with pytest.raises(capi.TbnavError):
            a.setSearchShape(**kw)
    assert Lib.tbnav_icp_set_search_shape(None, None) == capi.ERR_INVALID_ARG
    assert Lib.tbnav_icp_last_search_shape(a._h, None) == capi.ERR_INVALID_ARG
    for kw in (dict(drop_q10=0, flat_cells2=1e-9), dict(drop_q10=1023, flat_cells2=1e9)):
        a.setSearchShape(**kw)
        assert a.searchShapeParams() == (True, kw)
    with pytest.raises(TypeError):
        a.setSearchShape(flat=3)
    with pytest.raises(TypeError):
        a.setSearch(shape=True)                                # setSearch's keywords stay the search's
    s0, s1, dd, g = _corridor(3)
    info, rec = capi.IcpSearchInfo(), capi.IcpSearchShape()
    out = (C.c_double * 3)()
    assert Lib.tbnav_icp_search_with_shape(a._h, s0.ctypes.data, s1.ctypes.data, 360, (C.c_double * 3)(*g), out, C.byref(info), None) == capi.ERR_INVALID_ARG
    assert Lib.tbnav_icp_search_with_shape(a._h, s0.ctypes.data, s1.ctypes.data, 4097, (C.c_double * 3)(*g), out, C.byref(info), C.byref(rec)) == capi.ERR_INVALID_ARG
    a.close()
    with pytest.raises(capi.TbnavError):
        _aligner(gpu_pkg, search=True, shape=dict(drop_q10=2000))


@pytest.fixture(scope="module")
def host(pkg):
    pkg.capi.lib()
    Lib = C.CDLL(HOST_LIB)
    Lib.hst_icp_last_error.restype = C.c_char_p
    Lib.hst_icp_pf_run_search_shape.restype = C.c_int
    Lib.hst_icp_pf_run_search_shape.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, C.c_uint64] + \
        [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
    return Lib


def _corridor_drive():
    """six scans of a drive along the corridor, 10 cm a scan, true odometry, 2 mm range noise (seed 4).  The noise is that small on
    purpose: what the test measures is what the search does to the guess, and the line metric's own drift along a corridor at
    1 cm noise (14-69 mm over these five steps across seeds 1..12 on the CPU restatement, search or no search) would drown the
    1 cm bound."""
    n = 6
    steps, poses = rc.trajectory(n, inc=(0.0, 0.10, 0.0))
    rng = np.random.default_rng(4)
    scans = np.stack([orc.room_scan(poses[s], walls=CORRIDOR, rng=rng, noise_sigma=0.002) for s in range(n)])
    odom = np.stack([steps[0][0]] + [st[1] for st in steps]).astype(np.float64)
    u = np.array([st[3] for st in steps], dtype=np.float64)
    return scans, odom, u, np.array(poses)


def test_particle_filter_class_keeps_the_pose_along_a_corridor(host, gpu_pkg):
    """bmapping::ScanAlignment::useDeviceICP(-1, PointToLine, ICPSearch{shape = true}) inside bmapping::ParticleFilter on
    _corridor_drive(): the (ok, T) the class's matcher returns per scan equals the Python mirror's and the restated chain's, and
    the filter's pose along the corridor after the six scans is within 1 cm of the truth; the same drive with shape = false is more
    than 5 cm off.  The CPU restatement's figures for this exact drive (the restated chain fed to the oracle filter, N = 40,
    k = 50, seed 11): -4.4 mm with the shape, -501.9 mm without it (the search alone pulls every step back onto the scan before)."""
    from rtn_amd import icp
    N, k = 40, 50
    scans, odom, u, poses = _corridor_drive()
    n = len(scans)

    def run(shape):
        ok = np.zeros(n, dtype=np.int32); T = np.zeros((n, 3)); pose = np.zeros((n, 3)); neff = np.zeros(n, dtype=np.int32)
        rcode = host.hst_icp_pf_run_search_shape(1, shape, 256, 2.0, 6, N, k, 6.0, 11, _p(scans), 360, n, _p(odom), _p(u), _p(ok), _p(T),
                                                 _p(pose), _p(neff))
        assert rcode == 0, host.hst_icp_last_error()
        return ok, T, pose

    ok, T, pose = run(1)
    mirror, p = _aligner(gpu_pkg, search=True, shape=True, metric="line")
    L = _laser(p)
    stored = None
    for s in range(n):
        g = icp.init_guess(odom[s + 1], odom[s])
        m = mirror.pclICPWrapper(g, scans[s])
        assert bool(ok[s]) == m[0] and tuple(T[s]) == m[1], s
        if stored is not None:
            want, info, sh = F.match(scans[stored], scans[s], L, g, icp=LR.match)
            assert m[0] == want.ok and m[1] == tuple(want.T), s
            _same_shape(mirror.lastSearchShape(), sh, s)
            assert sh.kind == 1
        if m[0]:
            stored = s
    mirror.close()
    assert ok.all()

    def along(pose):
        return float((pose[n - 1] - pose[0])[1] - (poses[n - 1] - poses[0])[1])

    d_on = along(pose)
    ok0, T0, pose0 = run(0)
    d_off = along(pose0)
    print("filter pose error along the corridor after 6 scans: shape on %.4f m, off %.4f m" % (d_on, d_off))
    assert abs(d_on) < 0.01, d_on
    assert ok0.all() and abs(d_off) > 0.05, d_off
