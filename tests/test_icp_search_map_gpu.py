"""The correlative search against a filter's map (include/tbnav_icp.h MAP SEARCH M1-M9, csrc/icp_search_map.hip:
icp_search_table_from_occ) against its restatement (tests/icp_search_map_restatement.py) with ==, through the C-ABI: the table,
tgt_points, the whole score volume of the first stage and of the wide stage, every field of the info, shape and wide records, over the
case table (tests/icp_search_map_cases.py); then the tile tables, the best particle, the batch, the filter's distance-field modes, a
filter too large for a stored field, the ICP handle's stored scan, the rejections, and two behaviour cases on a 400 x 400 map.  The
occupancy goes in through the filter's own entry points and what the restatement sees is what the filter reads back."""
import ctypes as C

import numpy as np
import pytest

import icp_restatement as R
import icp_search_map_cases as mc
import icp_search_map_restatement as M
import icp_search_restatement as S
import icp_search_wide_restatement as W
import nav_from_map_cases as fc
import oracle_api as orc
import rbpf_cases as rc

pytestmark = pytest.mark.gpu

L_OCC = np.log(0.9 / (1 - 0.9))
KERNEL = "icp_search_table_from_occ"
FIELDS = ("resolution", "half_extent", "sigma", "ang_step", "min_quality", "stamp_cells", "lin_cells", "ang_steps", "slack_q10")
INFO = ("T", "quality", "score", "points", "candidates", "ia", "iy", "ix", "at_edge", "accepted", "searched")
SHAPE = ("S0", "Sx", "Sy", "Sxx", "Sxy", "Syy", "l1", "l2", "ex", "ey", "T_raw", "cells", "kind", "computed")
MAX_OCC_DIST = 10.0


def _filter(gpu_pkg, geom: M.Geom, N, **kw):
    from rtn_amd.rbpf import ParticleFilter, default_params
    half = -geom.xmin
    pf = ParticleFilter(default_params(N=N, k=2, map_min=-half, map_max=half, resolution=geom.resolution), **kw)
    assert (pf.xsize, pf.ysize) == (geom.side, geom.side)
    return pf


def _aligner(gpu_pkg, p: S.Params, wp=None, shape=None, device=-1):
    """p = None: the handle's search stays OFF (M1: the map search then runs with the default parameters)"""
    from rtn_amd import icp
    prm = icp.default_params(device=device)
    a = icp.ScanAlignment(prm, search=None if p is None else {f: getattr(p, f) for f in FIELDS})
    if shape is not None:
        a.setSearchShape(drop_q10=shape.drop_q10, flat_cells2=shape.flat_cells2)
    if wp is not None:
        a.setSearchWide(lin_cells=wp.lin_cells, ang_steps=wp.ang_steps, when=wp.when)
    laser = R.Laser(prm.beam_min, prm.beam_max, prm.beam_delta, prm.range_min, prm.range_max)
    return a, laser


def _set_occ(pf, p, occ, fresh_field=True):
    """the occupancy into slot p through tbnav_rbpf_set_log_odds (tests/test_nav_from_map_gpu.py's way)"""
    if fresh_field:
        pf.setOccDist(p, np.full(pf.G, MAX_OCC_DIST))
    pf.setLogOdds(p, np.asarray(occ).reshape(-1).astype(np.float64) * L_OCC)


def _occ_of(pf, p):
    """the particle's occupied cells as the filter sees them: distance 0 to the nearest occupied cell"""
    return (pf.occDist(p).reshape(pf.xsize, pf.xsize) == 0.0).astype(np.uint8)


def _same_info(got: dict, want, where):
    for f in INFO:
        assert got[f] == getattr(want, f), (where, f, got, want)


def _same_shape(got: dict, want, where):
    if want is None:
        assert got["computed"] == 0, (where, got)
        return
    for f in SHAPE:
        assert got[f] == getattr(want, f), (where, f, got, want)


def _check(a, pf, particle, scan, T, want: M.Result, where, wide_on):
    """every hook and the search itself against one restated result"""
    tab, cnt = a.searchMapTable(pf, T, particle)
    assert np.array_equal(tab, want.table), (where, np.argwhere(tab != want.table)[:8].tolist())
    assert cnt == want.tgt_points, (where, cnt, want.tgt_points)
    out = want.outcome
    if want.scores is not None:
        _, _, info, vol = a.searchMapScores(pf, T, scan, particle)
        assert np.array_equal(vol, want.scores), (where, np.argwhere(vol != want.scores)[:8].tolist())
        _same_info(info, out.first if wide_on else out.info, where + " first stage")
    if want.wide_scores is not None:
        _, _, info, vol = a.searchMapScores(pf, T, scan, particle, wide=True)
        assert np.array_equal(vol, want.wide_scores), (where, np.argwhere(vol != want.wide_scores)[:8].tolist())
        _same_info(info, out.info, where + " wide stage")
    acc, Tw, info = a.searchMap(pf, T, scan, particle)
    _same_info(info, out.info, where)
    assert acc == bool(out.info.accepted) and tuple(Tw) == tuple(out.info.T)
    _same_info(a.lastSearch(), out.info, where + " last")
    _same_shape(a.lastSearchShape(), out.shape, where)
    lw = a.lastSearchWide()
    assert lw["ran"] == out.ran, (where, lw)
    if wide_on:
        _same_info(lw["first"], out.first, where + " wide record")
    assert a.lastMapKernel() == KERNEL


# ---- 1: every case ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size_id", sorted({c.size_id for c in mc.CASES}))
def test_every_case_equals_the_restatement(gpu_pkg, size_id):
    geom = mc.geom(size_id)
    pf = _filter(gpu_pkg, geom, N=2)
    for c in (c for c in mc.CASES if c.size_id == size_id):
        occ = c.occ()
        _set_occ(pf, 1, occ)
        assert np.array_equal(_occ_of(pf, 1), occ), c.name
        a, laser = _aligner(gpu_pkg, c.p, c.wp, c.shape)
        assert a.lastMapKernel() == ""
        assert np.array_equal(R.cloud(c.scan, laser)[0], c.scan_cloud), c.name
        _check(a, pf, 1, c.scan, c.T, mc.expected(c.name), c.name, c.wp is not None)
        a.close()
    # slot 0 was never written: every tile id 0
    c = mc.CASE["full_map"] if size_id == "s80" else next(c for c in mc.CASES if c.size_id == size_id)
    a, _ = _aligner(gpu_pkg, c.p)
    tab, cnt = a.searchMapTable(pf, c.T, 0)
    assert not tab.any() and cnt == 0
    assert a.searchMap(pf, c.T, c.scan, 0)[2]["accepted"] == 0
    a.close(); pf.close()


# ---- 2: the tile table -----------------------------------------------------------------------------------------------------------------
def test_slots_that_share_tiles_and_then_diverge_each_give_their_own_table(gpu_pkg):
    c = mc.CASE["untouched_beside"]
    pf = _filter(gpu_pkg, c.geom, N=3)
    a, _ = _aligner(gpu_pkg, c.p)
    occ0 = c.occ()
    _set_occ(pf, 0, occ0)
    pf.gatherLocal(np.array([-1, 0, -1], dtype=np.int32))
    pf.copyParticle(2, pf, 0)
    for p in range(3):
        _check(a, pf, p, c.scan, c.T, mc.expected(c.name), f"shared slot {p}", False)
    pose = (0.3, 0.1, -0.2)
    pf.integrateScan(1, orc.room_scan(pose, walls=rc.ROOM_SMALL, noise_sigma=0.0), pose)
    for p in range(3):
        occ = _occ_of(pf, p)
        assert np.array_equal(occ, occ0) == (p != 1)
        _check(a, pf, p, c.scan, c.T, M.search(occ, c.geom, c.scan_cloud, c.T, c.p), f"diverged slot {p}", False)
    a.close(); pf.close()


# ---- 3: the best particle --------------------------------------------------------------------------------------------------------------
def test_best_particle_is_the_arg_max_of_the_weights_and_the_first_of_a_tie(gpu_pkg):
    c = mc.CASE["stamp_k3"]
    pf = _filter(gpu_pkg, c.geom, N=4)
    a, _ = _aligner(gpu_pkg, c.p)
    own = []
    for p, cell in enumerate(((30, 33), (28, 30), (33, 29), (31, 31))):
        occ = np.zeros((64, 64), dtype=np.uint8)
        occ[cell] = 1
        _set_occ(pf, p, occ)
        own.append(M.search(occ, c.geom, c.scan_cloud, c.T, c.p))
    assert len({r.table.tobytes() for r in own}) == 4
    for w, best in (([0.1, 0.4, 0.4, 0.1], 1), ([0.1, 0.2, 0.3, 0.4], 3), ([0.25, 0.25, 0.25, 0.25], 0), ([0.1, 0.2, 0.5, 0.2], 2)):
        pf.setParticles(w=np.array(w))
        _check(a, pf, M.BEST_PARTICLE, c.scan, c.T, own[best], f"best of {w}", False)
        assert pf.getRobotState()[1] == best
    a.close(); pf.close()


# ---- 4: the batch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_a_batch_mixing_particles_and_guesses_equals_the_single_calls(gpu_pkg, wide):
    c = mc.CASE["origin_1_31"]
    p = c.p.with_(min_quality=0.15)                  # some pairs accepted, some not: with the wide stage on only some escalate
    wp = W.WideParams(20, 4, W.ON_REJECT) if wide else None
    pf = _filter(gpu_pkg, c.geom, N=3)
    pats = fc.patterns(fc.SIZE[c.size_id])
    occs = [pats["random"], pats["one_tile"], pats["full_row"]]
    for s, occ in enumerate(occs):
        _set_occ(pf, s, occ)
    pf.setParticles(w=np.array([0.2, 0.5, 0.3]))
    a, _ = _aligner(gpu_pkg, p, wp)
    particles = [0, 1, 2, M.BEST_PARTICLE, 2, 0, 1]
    guesses = [c.T, mc.guess("s96", 40, 40), mc.guess("s96", 50, 47, th=-0.4), c.T, mc.guess("s96", 0, 95), mc.guess("s96", 95, 0, th=2.0), mc.guess("s96", 48, 48)]
    got = a.searchMapBatch(pf, guesses, c.scan, particles)
    ran = 0
    for i, (s, T) in enumerate(zip(particles, guesses)):
        want = M.search(occs[1 if s < 0 else s], c.geom, c.scan_cloud, T, p, wp)
        _same_info(got[i][2], want.outcome.info, f"pair {i}")
        single = a.searchMap(pf, T, c.scan, s)
        assert single[2] == got[i][2] and single[1] == got[i][1], i
        ran += want.outcome.ran
    assert not wide or 0 < ran < len(particles)
    a.searchMapBatch(pf, guesses, c.scan, particles)
    _same_info(a.lastSearch(), M.search(occs[1], c.geom, c.scan_cloud, guesses[-1], p, wp).outcome.info, "the batch's last pair")
    a.close(); pf.close()


# ---- 5: the filter's distance-field modes, and a filter with no stored field -------------------------------------------------------------
def test_reference_field_mode_and_query_mode_give_the_same_result(gpu_pkg):
    c = mc.CASE["default_table"]
    pose = (0.3, 0.1, -0.2)
    scan = orc.room_scan(pose, walls=rc.ROOM_SMALL, noise_sigma=0.0)
    results = []
    for mode in ("query", "reference"):
        pf = _filter(gpu_pkg, c.geom, N=2, df_mode=mode)
        pf.integrateScan(1, scan, pose)
        pf.integrateScan(1, scan, pose)
        a, _ = _aligner(gpu_pkg, c.p)
        tab, cnt = a.searchMapTable(pf, c.T, 1)
        _, _, info, vol = a.searchMapScores(pf, c.T, c.scan, 1)
        results.append((tab, cnt, info, vol))
        if mode == "query":
            want = M.search(_occ_of(pf, 1), c.geom, c.scan_cloud, c.T, c.p)
            assert cnt == want.tgt_points > 50 and np.array_equal(tab, want.table) and np.array_equal(vol, want.scores)
        a.close(); pf.close()
    (t0, c0, i0, v0), (t1, c1, i1, v1) = results
    assert np.array_equal(t0, t1) and c0 == c1 and i0 == i1 and np.array_equal(v0, v1)


def test_a_filter_too_large_for_a_stored_field(gpu_pkg):
    """70 000 particles of 64 x 64 cells: occDist is TBNAV_ERR_UNSUPPORTED on this handle (tests/test_nav_from_map_gpu.py); the map
    search reads the tiles' bits and needs no stored field."""
    c = mc.CASE["equal_d2"]
    N = 70000
    pf = _filter(gpu_pkg, c.geom, N=N, pool_bytes=640 << 20)
    _set_occ(pf, N - 1, c.occ(), fresh_field=False)
    a, _ = _aligner(gpu_pkg, c.p)
    _check(a, pf, N - 1, c.scan, c.T, mc.expected(c.name), "slot N - 1", False)
    w = np.full(N, 0.5 / (N - 1))
    w[N - 1] = 0.5
    pf.setParticles(w=w)
    _check(a, pf, M.BEST_PARTICLE, c.scan, c.T, mc.expected(c.name), "the best of 70 000", False)
    assert a.searchMapTable(pf, c.T, 12345)[1] == 0
    with pytest.raises(gpu_pkg.capi.TbnavError) as ei:
        pf.occDist(N - 1)
    assert ei.value.status == gpu_pkg.capi.ERR_UNSUPPORTED
    a.close(); pf.close()


# ---- 6: the ICP handle's stored scan (M8) ------------------------------------------------------------------------------------------------
def test_a_map_search_leaves_the_stored_scan_alone(gpu_pkg):
    c = mc.CASE["full_map"]
    pf = _filter(gpu_pkg, c.geom, N=1)
    _set_occ(pf, 0, c.occ())
    rng = np.random.default_rng(3)
    s0 = orc.room_scan((0.0, 0.0, 0.0), walls=rc.ROOM_SMALL, rng=rng)
    s1 = orc.room_scan((0.02, 0.05, 0.03), walls=rc.ROOM_SMALL, rng=rng)
    guess = (0.02, 0.05, 0.03)
    a, _ = _aligner(gpu_pkg, S.Params())     # the search on with the defaults: 0.05 m cells, the filter's
    b, _ = _aligner(gpu_pkg, S.Params())
    for h in (a, b):
        assert h.pclICPWrapper((0.0, 0.0, 0.0), s0)[0]
    assert a.searchMap(pf, c.T, c.scan, 0)[2]["searched"] == 1 and a.lastSearch()["T"][1] != 0.0
    ga, gb = a.pclICPWrapper(guess, s1), b.pclICPWrapper(guess, s1)
    assert ga == gb and ga[0]
    assert a.lastSearch() == b.lastSearch() and a.lastSearch()["searched"] == 1
    assert a.pclICPWrapper(guess, s1) == b.pclICPWrapper(guess, s1)      # ... and the scan the step stored is the same one
    for h in (a, b, pf):
        h.close()


# ---- 7: rejections -----------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_last_records_and_the_filter_untouched(gpu_pkg):
    cp = gpu_pkg.capi
    L = cp.lib()
    c = mc.CASE["shape"]
    pf = _filter(gpu_pkg, c.geom, N=2)
    _set_occ(pf, 1, c.occ())
    a, _ = _aligner(gpu_pkg, c.p, W.WideParams(17, 3, W.ON_REJECT), c.shape)
    a.searchMap(pf, c.T, c.scan, 1)
    before = (a.lastSearch(), a.lastSearchShape(), a.lastSearchWide(), a.searchParams())
    lo_before, parts_before = pf.logOdds(1).copy(), [np.array(v).copy() for v in pf.particles()]
    assert before[0]["searched"] == 1 and before[1]["computed"] == 1

    def untouched():
        same = (a.lastSearch(), a.lastSearchShape(), a.lastSearchWide(), a.searchParams()) == before
        return same and np.array_equal(pf.logOdds(1), lo_before) and all(np.array_equal(x, y) for x, y in zip(pf.particles(), parts_before))

    scan = np.ascontiguousarray(c.scan, dtype=np.float32)
    info = cp.IcpSearchInfo()
    d3 = lambda v: (C.c_double * 3)(*v)

    def one(T=c.T, particle=1, h=a._h, f=pf._h, sc=scan.ctypes.data, nb=scan.size, inf=C.byref(info)):
        return L.tbnav_icp_search_map(h, f, particle, sc, nb, d3(T) if T is not None else None, inf)

    nan, inf_ = float("nan"), float("inf")
    for particle in (2, -2, 1 << 20):
        assert one(particle=particle) == cp.ERR_INVALID_ARG and untouched()
    for kw in (dict(h=None), dict(f=None), dict(sc=None), dict(T=None), dict(inf=None), dict(nb=0), dict(nb=4097)):
        assert one(**kw) == cp.ERR_INVALID_ARG and untouched(), kw
    for T in ((nan, 0.0, 0.0), (0.1, nan, 0.0), (0.1, 0.0, inf_), (0.1, -2.0001, 0.0), (0.1, 0.0, 2.0), (0.1, 1e300, 0.0), (0.1, 0.0, -1e12)):
        assert one(T=T) == cp.ERR_OUT_OF_WORLD and untouched(), T
        assert M.search(c.occ(), c.geom, c.scan_cloud, T, c.p) is None
    tab = np.zeros((34, 34), dtype=np.uint8)
    cnt = C.c_uint32()
    assert L.tbnav_icp_search_map_table(a._h, pf._h, 1, d3((0.1, 5.0, 0.0)), tab.ctypes.data, C.byref(cnt)) == cp.ERR_OUT_OF_WORLD
    assert L.tbnav_icp_search_map_table(a._h, pf._h, 1, d3(c.T), None, C.byref(cnt)) == cp.ERR_INVALID_ARG and untouched()
    # M7: n >= 1, and one bad pair rejects the batch
    particles = np.array([1, 0, 1], dtype=np.int32)
    Ts = np.array([c.T, c.T, c.T], dtype=np.float64)
    infos = (cp.IcpSearchInfo * 3)()
    batch = lambda n, ps, ts: L.tbnav_icp_search_map_batch(a._h, pf._h, scan.ctypes.data, scan.size, n, ps.ctypes.data, ts.ctypes.data, C.cast(infos, C.c_void_p))
    assert batch(0, particles, Ts) == cp.ERR_INVALID_ARG and batch(-1, particles, Ts) == cp.ERR_INVALID_ARG and untouched()
    bad_p = particles.copy(); bad_p[2] = 2
    bad_T = Ts.copy(); bad_T[1, 1] = 7.0
    assert batch(3, bad_p, Ts) == cp.ERR_INVALID_ARG and batch(3, particles, bad_T) == cp.ERR_OUT_OF_WORLD and untouched()
    # the parameters' resolution is not the filter's
    other, _ = _aligner(gpu_pkg, c.p.with_(resolution=0.0500001))
    assert L.tbnav_icp_search_map(other._h, pf._h, 1, scan.ctypes.data, scan.size, d3(c.T), C.byref(info)) == cp.ERR_INVALID_ARG
    assert other.lastSearch()["searched"] == 0 and other.lastMapKernel() == ""
    other.close()
    # and the accepted call still works afterwards
    assert batch(3, particles, Ts) == cp.OK
    _check(a, pf, 1, c.scan, c.T, M.search(c.occ(), c.geom, c.scan_cloud, c.T, c.p, W.WideParams(17, 3, W.ON_REJECT), c.shape), "afterwards", True)
    a.close(); pf.close()


def _records(a):
    return a.lastSearch(), a.lastSearchShape(), a.lastSearchWide(), a.searchParams(), a.lastMapKernel()


def test_a_member_of_a_sharded_group_is_unsupported_and_changes_nothing(gpu_pkg):
    """M1: a filter handle that belongs to a group (tbnav_rbpf_group, two members on this device) is TBNAV_ERR_UNSUPPORTED"""
    from rtn_amd.rbpf import ParticleFilterGroup, default_params
    cp = gpu_pkg.capi
    c = mc.CASE["full_map"]
    half = -c.geom.xmin
    grp = ParticleFilterGroup(default_params(N=4, k=2, map_min=-half, map_max=half, resolution=c.geom.resolution), [0, 0])
    own = _filter(gpu_pkg, c.geom, N=1)
    _set_occ(own, 0, c.occ())
    a, _ = _aligner(gpu_pkg, c.p)
    a.searchMap(own, c.T, c.scan, 0)
    before = _records(a)
    for r in range(2):
        m = grp.member(r)
        lo = m.logOdds(0).copy()
        with pytest.raises(cp.TbnavError) as ei:
            a.searchMap(m, c.T, c.scan, 0)
        assert ei.value.status == cp.ERR_UNSUPPORTED
        with pytest.raises(cp.TbnavError) as ei:
            a.searchMapTable(m, c.T, 0)
        assert ei.value.status == cp.ERR_UNSUPPORTED
        with pytest.raises(cp.TbnavError) as ei:       # a bad particle is looked at first (M1's order)
            a.searchMap(m, c.T, c.scan, 99)
        assert ei.value.status == cp.ERR_INVALID_ARG
        assert _records(a) == before and np.array_equal(m.logOdds(0), lo)
    _check(a, own, 0, c.scan, c.T, mc.expected(c.name), "afterwards", False)
    a.close(); own.close(); grp.close()


def test_handles_on_different_devices_are_unsupported(gpu_pkg):
    """M1.  Two ranks aliased onto one device are ONE device to this check, so only a second GPU reaches it."""
    cp = gpu_pkg.capi
    if cp.lib().tbnav_device_count() < 2:
        pytest.skip("needs two MI355X: the filter on device 0, the ICP handle on device 1")
    c = mc.CASE["full_map"]
    pf = _filter(gpu_pkg, c.geom, N=1)
    _set_occ(pf, 0, c.occ())
    a, _ = _aligner(gpu_pkg, c.p, device=1)
    before = _records(a)
    with pytest.raises(cp.TbnavError) as ei:
        a.searchMap(pf, c.T, c.scan, 0)
    assert ei.value.status == cp.ERR_UNSUPPORTED and _records(a) == before
    a.close(); pf.close()


def test_no_filter_has_a_map_that_is_not_square(gpu_pkg):
    """what the kernel's indexing (one tile count for both axes) stands on: tbnav_rbpf_create refuses 64 x 48 cells"""
    from rtn_amd.rbpf import ParticleFilter, default_params
    with pytest.raises(gpu_pkg.capi.TbnavError) as ei:
        ParticleFilter(default_params(N=1, k=2, xmin=-1.6, xmax=1.6, ymin=-1.2, ymax=1.2, resolution=0.05))
    assert ei.value.status == gpu_pkg.capi.ERR_UNSUPPORTED


def test_a_handle_whose_search_is_off_searches_with_the_defaults(gpu_pkg):
    """M1: the parameters are the defaults while the handle's search is off, and the map search leaves it off"""
    c = mc.CASE["default_table"]
    pf = _filter(gpu_pkg, c.geom, N=2)
    _set_occ(pf, 1, c.occ())
    a, _ = _aligner(gpu_pkg, None)
    assert a.searchParams()[0] is False
    _check(a, pf, 1, c.scan, c.T, M.search(c.occ(), c.geom, c.scan_cloud, c.T, S.Params()), "search off", False)
    assert a.searchParams()[0] is False
    guess = (0.02, 0.05, 0.03)
    s0, s1 = (orc.room_scan(q, walls=rc.ROOM_SMALL, noise_sigma=0.0) for q in ((0.0, 0.0, 0.0), guess))
    a.pclICPWrapper((0.0, 0.0, 0.0), s0)
    assert a.pclICPWrapper(guess, s1)[0] and a.lastSearch()["searched"] == 0       # off means off for the step
    a.close(); pf.close()


# ---- 8: behaviour, on the map the oracle's GridMapper drew --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b1", "b5", "s0", "s1", "s2"])
def test_behaviour_cases_equal_the_restatement(gpu_pkg, name):
    b = {x.name: x for x in mc.BEHAVIOURS}[name]
    lo, occ, _ = mc.behaviour_map(b.map)
    pf = _filter(gpu_pkg, mc.S400, N=1)
    pf.setLogOdds(0, lo.reshape(-1))
    assert np.array_equal(_occ_of(pf, 0), occ)
    a, laser = _aligner(gpu_pkg, b.p, b.wp)
    scan = mc.behaviour_scan(b.room, b.truth)
    T = tuple(t + o for t, o in zip(b.truth, b.off))
    want = mc.behaviour_result(name)
    acc, Tw, info = a.searchMap(pf, T, scan)
    _same_info(info, want.outcome.info, name)
    assert acc == bool(b.accepted) and a.lastSearchWide()["ran"] == want.outcome.ran
    a.close(); pf.close()
