"""The alignment of a scan to a filter's map (include/tbnav_icp.h MAP ALIGNMENT A1-A11, csrc/icp_align_map.hip: icp_align_map<P>)
against its restatement (tests/icp_align_map_restatement.py) with ==, through the C-ABI: the hook's pairing record per beam and every
field of the info, T_out's bits included, over the case table (tests/icp_align_map_cases.py); then the tile tables, the best particle,
the filter's distance-field modes, the batch, the rejections, the kernel's name and relocalizeMap.  The occupancy goes in through the
filter's own entry points and what the restatement sees is what the filter reads back."""
import ctypes as C

import numpy as np
import pytest

import icp_align_map_cases as ac
import icp_align_map_restatement as A
import icp_restatement as R
import nav_from_map_cases as fc
import oracle_api as orc
import rbpf_cases as rc

pytestmark = pytest.mark.gpu

L_OCC = np.log(0.9 / (1 - 0.9))
MAX_OCC_DIST = 10.0
PAIRING = ("has_home", "hi", "hj", "mi", "mj", "D", "has_normal", "kept", "bx", "by", "nx", "ny")
PARAMS = ("half_cells", "gate_cells", "feature_cells", "max_flatness")


def _filter(gpu_pkg, geom, N, **kw):
    from rtn_amd.rbpf import ParticleFilter, default_params
    half = -geom.xmin
    pf = ParticleFilter(default_params(N=N, k=2, map_min=-half, map_max=half, resolution=geom.resolution), **kw)
    assert (pf.xsize, pf.ysize) == (geom.side, geom.side)
    return pf


def _aligner(gpu_pkg, icp_kw=None, device=-1):
    from rtn_amd import icp
    prm = icp.default_params(device=device, **(icp_kw or {}))
    a = icp.ScanAlignment(prm)
    laser = R.Laser(prm.beam_min, prm.beam_max, prm.beam_delta, prm.range_min, prm.range_max)
    return a, laser


def _set_occ(pf, p, occ, fresh_field=True):
    """the occupancy into slot p through tbnav_rbpf_set_log_odds (tests/test_nav_from_map_gpu.py's way)"""
    if fresh_field:
        pf.setOccDist(p, np.full(pf.G, MAX_OCC_DIST))
    pf.setLogOdds(p, np.asarray(occ).reshape(-1).astype(np.float64) * L_OCC)


def _occ_of(pf, p):
    return (pf.occDist(p).reshape(pf.xsize, pf.xsize) == 0.0).astype(np.uint8)


def _kw(p: A.Params):
    return {f: getattr(p, f) for f in PARAMS}


def _check(a, pf, particle, scan, T, p: A.Params, want: A.Result, where):
    """the hook's record and the call itself against one restated result, bit for bit"""
    got = a.alignMapPairs(pf, T, scan, particle, **_kw(p))
    for f in PAIRING:
        w = getattr(want.pairing, f)
        assert got[f].dtype == w.dtype and np.array_equal(got[f].view(np.uint8), w.view(np.uint8)), (where, f, np.nonzero(got[f] != w)[0][:8].tolist())
    ok, Tw, info = a.alignMap(pf, T, scan, particle, **_kw(p))
    assert info == dict(iterations=want.iterations, correspondences=want.correspondences, mse=want.mse, criterion=want.criterion), (where, info, want)
    assert ok == want.ok and tuple(float(v).hex() for v in Tw) == tuple(float(v).hex() for v in want.T), (where, Tw, want.T)
    assert a.lastAlignMapKernel() == f"icp_align_map<{_ladder(np.asarray(scan).size)}>", where


def _ladder(n_beams):
    per = -(-n_beams // 256)
    return next(P for P in (1, 2, 4, 6, 8, 16) if per <= P)


# ---- 1: every case ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size_id", sorted({c.size_id for c in ac.CASES}))
def test_every_case_equals_the_restatement(gpu_pkg, size_id):
    geom = ac.geom(size_id)
    pf = _filter(gpu_pkg, geom, N=2)
    for c in (c for c in ac.CASES if c.size_id == size_id):
        occ = c.occ()
        _set_occ(pf, 1, occ)
        assert np.array_equal(_occ_of(pf, 1), occ), c.name
        a, laser = _aligner(gpu_pkg, c.icp)
        assert a.lastAlignMapKernel() == ""
        cloud, beam = R.cloud(c.scan, laser)
        assert np.array_equal(cloud, c.cloud) and np.array_equal(beam, c.beam), c.name
        _check(a, pf, 1, c.scan, c.T, c.p, ac.expected(c.name), c.name)
        a.close()
    # slot 0 was never written: every tile id 0
    c = next(c for c in ac.CASES if c.size_id == size_id and c.name.startswith(("room", "origin", "stop")))
    a, _ = _aligner(gpu_pkg, c.icp)
    ok, T, info = a.alignMap(pf, c.T, c.scan, 0, **_kw(c.p))
    assert not ok and T == tuple(c.T) and info["criterion"] == R.NO_CORRESPONDENCES and info["correspondences"] == 0
    a.close(); pf.close()


# ---- 2: the tile table -----------------------------------------------------------------------------------------------------------------
def test_slots_that_share_tiles_and_then_diverge_each_align_to_their_own_map(gpu_pkg):
    c = ac.CASE["room_defaults"]
    pf = _filter(gpu_pkg, c.geom, N=3)
    a, _ = _aligner(gpu_pkg, c.icp)
    occ0 = c.occ()
    _set_occ(pf, 0, occ0)
    pf.gatherLocal(np.array([-1, 0, -1], dtype=np.int32))
    pf.copyParticle(2, pf, 0)
    for p in range(3):
        _check(a, pf, p, c.scan, c.T, c.p, ac.expected(c.name), f"shared slot {p}")
    pose = (0.3, 0.1, -0.2)
    pf.integrateScan(1, orc.room_scan(pose, walls=rc.ROOM_SMALL, noise_sigma=0.0), pose)
    for p in range(3):
        occ = _occ_of(pf, p)
        assert np.array_equal(occ, occ0) == (p != 1)
        want = A.align(occ, c.geom, c.cloud, c.beam, c.scan.size, c.T, c.p, **c.icp)
        _check(a, pf, p, c.scan, c.T, c.p, want, f"diverged slot {p}")
    a.close(); pf.close()


# ---- 3: the best particle --------------------------------------------------------------------------------------------------------------
def test_best_particle_is_the_arg_max_of_the_weights_and_the_first_of_a_tie(gpu_pkg):
    c = ac.CASE["stop_rel"]
    pf = _filter(gpu_pkg, c.geom, N=4)
    a, _ = _aligner(gpu_pkg, c.icp)
    own = []
    for p, h in enumerate((6, 5, 7, 4)):
        occ = ac.box_occ(c.size_id, 30, 33, h)()
        _set_occ(pf, p, occ)
        own.append(A.align(occ, c.geom, c.cloud, c.beam, c.scan.size, c.T, c.p, **c.icp))
    assert len({ac.digest(r) for r in own}) == 4
    for w, best in (([0.1, 0.4, 0.4, 0.1], 1), ([0.1, 0.2, 0.3, 0.4], 3), ([0.25, 0.25, 0.25, 0.25], 0), ([0.1, 0.2, 0.5, 0.2], 2)):
        pf.setParticles(w=np.array(w))
        _check(a, pf, A.BEST_PARTICLE, c.scan, c.T, c.p, own[best], f"best of {w}")
        assert pf.getRobotState()[1] == best
    a.close(); pf.close()


# ---- 4: the filter's distance-field modes ----------------------------------------------------------------------------------------------
def test_reference_field_mode_and_query_mode_give_the_same_result(gpu_pkg):
    c = ac.CASE["room_defaults"]
    pose = (0.3, 0.1, -0.2)
    scan = orc.room_scan(pose, walls=rc.ROOM_SMALL, noise_sigma=0.0)
    T = (0.31, 0.12, -0.19)
    results = []
    for mode in ("query", "reference"):
        pf = _filter(gpu_pkg, c.geom, N=2, df_mode=mode)
        pf.integrateScan(1, scan, pose)
        pf.integrateScan(1, scan, pose)
        a, laser = _aligner(gpu_pkg)
        if mode == "query":
            cloud, beam = R.cloud(scan, laser)
            want = A.align(_occ_of(pf, 1), c.geom, cloud, beam, scan.size, T, A.Params(), **ac.ICP)
            assert want.pairing.kept.sum() > 50
            _check(a, pf, 1, scan, T, A.Params(), want, mode)
        results.append((a.alignMap(pf, T, scan, 1), {f: v.tobytes() for f, v in a.alignMapPairs(pf, T, scan, 1).items()}))
        a.close(); pf.close()
    assert results[0] == results[1]


# ---- 5: the batch ----------------------------------------------------------------------------------------------------------------------
def test_a_batch_mixing_particles_and_guesses_equals_the_single_calls(gpu_pkg):
    c = ac.CASE["origin_1"]
    pf = _filter(gpu_pkg, c.geom, N=3)
    pats = fc.patterns(fc.SIZE[c.size_id])
    occs = [c.occ(), pats["one_tile"], pats["full_row"]]
    for s, occ in enumerate(occs):
        _set_occ(pf, s, occ)
    pf.setParticles(w=np.array([0.2, 0.5, 0.3]))
    a, _ = _aligner(gpu_pkg, c.icp)
    particles = [0, 1, 2, A.BEST_PARTICLE, 2, 0, 0]
    guesses = [c.T, ac.guess("s96", 40, 40), ac.guess("s96", 50, 47, th=-0.4), c.T, ac.guess("s96", 0, 95), ac.guess("s96", 95, 0, th=2.0),
               (c.T[0] - 0.02, c.T[1] + 0.01, c.T[2])]
    got = a.alignMapBatch(pf, guesses, c.scan, particles, **_kw(c.p))
    oks = 0
    for i, (s, T) in enumerate(zip(particles, guesses)):
        want = A.align(occs[1 if s < 0 else s], c.geom, c.cloud, c.beam, c.scan.size, T, c.p, **c.icp)
        assert got[i][0] == want.ok and tuple(float(v).hex() for v in got[i][1]) == tuple(float(v).hex() for v in want.T), i
        assert got[i][2] == dict(iterations=want.iterations, correspondences=want.correspondences, mse=want.mse, criterion=want.criterion), i
        assert a.alignMap(pf, T, c.scan, s, **_kw(c.p)) == got[i], i
        oks += want.ok
    assert 0 < oks < len(particles)
    a.close(); pf.close()


# ---- 6: rejections ---------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_last_records_and_the_filter_untouched(gpu_pkg):
    cp = gpu_pkg.capi
    L = cp.lib()
    c = ac.CASE["room_defaults"]
    pf = _filter(gpu_pkg, c.geom, N=2)
    _set_occ(pf, 1, c.occ())
    from rtn_amd import icp
    a = icp.ScanAlignment(icp.default_params(), search=True, shape=True)
    rng = np.random.default_rng(3)
    s0 = orc.room_scan((0.0, 0.0, 0.0), walls=rc.ROOM_SMALL, rng=rng)
    s1 = orc.room_scan((0.02, 0.05, 0.03), walls=rc.ROOM_SMALL, rng=rng)
    a.pclICPWrapper((0.0, 0.0, 0.0), s0)
    a.pclICPWrapper((0.02, 0.05, 0.03), s1)
    a.searchMap(pf, c.T, c.scan, 1)
    a.alignMap(pf, c.T, c.scan, 1)
    records = lambda: (a.lastSearch(), a.lastSearchShape(), a.lastSearchWide(), a.searchParams(), a.lastMapKernel(), a.lastGlobal(), a.lastAlignMapKernel())
    before = records()
    lo_before, parts_before = pf.logOdds(1).copy(), [np.array(v).copy() for v in pf.particles()]
    assert before[0]["searched"] == 1 and before[6] == "icp_align_map<2>"

    def untouched():
        return records() == before and np.array_equal(pf.logOdds(1), lo_before) and all(np.array_equal(x, y) for x, y in zip(pf.particles(), parts_before))

    scan = np.ascontiguousarray(c.scan, dtype=np.float32)
    info, ok, out = cp.IcpInfo(), C.c_int32(7), (C.c_double * 3)(9.0, 9.0, 9.0)
    d3 = lambda v: (C.c_double * 3)(*v)
    prm = lambda **kw: C.byref(icp._align_map_params(kw))

    def one(T=c.T, particle=1, h=a._h, f=pf._h, sc=scan.ctypes.data, nb=scan.size, par=None, o=out, k=C.byref(ok), inf=C.byref(info)):
        return L.tbnav_icp_align_map(h, f, particle, sc, nb, d3(T) if T is not None else None, par, o, k, inf)

    for particle in (2, -2, 1 << 20):
        assert one(particle=particle) == cp.ERR_INVALID_ARG and untouched()
    for kw in (dict(h=None), dict(f=None), dict(sc=None), dict(T=None), dict(o=None), dict(k=None), dict(inf=None), dict(nb=0), dict(nb=4097)):
        assert one(**kw) == cp.ERR_INVALID_ARG and untouched(), kw
    for kw in (dict(half_cells=7), dict(half_cells=257), dict(gate_cells=0), dict(gate_cells=17), dict(feature_cells=0), dict(feature_cells=5),
               dict(max_flatness=1.0), dict(max_flatness=-0.01), dict(max_flatness=float("nan")), dict(max_flatness=float("inf")), dict(reserved=1)):
        assert one(par=prm(**kw)) == cp.ERR_INVALID_ARG and untouched(), kw
        assert one(par=prm(**kw), T=(float("nan"), 0.0, 0.0)) == cp.ERR_INVALID_ARG          # A1's order
    for T in ac.NON_FINITE_GUESSES + ((0.1, -2.0001, 0.0), (0.1, 0.0, 2.0), (0.1, 1e300, 0.0), (0.1, 0.0, -1e12)):
        assert one(T=T) == cp.ERR_OUT_OF_WORLD and untouched(), T
    assert (ok.value, tuple(out)) == (7, (9.0, 9.0, 9.0))
    recs = (cp.IcpAlignMapPair * scan.size)()
    assert L.tbnav_icp_align_map_pairs(a._h, pf._h, 1, scan.ctypes.data, scan.size, d3(c.T), None, None) == cp.ERR_INVALID_ARG
    assert L.tbnav_icp_align_map_pairs(a._h, pf._h, 1, scan.ctypes.data, scan.size, d3((0.1, 5.0, 0.0)), None, C.cast(recs, C.c_void_p)) == cp.ERR_OUT_OF_WORLD
    # A8: n >= 1, and one bad pair rejects the batch
    particles = np.array([1, 0, 1], dtype=np.int32)
    Ts = np.array([c.T, c.T, c.T], dtype=np.float64)
    To, oks, infos = np.full((3, 3), 9.0), np.full(3, 7, dtype=np.int32), (cp.IcpInfo * 3)()
    batch = lambda n, ps, ts: L.tbnav_icp_align_map_batch(a._h, pf._h, scan.ctypes.data, scan.size, n, ps.ctypes.data, ts.ctypes.data, None,
                                                          To.ctypes.data, oks.ctypes.data, C.cast(infos, C.c_void_p))
    assert batch(0, particles, Ts) == cp.ERR_INVALID_ARG and batch(-1, particles, Ts) == cp.ERR_INVALID_ARG and untouched()
    bad_p = particles.copy(); bad_p[2] = 2
    bad_T = Ts.copy(); bad_T[1, 1] = 7.0
    assert batch(3, bad_p, Ts) == cp.ERR_INVALID_ARG and batch(3, particles, bad_T) == cp.ERR_OUT_OF_WORLD and untouched()
    assert (To == 9.0).all() and (oks == 7).all()
    # the stored scan is the one the steps stored, and an accepted call works afterwards and leaves the searches' records alone
    b = icp.ScanAlignment(icp.default_params(), search=True, shape=True)
    b.pclICPWrapper((0.0, 0.0, 0.0), s0)
    b.pclICPWrapper((0.02, 0.05, 0.03), s1)
    assert batch(3, particles, Ts) == cp.OK and oks.tolist() == [1, 0, 1]
    assert a.pclICPWrapper((0.0, 0.0, 0.0), s1) == b.pclICPWrapper((0.0, 0.0, 0.0), s1)
    a.searchMap(pf, c.T, c.scan, 1)
    assert records() == before
    c2 = ac.CASE["room_defaults"]
    a2, _ = _aligner(gpu_pkg, c2.icp)
    _check(a2, pf, 1, c2.scan, c2.T, c2.p, ac.expected(c2.name), "afterwards")
    a.close(); b.close(); a2.close(); pf.close()


def test_a_member_of_a_sharded_group_is_unsupported_and_changes_nothing(gpu_pkg):
    from rtn_amd.rbpf import ParticleFilterGroup, default_params
    cp = gpu_pkg.capi
    c = ac.CASE["stop_rel"]
    half = -c.geom.xmin
    grp = ParticleFilterGroup(default_params(N=4, k=2, map_min=-half, map_max=half, resolution=c.geom.resolution), [0, 0])
    a, _ = _aligner(gpu_pkg, c.icp)
    for r in range(2):
        m = grp.member(r)
        lo = m.logOdds(0).copy()
        for call in (lambda: a.alignMap(m, c.T, c.scan, 0), lambda: a.alignMapPairs(m, c.T, c.scan, 0), lambda: a.alignMapBatch(m, [c.T], c.scan, [0])):
            with pytest.raises(cp.TbnavError) as ei:
                call()
            assert ei.value.status == cp.ERR_UNSUPPORTED
        with pytest.raises(cp.TbnavError) as ei:       # a bad particle is looked at first (A1's order)
            a.alignMap(m, c.T, c.scan, 99)
        assert ei.value.status == cp.ERR_INVALID_ARG
        with pytest.raises(cp.TbnavError) as ei:       # and the group before the guess
            a.alignMap(m, (0.0, 1e9, 0.0), c.scan, 0)
        assert ei.value.status == cp.ERR_UNSUPPORTED
        assert a.lastAlignMapKernel() == "" and np.array_equal(m.logOdds(0), lo)
    a.close(); grp.close()


# ---- 7: relocalizeMap ------------------------------------------------------------------------------------------------------------------
def test_relocalize_map_is_localize_map_followed_by_align_map(gpu_pkg):
    c = ac.CASE["room_defaults"]
    pose = (0.3, 0.1, -0.2)
    scan = orc.room_scan(pose, walls=rc.ROOM_SMALL, noise_sigma=0.0)
    pf = _filter(gpu_pkg, c.geom, N=1)
    pf.integrateScan(0, scan, pose)
    pf.integrateScan(0, scan, pose)
    a, laser = _aligner(gpu_pkg)
    acc, Tg, ginfo = a.localizeMap(pf, scan, 0)
    assert acc
    ok, T, rec = a.relocalizeMap(pf, scan, 0)
    assert rec["localize"] == ginfo and (ok, T, rec["align"]) == a.alignMap(pf, Tg, scan, 0)
    cloud, beam = R.cloud(scan, laser)
    want = A.align(_occ_of(pf, 0), c.geom, cloud, beam, scan.size, Tg, A.Params(), **ac.ICP)
    assert ok == want.ok and tuple(float(v).hex() for v in T) == tuple(float(v).hex() for v in want.T)
    err = lambda q: np.hypot(q[1] - pose[1], q[2] - pose[2])
    print("relocalizeMap: the global search", err(Tg), "m off, aligned", err(T), "m off")
    # a search that is not accepted is not aligned
    ok, T, rec = a.relocalizeMap(pf, scan, 0, localize=dict(min_quality=2.0))
    assert not ok and rec["align"] is None and rec["localize"]["accepted"] == 0
    a.close(); pf.close()
