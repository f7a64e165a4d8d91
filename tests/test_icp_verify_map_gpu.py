"""The check of a pose against a filter's map (include/tbnav_icp.h MAP CHECK V1-V10, csrc/icp_verify_map.hip: icp_verify_map<P>)
against its restatement (tests/icp_verify_map_restatement.py) with ==, through the C-ABI: every field of the record and every field of
the hook's per-beam record, over the case table (tests/icp_verify_map_cases.py); then the tile tables, the best particle, the filter's
distance-field modes, the batch, a filter of 70 000 particles, the rejections, the kernel's name and relocalizeMapChecked.  The
log-odds go in through the filter's own entry points and what the restatement sees is what the filter reads back."""
import ctypes as C

import numpy as np
import pytest

import icp_restatement as R
import icp_search_map_cases as mc
import icp_verify_map_cases as vc
import icp_verify_map_restatement as V
import oracle_api as orc
import rbpf_cases as rc

pytestmark = pytest.mark.gpu

MAX_OCC_DIST = 10.0
PARAMS = ("half_cells", "slack_cells", "max_through_q10", "max_missing_q10", "min_hit_q10")


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


def _set_lo(pf, p, lo, fresh_field=True):
    """the log-odds into slot p through tbnav_rbpf_set_log_odds"""
    if fresh_field:
        pf.setOccDist(p, np.full(pf.G, MAX_OCC_DIST))
    pf.setLogOdds(p, np.asarray(lo, dtype=np.float64).reshape(-1))


def _classes_of(pf, p) -> V.Classes:
    """what the filter reads back: the occupancy from its distance field, UNKNOWN and FREE from its own exported map (G10)"""
    occ = (pf.occDist(p).reshape(pf.xsize, pf.xsize) == 0.0)
    exported = pf.particleMap(p)
    assert np.array_equal(np.asarray(exported, dtype=np.int8).reshape(pf.xsize, pf.xsize).T == 100, occ)
    return V.Classes.from_export(exported, occ, pf.xsize)


def _kw(p: V.Params):
    return {f: getattr(p, f) for f in PARAMS}


def _ladder(n_beams):
    per = -(-n_beams // 256)
    return next(P for P in (1, 2, 4, 6, 8, 16) if per <= P)


def _check(a, pf, particle, scan, T, p: V.Params, want: V.Result, where):
    """the hook's record, its info and the call itself against one restated result, field for field"""
    info, beams = a.verifyMapBeams(pf, T, scan, particle, **_kw(p))
    for f in V.BEAM_FIELDS:
        assert beams[f].dtype == want.beams[f].dtype and np.array_equal(beams[f], want.beams[f]), (where, f, np.nonzero(beams[f] != want.beams[f])[0][:8].tolist())
    assert set(info) == set(V.INFO_FIELDS)
    for f in V.INFO_FIELDS:
        assert info[f] == want.info[f], (where, f, info, want.info)
    assert a.verifyMap(pf, T, scan, particle, **_kw(p)) == info, where
    assert a.lastVerifyMapKernel() == f"icp_verify_map<{_ladder(np.asarray(scan).size)}>", where
    return info


# ---- 1: every case ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size_id", sorted({c.size_id for c in vc.CASES}))
def test_every_case_equals_the_restatement(gpu_pkg, size_id):
    """every case in a slot of its own that nobody has written before: an all-zero tile then stays the shared tile, id 0"""
    geom = vc.geom(size_id)
    cases = [c for c in vc.CASES if c.size_id == size_id]
    pf = _filter(gpu_pkg, geom, N=len(cases) + 1)
    for slot, c in enumerate(cases, start=1):
        _set_lo(pf, slot, c.lo())
        assert np.array_equal(_classes_of(pf, slot).cls, vc.classes_of(c).cls), c.name
        a, laser = _aligner(gpu_pkg, c.icp)
        assert a.lastVerifyMapKernel() == ""
        cloud, beam = R.cloud(c.scan, laser, c.Trs)
        assert np.array_equal(cloud, c.cloud) and np.array_equal(beam, c.beam), c.name
        _check(a, pf, slot, c.scan, c.T, c.p, vc.expected(c.name), c.name)
        a.close()
    # slot 0 was never written: every tile id 0, every cell UNKNOWN
    c = next(c for c in cases if c.name.startswith(("room", "origin")))
    a, _ = _aligner(gpu_pkg, c.icp)
    info = a.verifyMap(pf, c.T, c.scan, 0, **_kw(c.p))
    assert info["walked"] > 0 and info["unseen"] == info["walked"] and info["sensor_class"] == V.C_UNKNOWN and info["free_cells"] == 0 and info["accepted"] == 0
    want = V.verify(V.Classes(np.full((geom.side, geom.side), V.C_UNKNOWN)), geom, c.cloud, c.beam, c.scan.size, c.T, c.p, V.origin_of(c.Trs))
    _check(a, pf, 0, c.scan, c.T, c.p, want, "an unwritten slot")
    a.close(); pf.close()


# ---- 2: the tile table -----------------------------------------------------------------------------------------------------------------
def test_slots_that_share_tiles_and_then_diverge_are_each_checked_against_their_own_map(gpu_pkg):
    c = vc.CASE["room_defaults"]
    pf = _filter(gpu_pkg, c.geom, N=3)
    a, _ = _aligner(gpu_pkg, c.icp)
    _set_lo(pf, 0, c.lo())
    pf.gatherLocal(np.array([-1, 0, -1], dtype=np.int32))
    pf.copyParticle(2, pf, 0)
    for p in range(3):
        _check(a, pf, p, c.scan, c.T, c.p, vc.expected(c.name), f"shared slot {p}")
    pose = (0.3, 0.1, -0.2)
    pf.integrateScan(1, orc.room_scan(pose, walls=rc.ROOM_SMALL, noise_sigma=0.0), pose)
    own = [_classes_of(pf, p) for p in range(3)]
    assert np.array_equal(own[0].cls, own[2].cls) and not np.array_equal(own[0].cls, own[1].cls)
    particles, Ts = [0, 1, 2, 1], [c.T, c.T, c.T, (c.T[0] + 0.3, c.T[1] + 0.21, c.T[2] - 0.13)]
    got = a.verifyMapBatch(pf, Ts, c.scan, particles, **_kw(c.p))                       # V8: batch == singles
    for i, (p, T) in enumerate(zip(particles, Ts)):
        want = V.verify(own[p], c.geom, c.cloud, c.beam, c.scan.size, T, c.p)
        assert _check(a, pf, p, c.scan, T, c.p, want, f"diverged slot {p}") == got[i], i
    assert got[0] == got[2] != got[1]
    a.close(); pf.close()


# ---- 3: the best particle --------------------------------------------------------------------------------------------------------------
def test_best_particle_is_the_arg_max_of_the_weights_and_the_first_of_a_tie(gpu_pkg):
    names = ("accept_through_3", "accept_through_5", "accept_missing_4", "accept_hit_3")
    c = vc.CASE[names[0]]
    pf = _filter(gpu_pkg, c.geom, N=4)
    a, _ = _aligner(gpu_pkg, c.icp)
    own = []
    for p, name in enumerate(names):
        q = vc.CASE[name]
        _set_lo(pf, p, q.lo())
        own.append(vc.run(q, p=c.p))                 # (the cases share the scan and the pose)
        assert np.array_equal(q.scan, c.scan) and q.T == c.T
    assert len({vc.digest(r) for r in own}) == 4
    for w, best in (([0.1, 0.4, 0.4, 0.1], 1), ([0.1, 0.2, 0.3, 0.4], 3), ([0.25, 0.25, 0.25, 0.25], 0), ([0.1, 0.2, 0.5, 0.2], 2)):
        pf.setParticles(w=np.array(w))
        _check(a, pf, V.BEST_PARTICLE, c.scan, c.T, c.p, own[best], f"best of {w}")
        assert pf.getRobotState()[1] == best
    a.close(); pf.close()


# ---- 4: the filter's distance-field modes ----------------------------------------------------------------------------------------------
def test_reference_field_mode_and_query_mode_give_the_same_result(gpu_pkg):
    c = vc.CASE["room_defaults"]
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
            want = V.verify(_classes_of(pf, 1), c.geom, cloud, beam, scan.size, T, V.Params())
            assert want.info["hit"] > 50 and want.info["free_cells"] > 1000
            _check(a, pf, 1, scan, T, V.Params(), want, mode)
        info, beams = a.verifyMapBeams(pf, T, scan, 1)
        results.append((info, {f: v.tobytes() for f, v in beams.items()}))
        a.close(); pf.close()
    assert results[0] == results[1]


# ---- 5: the batch ----------------------------------------------------------------------------------------------------------------------
def test_a_batch_mixing_particles_and_poses_equals_the_single_calls(gpu_pkg):
    c = vc.CASE["origin_1"]
    pf = _filter(gpu_pkg, c.geom, N=3)
    los = [c.lo(), vc.CASE["origin_31"].lo(), vc.CASE["room_odd_H"].lo()]
    for s, lo in enumerate(los):
        _set_lo(pf, s, lo)
    own = [_classes_of(pf, s) for s in range(3)]
    pf.setParticles(w=np.array([0.2, 0.5, 0.3]))
    a, _ = _aligner(gpu_pkg, c.icp)
    particles = [0, 1, 2, V.BEST_PARTICLE, 2, 0, 0]
    poses = [c.T, mc.guess("s96", 40, 40), mc.guess("s96", 50, 47, th=-0.4), c.T, mc.guess("s96", 0, 95), mc.guess("s96", 95, 0, th=2.0),
             (c.T[0] - 0.02, c.T[1] + 0.01, c.T[2])]
    got = a.verifyMapBatch(pf, poses, c.scan, particles, **_kw(c.p))
    for i, (s, T) in enumerate(zip(particles, poses)):
        want = V.verify(own[1 if s < 0 else s], c.geom, c.cloud, c.beam, c.scan.size, T, c.p)
        assert got[i] == want.info, (i, got[i], want.info)
        assert a.verifyMap(pf, T, c.scan, s, **_kw(c.p)) == got[i], i
    assert len({tuple(sorted(g.items())) for g in got}) >= 5
    a.close(); pf.close()


# ---- 6: many particles -----------------------------------------------------------------------------------------------------------------
def test_a_filter_of_70_000_particles(gpu_pkg):
    """70 000 particles of 64 x 64 cells: the tile table's index is past 2^16 rows (and occDist is refused on this handle,
    tests/test_nav_from_map_gpu.py); the check reads the tiles' bits and log-odds and needs no stored field"""
    c = vc.CASE["beams_360"]
    N = 70000
    pf = _filter(gpu_pkg, c.geom, N=N, pool_bytes=640 << 20)
    _set_lo(pf, N - 1, c.lo(), fresh_field=False)
    a, _ = _aligner(gpu_pkg, c.icp)
    _check(a, pf, N - 1, c.scan, c.T, c.p, vc.expected(c.name), "slot N - 1")
    w = np.full(N, 0.5 / (N - 1))
    w[N - 1] = 0.5
    pf.setParticles(w=w)
    _check(a, pf, V.BEST_PARTICLE, c.scan, c.T, c.p, vc.expected(c.name), "the best of 70 000")
    info = a.verifyMap(pf, c.T, c.scan, 12345, **_kw(c.p))
    assert info["unseen"] == info["walked"] > 0
    a.close(); pf.close()


# ---- 7: rejections ---------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_last_records_and_the_filter_untouched(gpu_pkg):
    cp = gpu_pkg.capi
    L = cp.lib()
    c = vc.CASE["room_defaults"]
    pf = _filter(gpu_pkg, c.geom, N=2)
    _set_lo(pf, 1, c.lo())
    from rtn_amd import icp
    a = icp.ScanAlignment(icp.default_params(), search=True, shape=True)
    rng = np.random.default_rng(3)
    s0 = orc.room_scan((0.0, 0.0, 0.0), walls=rc.ROOM_SMALL, rng=rng)
    s1 = orc.room_scan((0.02, 0.05, 0.03), walls=rc.ROOM_SMALL, rng=rng)
    a.pclICPWrapper((0.0, 0.0, 0.0), s0)
    a.pclICPWrapper((0.02, 0.05, 0.03), s1)
    a.searchMap(pf, c.T, c.scan, 1)
    a.alignMap(pf, c.T, c.scan, 1)
    a.verifyMap(pf, c.T, c.scan, 1)
    records = lambda: (a.lastSearch(), a.lastSearchShape(), a.lastSearchWide(), a.searchParams(), a.lastMapKernel(), a.lastGlobal(), a.lastAlignMapKernel(),
                       a.lastVerifyMapKernel())
    before = records()
    lo_before, parts_before = pf.logOdds(1).copy(), [np.array(v).copy() for v in pf.particles()]
    assert before[0]["searched"] == 1 and before[7] == "icp_verify_map<2>"

    def untouched():
        return records() == before and np.array_equal(pf.logOdds(1), lo_before) and all(np.array_equal(x, y) for x, y in zip(pf.particles(), parts_before))

    scan = np.ascontiguousarray(c.scan, dtype=np.float32)
    info = cp.IcpVerifyMapInfo()
    info.points = 77
    d3 = lambda v: (C.c_double * 3)(*v)
    prm = lambda **kw: C.byref(icp._verify_map_params(kw))

    def one(T=c.T, particle=1, h=a._h, f=pf._h, sc=scan.ctypes.data, nb=scan.size, par=None, inf=C.byref(info)):
        return L.tbnav_icp_verify_map(h, f, particle, sc, nb, d3(T) if T is not None else None, par, inf)

    for particle in (2, -2, 1 << 20):
        assert one(particle=particle) == cp.ERR_INVALID_ARG and untouched()
    for kw in (dict(h=None), dict(f=None), dict(sc=None), dict(T=None), dict(inf=None), dict(nb=0), dict(nb=4097)):
        assert one(**kw) == cp.ERR_INVALID_ARG and untouched(), kw
    for kw in (dict(half_cells=7), dict(half_cells=129), dict(slack_cells=-1), dict(slack_cells=9), dict(max_through_q10=-1), dict(max_through_q10=1025),
               dict(max_missing_q10=-1), dict(max_missing_q10=1025), dict(min_hit_q10=-1), dict(min_hit_q10=1025), dict(reserved=1)):
        assert one(par=prm(**kw)) == cp.ERR_INVALID_ARG and untouched(), kw
        assert one(par=prm(**kw), T=(float("nan"), 0.0, 0.0)) == cp.ERR_INVALID_ARG          # V1's order
    for T in vc.NON_FINITE_POSES + ((0.1, -2.0001, 0.0), (0.1, 0.0, 2.0), (0.1, 1e300, 0.0), (0.1, 0.0, -1e12)):
        assert one(T=T) == cp.ERR_OUT_OF_WORLD and untouched(), T
    assert info.points == 77
    recs = (cp.IcpVerifyMapBeam * scan.size)()
    assert L.tbnav_icp_verify_map_beams(a._h, pf._h, 1, scan.ctypes.data, scan.size, d3(c.T), None, None, None) == cp.ERR_INVALID_ARG
    assert L.tbnav_icp_verify_map_beams(a._h, pf._h, 1, scan.ctypes.data, scan.size, d3((0.1, 5.0, 0.0)), None, None, C.cast(recs, C.c_void_p)) == cp.ERR_OUT_OF_WORLD
    assert L.tbnav_icp_verify_map_beams(a._h, pf._h, 1, scan.ctypes.data, scan.size, d3(c.T), None, None, C.cast(recs, C.c_void_p)) == cp.OK    # info may be NULL
    # V8: n >= 1, and one bad pair rejects the batch
    particles = np.array([1, 0, 1], dtype=np.int32)
    Ts = np.array([c.T, c.T, c.T], dtype=np.float64)
    infos = (cp.IcpVerifyMapInfo * 3)()
    for q in range(3):
        infos[q].points = 77
    batch = lambda n, ps, ts, out=C.cast(infos, C.c_void_p): L.tbnav_icp_verify_map_batch(a._h, pf._h, scan.ctypes.data, scan.size, n, ps.ctypes.data,
                                                                                          ts.ctypes.data, None, out)
    assert batch(0, particles, Ts) == cp.ERR_INVALID_ARG and batch(-1, particles, Ts) == cp.ERR_INVALID_ARG and batch(3, particles, Ts, None) == cp.ERR_INVALID_ARG
    bad_p = particles.copy(); bad_p[2] = 2
    bad_T = Ts.copy(); bad_T[1, 1] = 7.0
    assert batch(3, bad_p, Ts) == cp.ERR_INVALID_ARG and batch(3, particles, bad_T) == cp.ERR_OUT_OF_WORLD and untouched()
    assert [infos[q].points for q in range(3)] == [77, 77, 77]
    # the stored scan is the one the steps stored, and an accepted call works afterwards and leaves the other records alone
    b = icp.ScanAlignment(icp.default_params(), search=True, shape=True)
    b.pclICPWrapper((0.0, 0.0, 0.0), s0)
    b.pclICPWrapper((0.02, 0.05, 0.03), s1)
    assert batch(3, particles, Ts) == cp.OK and [infos[q].points for q in range(3)] == [360, 360, 360]
    assert infos[0].hit == infos[2].hit == vc.expected(c.name).info["hit"] and infos[1].unseen == infos[1].walked
    assert a.pclICPWrapper((0.0, 0.0, 0.0), s1) == b.pclICPWrapper((0.0, 0.0, 0.0), s1)
    a.searchMap(pf, c.T, c.scan, 1)
    assert records() == before
    a.close(); b.close(); pf.close()


def test_a_member_of_a_sharded_group_is_unsupported_and_changes_nothing(gpu_pkg):
    from rtn_amd.rbpf import ParticleFilterGroup, default_params
    cp = gpu_pkg.capi
    c = vc.CASE["ray_row"]
    half = -c.geom.xmin
    grp = ParticleFilterGroup(default_params(N=4, k=2, map_min=-half, map_max=half, resolution=c.geom.resolution), [0, 0])
    a, _ = _aligner(gpu_pkg, c.icp)
    for r in range(2):
        m = grp.member(r)
        lo = m.logOdds(0).copy()
        for call in (lambda: a.verifyMap(m, c.T, c.scan, 0), lambda: a.verifyMapBeams(m, c.T, c.scan, 0), lambda: a.verifyMapBatch(m, [c.T], c.scan, [0])):
            with pytest.raises(cp.TbnavError) as ei:
                call()
            assert ei.value.status == cp.ERR_UNSUPPORTED
        with pytest.raises(cp.TbnavError) as ei:       # a bad particle is looked at first (V1's order)
            a.verifyMap(m, c.T, c.scan, 99)
        assert ei.value.status == cp.ERR_INVALID_ARG
        with pytest.raises(cp.TbnavError) as ei:       # and the group before the pose
            a.verifyMap(m, (0.0, 1e9, 0.0), c.scan, 0)
        assert ei.value.status == cp.ERR_UNSUPPORTED
        assert a.lastVerifyMapKernel() == "" and np.array_equal(m.logOdds(0), lo)
    a.close(); grp.close()


# ---- 8: relocalizeMapChecked, and the behaviour on the device ----------------------------------------------------------------------------
def test_relocalize_map_checked_verifies_the_bench_rooms_scan_and_not_the_survey_rooms(gpu_pkg):
    """the bench room's map after 12 scans (drawn by the oracle's GridMapper, set through the filter's entry point): the bench room's
    scan is found, aligned and VERIFIED; the survey room's scan is not, whether or not the search's own rejection is overridden.  Each
    step equals the call it is made of, and the check's record equals the restatement at the pose the device found."""
    lo, occ, _ = mc.behaviour_map("bench")
    pf = _filter(gpu_pkg, mc.S400, N=1)
    pf.setLogOdds(0, lo.reshape(-1))
    classes = _classes_of(pf, 0)
    assert np.array_equal(classes.cls, vc.behaviour_classes("bench").cls)
    a, laser = _aligner(gpu_pkg)
    scan = mc.behaviour_scan("bench", vc.BEHAVIOUR_TRUTH)
    verified, T, rec = a.relocalizeMapChecked(pf, scan, 0)
    acc, Tg, ginfo = a.localizeMap(pf, scan, 0)
    assert acc and rec["localize"] == ginfo
    ok, Ta, ainfo = a.alignMap(pf, Tg, scan, 0)
    assert (rec["aligned"], rec["align"]) == (ok, ainfo) and T == (Ta if ok else Tg)
    cloud, beam = R.cloud(scan, laser)
    want = V.verify(classes, mc.S400, cloud, beam, scan.size, T, V.Params())
    assert rec["verify"] == want.info == a.verifyMap(pf, T, scan, 0)
    print("bench scan in the bench map:", T, rec["verify"])
    assert verified and rec["verify"]["accepted"] == 1
    assert a.relocalizeMap(pf, scan, 0)[:2] == (ok, Ta if ok else Tg)           # relocalizeMap itself is untouched
    # the other room's scan
    wrong = mc.behaviour_scan("survey", vc.BEHAVIOUR_TRUTH)
    verified, T, rec = a.relocalizeMapChecked(pf, wrong, 0)
    print("survey scan in the bench map:", T, rec["localize"]["quality"], rec["verify"])
    assert not verified and (rec["verify"] is None) == (rec["localize"]["accepted"] == 0)
    verified, T, rec = a.relocalizeMapChecked(pf, wrong, 0, even_if_rejected=True)
    cloud, beam = R.cloud(wrong, laser)
    assert rec["verify"] == V.verify(classes, mc.S400, cloud, beam, wrong.size, T, V.Params()).info
    print("... even if rejected:", T, rec["verify"])
    assert not verified and rec["verify"]["accepted"] == 0
    # a search that is not accepted is neither aligned nor checked
    verified, T, rec = a.relocalizeMapChecked(pf, scan, 0, localize=dict(min_quality=2.0))
    assert not verified and rec["align"] is None and rec["verify"] is None and rec["localize"]["accepted"] == 0
    a.close(); pf.close()
