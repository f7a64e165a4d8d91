"""The hypotheses of the global search (include/tbnav_icp.h HYPOTHESES H1-H10, csrc/icp_hyp.hip behind csrc/icp_global.hip) against their
brute-force restatement (tests/icp_hyp_restatement.py) with ==, through the C-ABI: every field of every hypothesis, T's bits included,
every field of the record but refined_blocks and rounds (bounded), and the candidate hook's three arrays, over the case table
(tests/icp_hyp_cases.py); K = 1 against localizeMap; the other records untouched; the kernel names; the tile tables, the best particle,
the filter's distance-field modes; every rejection of H1 and H6; a handle whose buffers grow; and relocalizeMapHypotheses on the rectangle
and the room against the restated chain.  The occupancy goes in through the filter's own entry points and is read back."""
import ctypes as C

import numpy as np
import pytest

import icp_global_cases as gc
import icp_global_restatement as G
import icp_hyp_cases as hc
import icp_hyp_restatement as H
import icp_restatement as R
import icp_verify_map_restatement as V
import oracle_api as orc

pytestmark = pytest.mark.gpu

L_OCC = np.log(0.9 / (1 - 0.9))
ROOM_64 = (-1.3, 1.2, -1.1, 1.4)
MAX_OCC_DIST = 10.0
FIELDS = ("resolution", "half_extent", "sigma", "ang_step", "min_quality", "stamp_cells", "lin_cells", "ang_steps", "slack_q10")
HYP = ("T", "quality", "score", "ia", "tx", "ty", "accepted")
INFO = ("searched", "n", "n_peaks", "best_score", "floor_score", "points", "occupied", "blocks", "floor_blocks", "candidates")
HP_FIELDS = ("max_hyp", "floor_q10", "sep_cells", "sep_steps", "wrap")
GLOBAL_KERNELS = ["icp_global_field", "icp_global_pool", "icp_global_offsets", "icp_global_bound", "icp_global_hist", "icp_global_list",
                  "icp_global_refine"]
KERNELS = GLOBAL_KERNELS + ["icp_hyp_collect", "icp_hyp_knock", "icp_hyp_select"]


def _filter(gpu_pkg, geom, N, **kw):
    from rtn_amd.rbpf import ParticleFilter, default_params
    half = -geom.xmin
    pf = ParticleFilter(default_params(N=N, k=2, map_min=-half, map_max=half, resolution=geom.resolution), **kw)
    assert (pf.xsize, pf.ysize) == (geom.side, geom.side)
    return pf


def _aligner(gpu_pkg, sp, device=-1):
    from rtn_amd import icp
    return icp.ScanAlignment(icp.default_params(device=device), search=None if sp is None else {f: getattr(sp, f) for f in FIELDS})


def _set_occ(pf, p, occ, fresh_field=True):
    if fresh_field:
        pf.setOccDist(p, np.full(pf.G, MAX_OCC_DIST))
    pf.setLogOdds(p, np.asarray(occ).reshape(-1).astype(np.float64) * L_OCC)


def _occ_of(pf, p):
    return (pf.occDist(p).reshape(pf.xsize, pf.xsize) == 0.0).astype(np.uint8)


def _gkw(gp: G.Params) -> dict:
    return dict(ang_count=gp.ang_count, ang_step=gp.ang_step, pool_log2=gp.pool_log2, region=gp.region, min_quality=gp.min_quality)


def _hkw(hp: H.HypParams) -> dict:
    return {f: getattr(hp, f) for f in HP_FIELDS}


def _check(a, pf, particle, scan, gp, hp, want: H.Result, where, hook=True):
    """the call, its record and its hook against one restated result; K = 1 against localizeMap"""
    assert want.status == "ok", where
    before = (a.lastGlobal(), a.lastGlobalKernels(), a.lastSearch(), a.lastMapKernel())
    hyps, info = a.localizeMapHypotheses(pf, scan, particle, hyp=_hkw(hp), **_gkw(gp))
    assert (a.lastGlobal(), a.lastGlobalKernels(), a.lastSearch(), a.lastMapKernel()) == before, where
    for f in INFO:
        assert info[f] == want.info[f], (where, f, info, want.info)
    assert len(hyps) == len(want.hyps) == info["n"], (where, hyps, want.hyps)
    for i, (got, w) in enumerate(zip(hyps, want.hyps)):
        for f in HYP:
            assert got[f] == getattr(w, f), (where, i, f, got, w)
    if info["best_score"] > 0:
        assert info["floor_blocks"] <= info["refined_blocks"] <= info["blocks"] and 1 <= info["rounds"], (where, info)
    assert a.lastHyp() == info
    assert a.lastHypKernels() == (KERNELS if info["best_score"] > 0 else GLOBAL_KERNELS), where
    if hook:
        index, score, peak = a.localizeMapHypCandidates(pf, scan, particle, hyp=_hkw(hp), **_gkw(gp))
        assert np.array_equal(index, want.index) and np.array_equal(score, want.score) and np.array_equal(peak, want.peak), where
        assert a.lastHyp() == info                                   # the hook is stateless
    # K = 1 is the global search's answer; a cap below n fills cap and reports n
    one, info1 = a.localizeMapHypotheses(pf, scan, particle, hyp=dict(_hkw(hp), max_hyp=1), **_gkw(gp))
    acc, T, ginfo = a.localizeMap(pf, scan, particle, **_gkw(gp))
    if info["best_score"] > 0:
        y = one[0]
        assert len(one) == 1 and info1["n_peaks"] == info["n_peaks"], where
        assert (y["T"], y["ia"], y["tx"], y["ty"], y["score"], y["quality"], y["accepted"]) == (
            tuple(T), ginfo["ia"], ginfo["tx"], ginfo["ty"], ginfo["score"], ginfo["quality"], ginfo["accepted"]), where
        assert hyps[0] == y
    else:
        assert one == [] and info1["n"] == 0, where
    if info["n"] > 1:
        few, info2 = a.localizeMapHypotheses(pf, scan, particle, hyp=_hkw(hp), cap=1, **_gkw(gp))
        assert few == hyps[:1] and info2["n"] == info["n"], where
    return info


# ---- 1: every case ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size_id", sorted({c.size_id for c in hc.CASES}))
def test_every_case_equals_the_restatement(gpu_pkg, size_id):
    pf = _filter(gpu_pkg, gc.geom(size_id), N=2)
    for c in (c for c in hc.CASES if c.size_id == size_id):
        occ = c.occ()
        _set_occ(pf, 1, occ)
        assert np.array_equal(_occ_of(pf, 1), occ), c.name
        a = _aligner(gpu_pkg, c.search)
        assert a.lastHypKernels() == [] and a.lastHyp() == {k: 0 for k in a.lastHyp()}
        _check(a, pf, 1, c.scan, c.gp, c.hp, hc.expected(c.name), c.name)
        a.close()
    # slot 0 was never written: every tile id 0, best = 0, empty
    c = next(c for c in hc.CASES if c.size_id == size_id and len(c.cloud) > 0)
    a = _aligner(gpu_pkg, c.search)
    hyps, info = a.localizeMapHypotheses(pf, c.scan, 0, hyp=_hkw(c.hp), **_gkw(c.gp))
    assert hyps == [] and (info["searched"], info["n"], info["n_peaks"], info["best_score"], info["occupied"], info["candidates"]) == (1, 0, 0, 0, 0, 0)
    a.close(); pf.close()


# ---- 2: the tile table, the best particle, the field modes ------------------------------------------------------------------------------------
def test_slots_that_share_tiles_and_then_diverge_each_give_their_own_result(gpu_pkg):
    c = hc.CASE["region_ragged"]
    pf = _filter(gpu_pkg, c.geom, N=3)
    a = _aligner(gpu_pkg, c.search)
    occ0 = c.occ()
    _set_occ(pf, 0, occ0)
    pf.gatherLocal(np.array([-1, 0, -1], dtype=np.int32))
    pf.copyParticle(2, pf, 0)
    for p in range(3):
        _check(a, pf, p, c.scan, c.gp, c.hp, hc.expected(c.name), f"shared slot {p}")
    pose = (0.3, 0.1, -0.2)
    pf.integrateScan(1, orc.room_scan(pose, walls=(-0.9, 0.8, -0.7, 0.9), noise_sigma=0.0), pose)
    for p in range(3):
        occ = _occ_of(pf, p)
        assert np.array_equal(occ, occ0) == (p != 1)
        _check(a, pf, p, c.scan, c.gp, c.hp, H.localize_hyp(occ, c.geom, c.cloud, c.search, c.gp, c.hp), f"diverged slot {p}")
    a.close(); pf.close()


def test_best_particle_is_the_arg_max_of_the_weights_and_the_first_of_a_tie(gpu_pkg):
    c = hc.CASE["sep_tx_out"]
    pf = _filter(gpu_pkg, c.geom, N=4)
    a = _aligner(gpu_pkg, c.search)
    own = []
    for p, cell in enumerate(((30, 33), (28, 30), (33, 29), (31, 31))):
        occ = np.zeros((64, 64), dtype=np.uint8)
        occ[cell] = 1
        occ[cell[0] + 8, cell[1]] = 1
        _set_occ(pf, p, occ)
        own.append(H.localize_hyp(occ, c.geom, c.cloud, c.search, c.gp, c.hp))
    assert len({tuple((y.tx, y.ty) for y in r.hyps) for r in own}) == 4 and all(len(r.hyps) == 2 for r in own)
    for w, best in (([0.1, 0.4, 0.4, 0.1], 1), ([0.1, 0.2, 0.3, 0.4], 3), ([0.25, 0.25, 0.25, 0.25], 0), ([0.1, 0.2, 0.5, 0.2], 2)):
        pf.setParticles(w=np.array(w))
        _check(a, pf, G.BEST_PARTICLE, c.scan, c.gp, c.hp, own[best], f"best of {w}")
    a.close(); pf.close()


def test_reference_field_mode_and_query_mode_give_the_same_result(gpu_pkg):
    geom, sp = gc.geom("s64"), gc.SP5
    gp, hp = G.Params(ang_count=8, ang_step=np.pi / 4), H.HypParams(sep_steps=1, floor_q10=700)
    pose = (0.3, 0.1, -0.2)
    scan = orc.room_scan(pose, walls=ROOM_64, noise_sigma=0.0)
    results = []
    for mode in ("query", "reference"):
        pf = _filter(gpu_pkg, geom, N=2, df_mode=mode)
        pf.integrateScan(1, scan, pose)
        pf.integrateScan(1, scan, pose)
        a = _aligner(gpu_pkg, sp)
        if mode == "query":
            want = H.localize_hyp(_occ_of(pf, 1), geom, R.cloud(scan, gc.LASER)[0], sp, gp, hp)
            assert want.info["occupied"] > 50 and want.info["n_peaks"] >= 1
            _check(a, pf, 1, scan, gp, hp, want, mode)
        hyps, info = a.localizeMapHypotheses(pf, scan, 1, hyp=_hkw(hp), **_gkw(gp))
        results.append((hyps, {k: v for k, v in info.items() if k not in ("refined_blocks", "rounds")},
                        [x.tolist() for x in a.localizeMapHypCandidates(pf, scan, 1, hyp=_hkw(hp), **_gkw(gp))]))
        a.close(); pf.close()
    assert results[0] == results[1]


# ---- 3: rejections -----------------------------------------------------------------------------------------------------------------------
def _records(a):
    return (a.lastSearch(), a.lastSearchShape(), a.lastSearchWide(), a.searchParams(), a.lastMapKernel(), a.lastGlobal(), a.lastGlobalKernels(),
            a.lastHyp(), a.lastHypKernels())


def test_every_rejection_of_h1_and_h6_leaves_the_records_as_they_were(gpu_pkg):
    cp = gpu_pkg.capi
    L = cp.lib()
    c = hc.CASE["floor_equal"]
    pf = _filter(gpu_pkg, c.geom, N=2)
    _set_occ(pf, 1, c.occ())
    a = _aligner(gpu_pkg, c.search)
    a.localizeMap(pf, c.scan, 1, **_gkw(c.gp))
    _check(a, pf, 1, c.scan, c.gp, c.hp, hc.expected(c.name), c.name, hook=False)
    before = _records(a)
    assert before[5]["searched"] == 1 and before[7]["searched"] == 1 and before[7]["n"] == 2
    lo_before = pf.logOdds(1).copy()

    def untouched():
        return _records(a) == before and np.array_equal(pf.logOdds(1), lo_before)

    scan = np.ascontiguousarray(c.scan, dtype=np.float32)
    info = cp.IcpHypInfo()
    hyps = (cp.IcpHypothesis * 8)()

    def gparams(gp=c.gp, **kw):
        p = cp.IcpGlobalParams()
        L.tbnav_icp_default_global_params(C.byref(p))
        p.ang_count, p.ang_step, p.pool_log2 = gp.ang_count, gp.ang_step, gp.pool_log2
        p.region[:] = gp.region
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def hparams(hp=c.hp, **kw):
        p = cp.IcpHypParams()
        L.tbnav_icp_default_hyp_params(C.byref(p))
        for f in HP_FIELDS:
            setattr(p, f, getattr(hp, f))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def one(particle=1, h=a._h, f=pf._h, sc=scan.ctypes.data, nb=scan.size, g=None, p=None, out=C.cast(hyps, C.c_void_p), cap=8, inf=C.byref(info)):
        return L.tbnav_icp_localize_map_hyp(h, f, particle, sc, nb, C.byref(g) if g is not None else None, C.byref(p) if p is not None else None,
                                            out, cap, inf)

    assert one(g=gparams(), p=hparams()) == cp.OK and info.n == 2 and untouched()
    for kw in (dict(h=None), dict(f=None), dict(sc=None), dict(inf=None), dict(out=None), dict(cap=0), dict(cap=-1), dict(nb=0), dict(nb=4097),
               dict(particle=2), dict(particle=-2)):
        assert one(g=gparams(), p=hparams(), **kw) == cp.ERR_INVALID_ARG and untouched(), kw
    for kw in hc.BAD_PARAMS:
        assert one(g=gparams(), p=hparams(**kw)) == cp.ERR_INVALID_ARG and untouched(), kw
        assert not H.valid(c.hp.with_(**kw)), kw
    for kw in (dict(ang_count=0), dict(pool_log2=6), dict(reserved=1)):
        assert one(g=gparams(**kw), p=hparams()) == cp.ERR_INVALID_ARG and untouched(), kw
    count = C.c_int64()
    hook = L.tbnav_icp_localize_map_hyp_candidates
    assert hook(a._h, pf._h, 1, scan.ctypes.data, scan.size, C.byref(gparams()), C.byref(hparams(wrap=2)), None, None, None, 0,
                C.byref(count)) == cp.ERR_INVALID_ARG
    assert hook(a._h, pf._h, 1, scan.ctypes.data, scan.size, C.byref(gparams()), C.byref(hparams()), None, None, None, 0, None) == cp.ERR_INVALID_ARG
    assert hook(a._h, pf._h, 1, scan.ctypes.data, scan.size, C.byref(gparams()), C.byref(hparams()), None, None, None, 4, C.byref(count)) == cp.ERR_INVALID_ARG
    assert untouched()
    # a member of a sharded group is UNSUPPORTED; a bad parameter is looked at first
    from rtn_amd.rbpf import ParticleFilterGroup, default_params
    half = -c.geom.xmin
    grp = ParticleFilterGroup(default_params(N=4, k=2, map_min=-half, map_max=half, resolution=c.geom.resolution), [0, 0])
    m = grp.member(0)
    assert one(f=m._h, particle=0, g=gparams(), p=hparams()) == cp.ERR_UNSUPPORTED and one(f=m._h, particle=0, g=gparams(), p=hparams(max_hyp=0)) == cp.ERR_INVALID_ARG
    assert untouched()
    grp.close()
    # H1's bins and H6's two limits, on a fully occupied map of 200 cells that scores one point
    big = _filter(gpu_pkg, hc.G200, N=1)
    _set_occ(big, 0, hc.FULL_200())
    assert int(_occ_of(big, 0).sum()) == 200 * 200
    assert H.bins(hc.BINS_GP, 200, hc.BINS_HP) > H.MAX_BINS
    assert one(f=big._h, particle=0, g=gparams(hc.BINS_GP), p=hparams(hc.BINS_HP)) == cp.ERR_UNSUPPORTED and untouched()
    cloud = R.cloud(c.scan, gc.LASER)[0]
    for name, gp, hp in hc.REFUSED:
        vol = G.localize(hc.FULL_200(), hc.G200, cloud, c.search, gp)
        t = H.floor_of(int(vol.scores.max()), hp.floor_q10)
        over = int((vol.bounds >= t).sum()) > H.MAX_REFINE if name == "floor_blocks" else (
            int((vol.bounds >= t).sum()) <= H.MAX_REFINE and int((vol.scores >= t).sum()) > H.MAX_CANDIDATES)
        assert over and H.hypotheses(vol, hc.G200, gp, hp).status == "unsupported", name
        assert one(f=big._h, particle=0, g=gparams(gp), p=hparams(hp)) == cp.ERR_UNSUPPORTED and untouched(), name
    big.close()
    _check(a, pf, 1, c.scan, c.gp, c.hp, hc.expected(c.name), "afterwards")
    a.close(); pf.close()


# ---- 4: the buffers ---------------------------------------------------------------------------------------------------------------------------
def test_a_handle_whose_buffers_grow_from_a_24_cell_to_a_96_cell_map_and_back(gpu_pkg):
    geom = gc.geom("r24")
    occ24 = gc.room("r24")()
    scan24 = gc.scan_in(occ24, geom, (np.pi / 4, 0.7, -0.4), keep=gc.spread(72))
    gp24, hp24 = G.Params(ang_count=8, ang_step=np.pi / 4, pool_log2=1), H.HypParams(sep_cells=2, sep_steps=1, floor_q10=600)
    want24 = H.localize_hyp(occ24, geom, R.cloud(scan24, gc.LASER)[0], gc.SP50, gp24, hp24)
    assert want24.info["n_peaks"] >= 1
    large = hc.CASE["room"]
    a = _aligner(gpu_pkg, None)
    small = _filter(gpu_pkg, geom, N=1)
    _set_occ(small, 0, occ24)
    pf = _filter(gpu_pkg, large.geom, N=1)
    _set_occ(pf, 0, large.occ())
    for which in ("small", "large", "small"):
        a.setSearch(**{f: getattr(gc.SP50 if which == "small" else large.search, f) for f in FIELDS})
        if which == "small":
            _check(a, small, 0, scan24, gp24, hp24, want24, which)
        else:
            _check(a, pf, 0, large.scan, large.gp, large.hp, hc.expected(large.name), which)
    a.close(); small.close(); pf.close()


# ---- 5: the chain -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rectangle", "room"])
def test_relocalize_with_hypotheses_equals_the_restated_chain(gpu_pkg, which):
    c = hc.CASE[which]
    lo, occ, scan, want = hc.behaviour(which)
    pf = _filter(gpu_pkg, c.geom, N=1)
    pf.setOccDist(0, np.full(pf.G, MAX_OCC_DIST))
    pf.setLogOdds(0, lo.reshape(-1))
    assert np.array_equal(_occ_of(pf, 0), occ)
    exported = pf.particleMap(0)
    assert np.array_equal(V.Classes.from_export(exported, occ != 0, 96).cls, V.Classes.from_log_odds(lo, occ).cls)
    a = _aligner(gpu_pkg, c.search)
    got = a.relocalizeMapHypotheses(pf, scan, 0, localize=_gkw(c.gp), hyp=_hkw(c.hp))
    assert (got["verified_count"], got["best"], got["ambiguous"], got["T"]) == (want["verified_count"], want["best"], want["ambiguous"], want["T"])
    assert len(got["hypotheses"]) == len(want["hypotheses"])
    for g, w in zip(got["hypotheses"], want["hypotheses"]):
        assert g["found"]["T"] == w["found"].T and g["found"]["accepted"] == w["found"].accepted
        assert g["fine"][0] == w["fine"].ok and g["fine"][1] == tuple(w["fine"].T)
        assert g["T"] == w["T"] and g["verified"] == w["verified"]
        assert all(g["check"][k] == w["check"][k] for k in ("walked", "hit", "through", "missing", "accepted"))
    if which == "rectangle":
        assert got["ambiguous"] and got["verified_count"] == 2 and [h["verified"] for h in got["hypotheses"]] == [True, True]
    else:
        assert not got["ambiguous"] and got["best"] == 0 and [h["verified"] for h in got["hypotheses"]] == [True, False, False, False]
        assert all(h["found"]["accepted"] for h in got["hypotheses"])
    a.close(); pf.close()
