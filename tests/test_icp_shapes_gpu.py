"""The device ICP (include/tbnav_icp.h, csrc/icp.hip) on the cases of tests/icp_cases.py, against the numpy restatements
(tests/icp_restatement.py, tests/icp_line_restatement.py) bit for bit: every instantiation of icp_align<Metric, P> for both
metrics at its edges, exact distance ties across the chains of the nearest-neighbour scan, every stop rule, sparse scans, 2 and 3
correspondences, the distance gate on its edge, guesses that are not numbers, lasers that take createPointCloud's other
branches, one handle at changing beam counts, and tbnav_icp_step_batch over mixed runs at 767 and 4096 beams.  No tolerance
anywhere: ok, T as bit patterns, iterations, criterion, correspondences, mse.  test_icp_cases.py shows on the CPU that the cases
do what they are here for (among them: a merge with the wrong tie-break gives another T on the tie cases)."""
import numpy as np
import pytest

import icp_cases as ic
import icp_line_restatement as LR
import icp_restatement as R
import rbpf_cases as rc

pytestmark = pytest.mark.gpu


def _laser(params):
    return R.Laser(params.beam_min, params.beam_max, params.beam_delta, params.range_min, params.range_max)


def _aligner(gpu_pkg, kw, metric="point"):
    from rtn_amd import icp
    p = icp.default_params(**kw)
    assert _laser(p) == ic.laser(kw) and tuple(p.Trs) == tuple(float(v) for v in kw.get("Trs", (0.0, 0.0, 0.0)))
    return icp.ScanAlignment(p, metric=metric), p


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64).tolist()


def _same(got, want: R.Result, where=""):
    ok, T, info = got
    assert ok == want.ok, (where, got, want)
    assert (info["iterations"], info["criterion"], info["correspondences"]) == (want.iterations, want.criterion, want.correspondences), (where, info, want)
    assert _bits(info["mse"]) == _bits(want.mse), (where, info["mse"], want.mse)
    assert _bits(T) == _bits(want.T), (where, T, want.T)


def _same_run(a, b, where=""):
    """two runs of the kernel on the same input: identical bits"""
    assert a[0] == b[0] and _bits(a[1]) == _bits(b[1]) and a[2]["mse"] == b[2]["mse"] and a[2] == b[2], (where, a, b)


def _invalid_arg(gpu_pkg, fn, *args):
    with pytest.raises(gpu_pkg.capi.TbnavError) as e:
        fn(*args)
    assert e.value.status == gpu_pkg.capi.ERR_INVALID_ARG, e.value


def _match_case(gpu_pkg, case):
    n = case.tgt.size
    for metric in ("point", "line"):
        a, p = _aligner(gpu_pkg, case.kw, metric)
        try:
            if metric == "line" and n > LR.MAX_BEAMS:
                _invalid_arg(gpu_pkg, a.pclICP, case.T, case.tgt, case.src)
                continue
            want = ic.restate(case, metric)
            got = a.pclICP(case.T, case.tgt, case.src)
            _same(got, want, (case.name, metric))
            _same_run(a.pclICP(case.T, case.tgt, case.src), got, (case.name, metric, "second run"))
        finally:
            a.close()


@pytest.mark.parametrize("case", ic.beam_count_cases(), ids=lambda c: c.name)
def test_every_instantiation_at_its_edges(gpu_pkg, case):
    _match_case(gpu_pkg, case)


def test_the_beam_counts_cover_every_instantiation():
    """What the parametrised test above launches, derived from run_pairs' dispatch (ceil(n / 256) -> P): a change of the beam
    counts or of the dispatch table cannot silently shrink the coverage."""
    point = {ic.beams_per_thread(c.tgt.size) for c in ic.beam_count_cases()}
    line = {ic.beams_per_thread(c.tgt.size, "line") for c in ic.beam_count_cases() if c.tgt.size <= LR.MAX_BEAMS}
    assert point == {1, 2, 3, 4, 6, 8, 12, 16}, point
    assert line == {1, 2, 3, 4, 6, 8}, line
    assert {ic.chains(P) for P in point} == {1, 2, 4}


@pytest.mark.parametrize("case", ic.tie_cases(), ids=lambda c: c.name)
def test_distance_ties_go_to_the_lowest_beam_index(gpu_pkg, case):
    _match_case(gpu_pkg, case)


@pytest.mark.parametrize("case", ic.criterion_cases(), ids=lambda c: c.name)
def test_every_stop_rule(gpu_pkg, case):
    _match_case(gpu_pkg, case)


@pytest.mark.parametrize("case", ic.edge_cases(), ids=lambda c: c.name)
def test_edges_of_the_layout_and_of_the_contract(gpu_pkg, case):
    _match_case(gpu_pkg, case)


def test_clouds_and_normals_of_the_edge_lasers_and_the_edge_beam_counts(gpu_pkg):
    by_name = {c.name: c for c in ic.all_cases()}
    names = ["negative_delta_and_beam_max", "beam_min_minus_pi_and_Trs", "range_bounds", "sparse_n360_5pct_bunched",
             "sparse_n4096_1pct_spread", "tie_w135_n405", "n1", "n2", "n3", "n5", "n4095", "n4096"]
    for name in names:
        c = by_name[name]
        n = c.tgt.size
        a, p = _aligner(gpu_pkg, c.kw, "line" if n <= LR.MAX_BEAMS else "point")
        L, Trs = _laser(p), tuple(p.Trs)
        for sc in (c.tgt, c.src):
            got = a.cloud(sc)
            want, _ = R.cloud(sc, L, Trs)
            assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
            if n <= LR.MAX_BEAMS:
                nxy, has = a.normals(sc)
                want_n, want_h = LR.normals(sc, L, Trs)
                assert np.array_equal(has, want_h) and np.array_equal(nxy.view(np.uint32), want_n.view(np.uint32)), name
            else:
                _invalid_arg(gpu_pkg, a.normals, sc)
        a.close()


def _pair(n, seed):
    a, b = ic.room_pair(n, 1.0, seed, walls=ic.UNIT_ROOM if n > 361 else rc.ROOM_BENCH)
    return a, b


def test_one_handle_at_changing_beam_counts(gpu_pkg):
    """The beam table, d_scans and d_stored are regrown (and shrunk in use) under one handle: match at 360 -> 4096 -> 3 -> 1080
    -> 360 beams, then reset + step at each count; a step at another count without a reset is refused and changes nothing."""
    a, p = _aligner(gpu_pkg, {})
    L = _laser(p)
    g = (0.015, 0.035, 0.015)
    for n in (360, 4096, 3, 1080, 360):
        s0, s1 = _pair(n, 300 + n)
        want = R.match(s0, s1, L, g)
        got = a.pclICP(g, s0, s1)
        _same(got, want, ("match", n))
        _same_run(a.pclICP(g, s0, s1), got, ("match again", n))
    NOT_RUN = gpu_pkg.capi.ICP_NOT_RUN
    prev = None
    for n in (360, 4096, 3, 1080, 360):
        s0, s1 = _pair(n, 400 + n)
        if prev is not None:    # another count without a reset: refused, the stored scan stays
            _invalid_arg(gpu_pkg, a.pclICPWrapper, g, s0)
            stored, nxt = prev
            _same(a.pclICPWrapper(g, nxt), R.match(stored, nxt, L, g), ("step after a refused step", n))
        a.reset()
        ok, T, info = a.pclICPWrapper(g, s0)
        assert ok and T == (0.0, 0.0, 0.0) and info["criterion"] == NOT_RUN
        want = R.match(s0, s1, L, g)
        _same(a.pclICPWrapper(g, s1), want, ("step", n))
        prev = (s1 if want.ok else s0, _pair(n, 500 + n)[1])
    a.close()
    # the same walk with the line metric, inside its limit
    b, p = _aligner(gpu_pkg, {}, "line")
    for n in (360, 2048, 3, 1080, 360):
        s0, s1 = _pair(n, 300 + n)
        got = b.pclICP(g, s0, s1)
        _same(got, LR.match(s0, s1, L, g), ("line match", n))
        _same_run(b.pclICP(g, s0, s1), got, ("line match again", n))
    b.close()


@pytest.mark.parametrize("n,n_scans", [(767, 24), (4096, 64)])
def test_step_batch_over_a_mixed_run(gpu_pkg, n, n_scans):
    """tbnav_icp_step_batch over a run that holds the tie pair, sparse, degenerate and all-invalid scans between ordinary ones:
    equal to one tbnav_icp_step per scan and to the restatement's wrapper; at 767 beams icp_align<PointMetric, 3> (two chains), at 4096
    beams icp_align<PointMetric, 16>, whose first launch runs 63 workgroups side by side."""
    kw, scans, T_init = ic.batch_run(n, n_scans)
    assert ic.beams_per_thread(n) == {767: 3, 4096: 16}[n]
    a, p = _aligner(gpu_pkg, kw)
    one = [a.pclICPWrapper(T_init[s], scans[s]) for s in range(n_scans)]
    b, _ = _aligner(gpu_pkg, kw)
    ok, T, info = b.wrapperBatch(T_init, scans)
    launches = b.lastBatchLaunches()
    for s in range(n_scans):
        assert bool(ok[s]) == one[s][0] and _bits(T[s]) == _bits(one[s][1]) and info[s] == one[s][2], s
    w = R.Wrapper(_laser(p))
    for s in range(n_scans):
        _same((bool(ok[s]), tuple(T[s]), info[s]), w.step(scans[s], T_init[s]), s)
    crit = [i["criterion"] for i in info]
    capi = gpu_pkg.capi
    assert crit[0] == capi.ICP_NOT_RUN and crit[14] == capi.ICP_DEGENERATE and info[14]["correspondences"] == 4
    assert [s for s in range(n_scans) if not ok[s]] == [5, 14, 20, 21]
    assert crit[5] == crit[20] == crit[21] == capi.ICP_NO_CORRESPONDENCES
    assert info[1]["correspondences"] == 361 and info[13]["correspondences"] == 3
    assert launches > 1, "a failure must realign the pairs that depended on it"
    b.reset()
    ok2, T2, info2 = b.wrapperBatch(T_init, scans)
    assert np.array_equal(ok, ok2) and np.array_equal(T.view(np.uint64), T2.view(np.uint64)) and info == info2
    a.close(); b.close()


def test_line_step_batch_over_a_mixed_run(gpu_pkg):
    """The same run at 767 beams through icp_align<LineMetric, 3>."""
    n, n_scans = 767, 24
    kw, scans, T_init = ic.batch_run(n, n_scans)
    a, p = _aligner(gpu_pkg, kw, "line")
    one = [a.pclICPWrapper(T_init[s], scans[s]) for s in range(n_scans)]
    b, _ = _aligner(gpu_pkg, kw, "line")
    ok, T, info = b.wrapperBatch(T_init, scans)
    w = LR.Wrapper(_laser(p))
    for s in range(n_scans):
        assert bool(ok[s]) == one[s][0] and _bits(T[s]) == _bits(one[s][1]) and info[s] == one[s][2], s
        _same((bool(ok[s]), tuple(T[s]), info[s]), w.step(scans[s], T_init[s]), s)
    assert 0 < int(ok.sum()) < n_scans
    b.reset()
    ok2, T2, info2 = b.wrapperBatch(T_init, scans)
    assert np.array_equal(ok, ok2) and np.array_equal(T.view(np.uint64), T2.view(np.uint64)) and info == info2
    a.close(); b.close()
