"""The cases of tests/icp_cases.py on the restatements alone (CPU): every case does what it is there for, so that the GPU tests
which hold the kernel to the restatements on these cases (test_icp_shapes_gpu.py) test what they claim to.  Every instantiation
of the two kernels is named by a beam count, every stop rule is reached, the correspondence counts and the distance gate sit
exactly on their edges, and on the tie cases a nearest-neighbour merge with the wrong tie-break gives another answer."""
import math

import numpy as np
import pytest

import icp_cases as ic
import icp_line_restatement as LR
import icp_restatement as R

ALL_CRITERIA = {R.ITERATIONS, R.TRANSFORM, R.ABS_MSE, R.REL_MSE, R.NO_CORRESPONDENCES, R.DEGENERATE}


@pytest.fixture(scope="module")
def criterion_results():
    return {(c.name, m): ic.restate(c, m) for c in ic.criterion_cases() for m in ("point", "line")}


@pytest.fixture(scope="module")
def edge_results():
    return {(c.name, m): ic.restate(c, m) for c in ic.edge_cases() for m in ("point", "line") if m == "point" or c.tgt.size <= LR.MAX_BEAMS}


def test_beam_counts_name_every_instantiation_at_both_edges_and_one_past():
    cases = ic.beam_count_cases()
    assert [c.tgt.size for c in cases] == list(ic.BEAM_COUNTS) and all(c.src.size == c.tgt.size for c in cases)
    point = {n: ic.beams_per_thread(n) for n in ic.BEAM_COUNTS}
    line = {n: ic.beams_per_thread(n, "line") for n in ic.BEAM_COUNTS if n <= LR.MAX_BEAMS}
    assert set(point.values()) == {1, 2, 3, 4, 6, 8, 12, 16}
    assert set(line.values()) == {1, 2, 3, 4, 6, 8}
    assert {ic.chains(P) for P in point.values()} == {1, 2, 4}
    for P in ic.POINT_P:   # at (or one under) the upper edge, and unless it is the limit, one past it: the next one's lower edge
        assert any(point.get(n) == P for n in (P * ic.B - 1, P * ic.B)), P
        if P * ic.B < ic.MAX_BEAMS:
            assert point[P * ic.B + 1] > P
    # the float4 padding: counts of every residue mod 4; the last register slot invalid in all threads but one / in one thread
    assert {n % 4 for n in ic.BEAM_COUNTS} == {0, 1, 2, 3}
    assert max(ic.BEAM_COUNTS) == ic.MAX_BEAMS


def test_every_stop_rule_is_reached_with_both_metrics(criterion_results):
    res = criterion_results
    assert {r.criterion for (name, m), r in res.items() if m == "point"} == ALL_CRITERIA
    assert {r.criterion for (name, m), r in res.items() if m == "line"} == ALL_CRITERIA
    for m in ("point", "line"):
        assert all(res[f"rel_mse_s{s}", m].criterion == R.REL_MSE for s in range(1, 6)), m
        both = [res[f"abs_mse_or_cycle_s{s}", m] for s in range(1, 6)]
        assert {r.criterion for r in both} == {R.ABS_MSE, R.ITERATIONS}, m
        assert all(r.iterations == 100 for r in both if r.criterion == R.ITERATIONS)
        # the carry prev = mse ran for many iterations before a rule fired
        assert max(r.iterations for r in both if r.criterion == R.ABS_MSE) > 20, m
        r = res["identical", m]
        assert (r.criterion, r.iterations, r.mse, r.T) == (R.TRANSFORM, 1, 0.0, (0.0, 0.0, 0.0)), (m, r)
        assert res["max_iter_2", m].iterations == 2 and res["max_iter_2", m].criterion == R.ITERATIONS
        assert res["default_s1", m].criterion == R.TRANSFORM
        assert res["empty_source", m].criterion == R.NO_CORRESPONDENCES
    long = [res[f"max_iter_{ic.MAX_ITER}_s{s}", "point"] for s in range(1, 6)]
    assert any(r.iterations == ic.MAX_ITER and r.criterion == R.ITERATIONS for r in long)
    assert any(100 < r.iterations < ic.MAX_ITER and r.criterion == R.ABS_MSE for r in long)
    assert any(100 < res[f"max_iter_{ic.MAX_ITER}_s{s}", "line"].iterations < ic.MAX_ITER for s in range(1, 6))
    r = res["degenerate_one_target_point", "point"]
    assert (r.ok, r.criterion, r.correspondences, r.iterations, r.T) == (False, R.DEGENERATE, 4, 1, (0.0, 0.0, 0.0)) and r.mse > 0.0
    r = res["corridor_without_noise", "line"]
    assert (r.ok, r.criterion, r.iterations) == (False, R.DEGENERATE, 1) and r.correspondences > 200


def test_correspondence_counts_and_the_distance_gate_sit_on_their_edges(edge_results):
    res = edge_results
    for m in ("point", "line"):
        r = res["corr_2", m]
        assert (r.ok, r.criterion, r.correspondences, r.iterations) == (False, R.NO_CORRESPONDENCES, 2, 1), (m, r)
        r = res["corr_3", m]
        assert r.ok and r.correspondences == 3, (m, r)
    r = res["max_corr_dist_at_one_iteration", "point"]
    assert (r.ok, r.criterion, r.correspondences) == (True, R.ITERATIONS, 3), r
    assert r.mse == 0.25 / 3.0   # the pair at exactly 0.5 m is in, the other two are exact
    r = res["max_corr_dist_above_one_iteration", "point"]
    assert (r.ok, r.criterion, r.correspondences) == (False, R.NO_CORRESPONDENCES, 2), r
    assert res["max_corr_dist_at", "point"].ok and not res["max_corr_dist_above", "point"].ok
    cases = {c.name: c for c in ic.edge_cases()}
    at, above = cases["max_corr_dist_at"], cases["max_corr_dist_above"]
    assert float(above.src[0]) - float(at.src[0]) == 2.0 ** -23 and np.array_equal(at.src[1:], above.src[1:], equal_nan=True)


def test_sparse_scans_are_sparse_and_the_bunched_ones_sit_in_a_few_threads(edge_results):
    seen = 0
    for c in ic.edge_cases():
        if not c.name.startswith("sparse_"):
            continue
        seen += 1
        n = c.tgt.size
        frac = int(c.name.split("_")[2][:-3]) / 100.0
        valid = np.flatnonzero(~np.isnan(c.src))
        assert np.array_equal(np.isnan(c.src), np.isnan(c.tgt))
        threads = np.unique(valid % ic.B).size
        if c.name.endswith("bunched"):
            assert threads == max(1, round(frac * ic.B)), (c.name, threads)
            assert valid.size > threads                           # more than one beam in a thread: the per-thread order counts
        else:
            assert valid.size == max(1, round(frac * n)), (c.name, valid.size)
            assert threads > min(valid.size, ic.B) // 2, (c.name, threads)
        assert edge_results[c.name, "point"].ok, c.name           # they align: the sums run, not only the first gate
    assert seen == 12


def test_special_guesses_are_evaluated_and_fail_or_converge_as_the_contract_says(edge_results):
    for slot in "txy":
        for name, v in ic.T_SPECIALS:
            for m in ("point", "line"):
                r = edge_results[f"guess_{slot}_{name}", m]
                if slot == "t" and math.isfinite(v):
                    assert r.ok, (slot, name, m, r)                       # cos / sin of a huge angle are numbers
                else:
                    assert (r.ok, r.criterion, r.iterations, r.correspondences, r.T) == (False, R.NO_CORRESPONDENCES, 1, 0, (0.0, 0.0, 0.0)), (slot, name, m, r)
    with np.errstate(over="ignore"):
        assert math.isinf(float(np.float32(1e39))) and math.isfinite(float(np.float32(1e30)))
    assert math.isnan(ic.ref_guess((math.inf, 1.0, 2.0))[0]) and ic.ref_guess((0.5, math.inf, 2.0)) == (0.5, math.inf, 2.0)


def test_edge_lasers_take_the_other_branches(edge_results):
    cases = {c.name: c for c in ic.edge_cases()}
    c = cases["negative_delta_and_beam_max"]
    L = ic.laser(c.kw)
    assert L.beam_max < 0.0 and L.beam_delta < 0.0
    W = ic.wrap_period(L, c.tgt.size)
    assert 355 <= W < c.tgt.size, W                                      # the beam_max < 0 wrap is taken inside the scan
    pos = R.beam_table(R.lds01(), c.tgt.size)
    neg = R.beam_table(L, c.tgt.size)
    assert np.array_equal(neg[1:W, 0], pos[1:W, 0]) and np.array_equal(neg[1:W, 1], -pos[1:W, 1])
    c = cases["beam_min_minus_pi_and_Trs"]
    L = ic.laser(c.kw)
    assert L.beam_min == float(np.float32(-math.pi)) and R.beam_table(L, 360)[0, 0] == np.float32(-1.0)
    for name in ("negative_delta_and_beam_max", "beam_min_minus_pi_and_Trs"):
        for m in ("point", "line"):
            r = edge_results[name, m]
            assert r.ok and np.allclose(r.T, (0.02, 0.04, 0.01), atol=0.02), (name, m, r)   # the scans fit the laser: a true alignment
    c = cases["range_bounds"]
    pts, beam = R.cloud(c.tgt, ic.laser(c.kw))
    assert 3 in beam and 200 in beam and 50 not in beam and 120 not in beam   # range_min is in, range_max is out
    assert c.tgt[3] == np.float32(0.12) and c.tgt[120] == np.float32(3.5)


# ---- ties ----

def _first(d, tgt_beam, C):
    return np.argmin(d, axis=1)


def _last_of_equal_minima(d, tgt_beam, C):
    return d.shape[1] - 1 - np.argmin(d[:, ::-1], axis=1)


def _lower_chain_first(d, tgt_beam, C):
    """what merging the chains' minima by distance alone gives: among equal minima the one in the lowest chain"""
    with np.errstate(invalid="ignore"):
        eq = d == np.min(d, axis=1)[:, None]
    key = (tgt_beam % C) * (1 << 20) + tgt_beam
    return np.argmin(np.where(eq, key[None, :], 1 << 40), axis=1)


def _match_with(pick, case, C):
    """icp_restatement.match_clouds with the argmin step handed in (a local copy: the restatement itself has no switch)."""
    L = ic.laser(case.kw)
    tgt, tgt_beam = R.cloud(case.tgt, L)
    src, src_beam = R.cloud(case.src, L)
    n_beams, B, T_init = case.src.size, ic.B, case.T
    max_iter, max_corr_dist, transform_eps, fitness_eps = 100, 0.5, 1e-8, 1e-6
    c0, s0 = float(R.F32(math.cos(T_init[0]))), float(R.F32(math.sin(T_init[0])))
    Rm = [[c0, -s0], [s0, c0]]
    t = [float(R.F32(T_init[1])), float(R.F32(T_init[2]))]
    max2 = max_corr_dist * max_corr_dist
    prev = R.DBL_MAX
    sx, sy = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64)
    thread, rnd = src_beam % B, src_beam // B
    rounds = (n_beams + B - 1) // B
    k = 0
    while True:
        k += 1
        ax = (((Rm[0][0] * sx) + (Rm[0][1] * sy)) + t[0]).astype(np.float32)
        ay = (((Rm[1][0] * sx) + (Rm[1][1] * sy)) + t[1]).astype(np.float32)
        dx = ax[:, None] - tgt[None, :, 0]
        dy = ay[:, None] - tgt[None, :, 1]
        d = dx * dx + dy * dy
        j = pick(d, tgt_beam, C)
        dmin = d[np.arange(d.shape[0]), j]
        keep = dmin.astype(np.float64) <= max2
        n = int(keep.sum())
        if n < 3:
            return R.Result(False, (0.0, 0.0, 0.0), k, n, 0.0, R.NO_CORRESPONDENCES)
        a64x, a64y = ax.astype(np.float64), ay.astype(np.float64)
        b64x, b64y = tgt[j, 0].astype(np.float64), tgt[j, 1].astype(np.float64)
        vals = [a64x, a64y, b64x, b64y, a64x * b64x, a64y * b64y, a64x * b64y, a64y * b64x, dmin.astype(np.float64)]
        tot = []
        for v in vals:
            partial = np.zeros(B)
            for q in range(rounds):
                sel = keep & (rnd == q)
                partial[thread[sel]] = partial[thread[sel]] + v[sel]
            tot.append(R._tree_sum(partial))
        Sax, Say, Sbx, Sby, Sxx, Syy, Sxy, Syx, Sd = tot
        dn = float(n)
        A = (Sxx + Syy) - ((Sax * Sbx) + (Say * Sby)) / dn
        S = (Sxy - Syx) - ((Sax * Sby) - (Say * Sbx)) / dn
        r = math.sqrt((A * A) + (S * S))
        mse = Sd / dn
        if r == 0.0:
            return R.Result(False, (0.0, 0.0, 0.0), k, n, mse, R.DEGENERATE)
        c, s = A / r, S / r
        amx, amy, bmx, bmy = Sax / dn, Say / dn, Sbx / dn, Sby / dn
        tix = bmx - ((c * amx) - (s * amy))
        tiy = bmy - ((s * amx) + (c * amy))
        Rm = [[(c * Rm[0][0]) - (s * Rm[1][0]), (c * Rm[0][1]) - (s * Rm[1][1])],
              [(s * Rm[0][0]) + (c * Rm[1][0]), (s * Rm[0][1]) + (c * Rm[1][1])]]
        t = [((c * t[0]) - (s * t[1])) + tix, ((s * t[0]) + (c * t[1])) + tiy]
        crit = None
        if k >= max_iter:
            crit = R.ITERATIONS
        elif c >= 1.0 - transform_eps and ((tix * tix) + (tiy * tiy)) <= transform_eps:
            crit = R.TRANSFORM
        else:
            dm = abs(mse - prev)
            if dm < 1e-12:
                crit = R.ABS_MSE
            elif dm / prev < fitness_eps:
                crit = R.REL_MSE
        if crit is not None:
            return R.Result(True, (math.atan2(Rm[1][0], Rm[0][0]), t[0], t[1]), k, n, mse, crit)
        prev = mse


@pytest.mark.parametrize("case", ic.tie_cases(), ids=lambda c: c.name)
def test_tie_cases_hold_ties_and_a_wrong_tie_break_changes_the_answer(case):
    n = case.tgt.size
    P = ic.beams_per_thread(n)
    C = ic.chains(P)
    assert (P, C) == {405: (2, 4), 767: (3, 2), 1023: (4, 2), 1083: (6, 1)}[n]
    tied, wrong_chain = ic.count_ties(case, C)
    print(case.name, "P", P, "C", C, "tied source points", tied, "lowest index not in the lowest chain", wrong_chain)
    assert tied >= 10, tied
    true = ic.restate(case)
    assert true.ok
    copy = _match_with(_first, case, C)
    assert copy == true                                   # the local copy is the restatement, bit for bit
    last = _match_with(_last_of_equal_minima, case, C)
    assert tuple(last.T) != tuple(true.T)
    assert max(abs(a - b) for a, b in zip(last.T, true.T)) > 1e-3, (last.T, true.T)
    if C > 1:
        assert wrong_chain >= 5, wrong_chain
        chain = _match_with(_lower_chain_first, case, C)
        assert tuple(chain.T) != tuple(true.T)
        assert max(abs(a - b) for a, b in zip(chain.T, true.T)) > 1e-3, (chain.T, true.T)
    else:
        assert _match_with(_lower_chain_first, case, C) == true   # one chain: nothing to merge, the control


def test_the_local_copy_is_the_restatement_on_ordinary_cases_too(criterion_results):
    for c in ic.criterion_cases():
        if not c.kw:
            assert _match_with(_first, c, 4) == criterion_results[c.name, "point"], c.name


def test_every_case_has_a_name_of_its_own_and_scans_of_one_size():
    cases = ic.all_cases()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert c.tgt.dtype == c.src.dtype == np.float32 and c.tgt.shape == c.src.shape and 1 <= c.tgt.size <= ic.MAX_BEAMS, c.name
        assert len(c.T) == 3


def test_create_refuses_a_distance_gate_whose_square_is_not_finite(pkg):
    """Found while reading the kernel for these cases: a source point with no nearest target (an empty target cloud, a NaN guess)
    stays at distance +inf with the index 0x7fffffff, and '(double)d <= max_corr_dist^2' let it through as a pair when the gate
    itself was +inf: an out-of-range LDS read.  tbnav_icp_create now refuses such a gate, before it looks for a device."""
    import ctypes as C
    c = pkg.capi
    L = c.lib()
    for bad in (math.inf, 1e200, 1.4e154, math.nan, 0.0, -0.5):
        p = c.IcpParams()
        L.tbnav_icp_default_params(C.byref(p))
        p.max_corr_dist = bad
        h = C.c_void_p()
        assert L.tbnav_icp_create(C.byref(p), C.byref(h)) == c.ERR_INVALID_ARG, bad
        assert not h.value
    for good in (0.5, 1e150):
        p = c.IcpParams()
        L.tbnav_icp_default_params(C.byref(p))
        p.max_corr_dist = good
        h = C.c_void_p()
        rc = L.tbnav_icp_create(C.byref(p), C.byref(h))
        assert rc != c.ERR_INVALID_ARG, good      # accepted: what follows depends on there being a device
        if rc == c.OK:
            L.tbnav_icp_destroy(h)
