"""The resampling case table (tests/resample_cases.py) on the CPU: with the host's sequential routine (rtn_amd.rbpf.resample_global)
and, where it applies, the oracle filter, every case reaches what it names — both decisions at every N that can resample, the clamp
at N - 1, runs of parent 0, children of 0, 1 and more, runs that straddle the chunk border — the restated literals are the
sources', and the restated arg-max is the oracle's best().  No device."""
import os

import numpy as np
import pytest

import oracle_api as orc
import resample_cases as rsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "csrc")


@pytest.fixture(scope="module")
def table(pkg):
    """(N, shape, z) -> (prior, parents, normalised weights, stats, running sums) by the host routine, once for the whole file."""
    from rtn_amd.rbpf import resample_global
    out = {}
    for N in rsc.SIZES:
        for shape, w, z in rsc.normalise_runs(N):
            parents, wn, st = resample_global(w, z)
            out[(N, shape, z)] = (w, parents, wn, st, np.cumsum(wn))
    return out


def test_the_restated_literals_are_the_sources():
    read = lambda name: open(os.path.join(CSRC, name)).read()
    for src, pieces in ((read("rbpf_plan.hpp"), ("constexpr int kNormChunk = 2048;",)),
                        (read("rbpf_device.hpp"), ("constexpr int kResampleThreads = 1024;", "constexpr int kTS = 32, kTSh = 5,")),
                        (read("rbpf_normalize.hpp"), ("const int neff = (int)(1.0 / sq);", "const int res = (neff < (N / 2)) ? 1 : 0;",
                                                      "constexpr int kSeqBlk = NTHR == 256 ? 32 : 16;", "const bool one_chunk = N <= kNormChunk;",
                                                      "const bool plain = one_chunk || !PAR;", "int lo = 0, hi = N - 1;",
                                                      "const double U = r + (double)(m * (1.0 / (N - 1)));", "int lo = m, hi = N;")),
                        (read("rbpf_raycast.hip"), ("normalize_body<NT, false>(nz.N,",)),
                        (read("rbpf_resample.hip"), ("normalize_body<256, true>(N,", "__launch_bounds__(256) void rbpf_argmax(",
                                                     "if (w > bv) { bv = w; bi = i; }",
                                                     "if (ov > sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi < si[threadIdx.x]))")),
                        (read("rbpf_batch.hip"), ("out->neff = static_cast<int>(1.0 / sq);", "out->resampled = (out->neff < (N / 2)) ? 1 : 0;")),
                        (read("rbpf.hip"), ("const bool overlap = !local_only && !h->timing;",
                                            "TBNAV_TRY(launch_raycast(h, c, h->N, h->d_sens, overlap ? &nz : nullptr, d_err, beams_dev));",
                                            "if (!local_only && !overlap)   // (no gate, no flag: see above)\n    TBNAV_TRY(launch_normalize(h, NormArgs{",
                                            "p.grid = count + (p.box() && nz ? 1 : 0);",
                                            "return nz ? launch_normalize(h, *nz) : TBNAV_OK;",
                                            "const int blocks = (int)std::min<size_t>((n + kResampleThreads - 1) / kResampleThreads, 8192);",
                                            "const int chunks = (int)std::min<size_t>(std::max<size_t>(work / 2048, 1), 64);")),
                        (read("rbpf_api.hip"), ('"rbpf_raycast_box<%d, %d, %s, %d>"', 'snprintf(raycast, (size_t)raycast_cap, "rbpf_raycast");',
                                                "hipLaunchKernelGGL(rbpf_argmax, dim3(1), dim3(256),"))):
        for piece in pieces:
            assert piece in src, (f"the source no longer writes `{piece}`: if the rule changed, change its restatement in tests/resample_cases.py "
                                  "with it; if only its spelling changed, update this list")
    assert rsc.K_NORM_CHUNK == 2048 and rsc.K_RESAMPLE_THREADS == 1024 and rsc.ARGMAX_THREADS == 256
    # the sizes sit on both sides of every block the code works in
    for blk in (16, 32, 256, rsc.K_NORM_CHUNK):
        assert {blk - 1, blk, blk + 1} <= set(rsc.SIZES)
    assert 2 * rsc.K_NORM_CHUNK + 1 in rsc.SIZES
    assert [rsc.normalise_home(f)[0] for f in rsc.FORMS] == ["rbpf_raycast_box", "rbpf_raycast_box", "rbpf_normalize", "rbpf_normalize"]
    assert [rsc.normalise_home(f)[2] for f in rsc.FORMS] == [1, 1, 0, 0]
    assert rsc.chunks(2048) == 1 and rsc.chunks(2049) == 2 and rsc.chunks(4097) == 3
    # the one run whose table loop makes a second trip: 400 x 400 cells are 13 x 13 tiles
    TT = ((400 + 31) // 32) ** 2
    n2 = rsc.smallest_n_with_two_trips(TT)
    assert TT == 169 and n2 == 49637 and rsc.table_trips(n2, TT) == 2 and rsc.table_trips(n2 - 1, TT) == 1


def test_the_decision_rule_is_the_host_s_and_both_decisions_occur_from_4_particles_on(table):
    for N in rsc.SIZES:
        seen = set()
        for (n, shape, z), (w, parents, wn, st, cs) in table.items():
            if n != N:
                continue
            assert rsc.decision(st.sq_sum, N) == (st.neff, st.resampled), (N, shape, z)
            seen.add(st.resampled)
            if not st.resampled:
                assert np.array_equal(parents, np.arange(N))
        assert seen == ({0, 1} if rsc.can_resample(N) else {0}), (N, seen)
    assert [N for N in rsc.SIZES if not rsc.can_resample(N)] == [1, 2, 3]


def test_every_shape_does_what_it_is_there_for(table):
    for N in rsc.SIZES:
        if not rsc.can_resample(N):
            continue
        at = lambda shape, z: table[(N, shape, z)]
        res = {key[1:]: v for key, v in table.items() if key[0] == N and v[3].resampled}
        # the clamp: some slot's U lies beyond the last running sum
        w, parents, wn, st, cs = at("dominant-0", 2.5)
        U = 2.5 / N + np.arange(N) * (1.0 / (N - 1))
        assert st.resampled and U[-1] > 1.0 + 1e-6 > cs[-1] and parents[-1] == N - 1
        w, parents, wn, st, cs = at("last", 0.3)
        assert st.resampled and set(parents.tolist()) == {N - 1}
        # z = -2.5: a run of parent 0 longer than 1
        assert any(z == -2.5 and (p[:2] == 0).all() for (shape, z), (w, p, wn, st, cs) in res.items()), N
        # children: 0, 1 and more, somewhere at this N
        kids = set()
        for (shape, z), (w, p, wn, st, cs) in res.items():
            kids |= set(np.minimum(np.bincount(p, minlength=N), 2).tolist())
        assert kids == {0, 1, 2}, (N, kids)
        # the dominant weights' slots: the whole comb but its ends falls on one parent
        for shape, j in (("dominant-0", 0), ("dominant-third", N // 3), ("dominant-last", N - 1)):
            w, parents, wn, st, cs = at(shape, 0.3)
            assert st.resampled and np.bincount(parents, minlength=N)[j] >= N - 2, (N, shape)
        assert (rsc.prior("every-once", N) is not None) == (N >= rsc.EVERY_ONCE_MIN_N and N % 2 == 0)
        if rsc.prior("every-once", N) is not None:
            w, parents, wn, st, cs = at("every-once", 0.0)
            assert st.resampled and np.array_equal(parents, np.arange(N)), N     # resampled, and children == 1 everywhere
            assert (w > 0).all() and st.neff == N // 2 - 1
        # half the weights are exactly zero, and no slot chooses a zero weight's particle (a running sum that does not move cannot be
        # the first to reach U) — but for the slots clamped at N - 1, whatever its weight
        w, parents, wn, st, cs = at("half-zero", 0.3)
        assert (w == 0.0).sum() >= 1 and (N < 16 or abs((w == 0.0).mean() - 0.5) < 0.3)
        assert (st.resampled or N < 16) and (not st.resampled or (wn[parents[parents < N - 1]] > 0.0).all()), N
        if N > rsc.K_NORM_CHUNK:      # a run of equal parents across the chunk border
            b = rsc.K_NORM_CHUNK
            assert sum(1 for (shape, z), (w, p, wn, st, cs) in res.items() if p[b - 1] == p[b]) >= 3, N
            w, parents, wn, st, cs = at("dominant-third", -2.5)      # (at 2049 slot 2048 is the last: a positive z clamps it to N - 1)
            assert st.resampled and parents[b - 1] == parents[b] == N // 3
    # lognormal: 20 orders of magnitude
    w = rsc.prior("lognormal", 4097)
    assert w.max() / w.min() > 1e20
    # dyadic: every partial sum is exact, so every add is a tie candidate of the parallel chains
    w = rsc.prior("dyadic", 4097)
    assert float(np.sum(w)) == float(sum(int(v * 2.0 ** 40) for v in w)) / 2.0 ** 40


def test_the_host_routine_equals_the_oracle_filter_on_the_table_s_shapes(pkg):
    """tests/test_sharded_gloo.py's comparison on this table: normalizeWeights / effectiveParticles / lowVarianceResampling of the
    oracle filter, driven through one scan whose beams are all out of range (the maps stay empty)."""
    from rtn_amd.rbpf import resample_global
    checked = 0
    for N in (4, 5, 15, 16, 17, 33):
        for shape, w, z in rsc.normalise_runs(N):
            pf = orc.PfAPI(orc.pf_params(N=N, k=4, map_min=-0.5, map_max=0.5))
            pf.set_particles(w=w)
            nz = np.tile(orc.normal_stream(5, 3 * 4 + 3, 0.0, 1.0), N).tolist() + [z]
            tr = pf.slam(np.full(360, 9.0, dtype=np.float32), (0, 0.05, 0), (0.0, 0.05, 0.0), (0, 0, 0), True, (0.0, 0.05, 0.0), nz)
            assert tr["rc"] == 0
            parents, wn, st = resample_global(tr["weight_raw"], z)
            assert (st.sum_w, st.sq_sum, st.neff, st.resampled) == (tr["sum_w"], tr["sq_sum"], tr["neff"], tr["resampled"]), (N, shape, z)
            if st.resampled:
                assert np.array_equal(parents, tr["resample_idx"]), (N, shape, z)
                assert np.array_equal(wn[parents], pf.particles()[2])
                checked += 1
            pf.close()
    assert checked >= 40


def test_the_parent_lists_hold_what_they_name():
    for N in (6, 7, 40):
        lists = rsc.parent_lists(N)
        p, kids = rsc.resolve(lists["identity"])
        assert np.array_equal(p, np.arange(N)) and (kids == 1).all()
        assert rsc.resolve(lists["all-to-0"])[1][0] == N and rsc.resolve(lists["all-to-last"])[1][N - 1] == N
        p, kids = rsc.resolve(lists["reversal"])
        assert np.array_equal(p, np.arange(N)[::-1]) and (kids == 1).all()
        p, kids = rsc.resolve(lists["counts"])
        assert (kids[2], kids[0], kids[1]) == (N - 3, 2, 1) and (kids[3:] == 0).all() and (np.diff(p) < 0).any()     # (not sorted)
        p, kids = rsc.resolve(lists["keep"])
        assert (lists["keep"] == -1).sum() >= 3 and p[0] == 0 and p[1] == 0 and p[3] == 2 and kids[0] == 2 and kids[1] == 0
        for name, l in lists.items():
            assert l.dtype == np.int32 and l.size == N and l.min() >= -1 and l.max() < N, name


def test_the_restated_arg_max_is_the_oracle_s_best():
    for N in rsc.ARGMAX_SIZES:
        pf = orc.PfAPI(orc.pf_params(N=N, k=4, map_min=-0.5, map_max=0.5))
        cases = rsc.argmax_cases(N)
        assert {"only-last", "zeros", "denormal"} <= set(cases)
        for name, w in cases.items():
            pf.set_particles(w=w)
            want = rsc.argmax_restated(w)
            assert pf.best() == want, (N, name)
            mx = np.flatnonzero(w == w.max())
            assert want == (int(mx[0]) if w.max() > 0.0 else 0)
            if name in ("cross", "cross-3"):       # the lowest index among the maxima sits in a higher thread than another maximum
                assert len(mx) >= 2 and mx[0] % rsc.ARGMAX_THREADS > min(m % rsc.ARGMAX_THREADS for m in mx[1:]), (N, name)
            if name == "stride":
                assert len(mx) == 2 and mx[0] % rsc.ARGMAX_THREADS == mx[1] % rsc.ARGMAX_THREADS
            if name == "denormal":
                assert w.max() == 5e-324 and want == N // 2
        assert ("cross" in cases) == (N > rsc.ARGMAX_THREADS)
        pf.close()
