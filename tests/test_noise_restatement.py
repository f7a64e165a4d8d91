"""noise_restatement.py held to outside facts, and noise_cases.py shown to be sharp (no GPU):
  * Philox4x32-10 against the three known-answer vectors of the Random123 distribution, in both forms;
  * the uniforms' ranges and what the top and bottom inputs give: no input gives a NaN or an infinity;
  * the counter spaces the headers promise: ticks, shards and scans never share a counter;
  * the longdouble Box-Muller against mpmath at 200 bits (2^-60 relative);
  * the restated streams against the normal law (Kolmogorov-Smirnov at the 1 % level on 2^20 values per sampler);
  * every mutation of noise_restatement.MUTATIONS changes the restated values of at least one table row.
"""
import math

import numpy as np
import pytest

import noise_cases as nc
import noise_restatement as nr

LD = np.longdouble
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
TOP = 0xFFFFFFFF


def test_philox_known_answers_in_both_forms():
    for ctr, key, want in KAT:
        assert nr.philox4x32_10(ctr, key) == want
        assert tuple(int(w) for w in nr.philox4x32_10_vec(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))) == want
    assert nr.philox4x32_10(KAT[0][0], KAT[0][1], rounds=9) != KAT[0][2]


def test_vectorised_philox_equals_the_integer_form():
    rng = np.random.default_rng(1)
    c = rng.integers(0, 2 ** 32, size=(10000, 4), dtype=np.uint64)
    k = rng.integers(0, 2 ** 32, size=(10000, 2), dtype=np.uint64)
    got = nr.philox4x32_10_vec(c, k)
    want = np.array([nr.philox4x32_10(c[j], k[j]) for j in range(len(c))], dtype=np.uint64)
    assert np.array_equal(got, want)
    # the device's words of a 64-bit counter and seed: (low, high, 0, 0), (low, high)
    ctr, seed = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    assert tuple(int(w) for w in nr.device_words([ctr], seed)[0]) == nr.philox4x32_10((0x89ABCDEF, 0x01234567, 0, 0), (0x76543210, 0xFEDCBA98))


def test_pi_parts():
    import mpmath
    with mpmath.workprec(300):
        hi = mpmath.mpf(int(nr.PI_HI * LD(2) ** 62)) / mpmath.mpf(2) ** 62
        assert int(nr.PI_HI * LD(2) ** 62) == 0xC90FDAA22168C234
        lo = mpmath.mpf(int(nr.PI_LO * LD(2) ** 126)) / mpmath.mpf(2) ** 126
        assert abs(hi + lo - mpmath.pi) < mpmath.mpf(2) ** -126


def _words(r0, r1, r2, r3):
    return np.array([[r0, r1, r2, r3]], dtype=np.uint64)


EDGE_WORDS = [0, 1, 0xFF, 0x100, 0xFFF, 0x1000, 0x7FFFFFFF, 0x80000000, 0x800000FF, 0xFFFFF000, 0xFFFFF7FF, 0xFFFFF800, 0xFFFFFF00, TOP]


def test_uniform_ranges_and_edge_values():
    # MPPI wide: [2^-53, 1 - 2^-53], never 0 or 1
    lo, hi = nr.uniforms_wide(_words(0, 0, 0, 0)), nr.uniforms_wide(_words(TOP, TOP, TOP, TOP))
    assert lo[0][0] == lo[1][0] == 2.0 ** -53 and hi[0][0] == hi[1][0] == 1.0 - 2.0 ** -53
    # narrow and RBPF: (0, 1], exactly 1.0 at the top input (the half is lost to rounding from 2^23 / 2^52 on)
    lo, hi = nr.uniforms_narrow(_words(0, 0, 0, 0)), nr.uniforms_narrow(_words(TOP, TOP, 0, 0))
    assert lo[0][0] == lo[1][0] == np.float32(2.0 ** -25) and hi[0][0] == hi[1][0] == np.float32(1.0)
    assert nr.uniforms_narrow(_words(0x7FFFFF00, 0x80000000, 0, 0))[0][0] == np.float32((2 ** 23 - 0.5) * 2.0 ** -24)  # the last input that keeps its half
    assert nr.uniforms_narrow(_words(0x80000100, 0, 0, 0))[0][0] == np.float32((2 ** 23 + 2) * 2.0 ** -24)            # 2^23 + 1.5 rounds to even
    lo, hi = nr.uniforms_rbpf(_words(0, 0, 0, 0)), nr.uniforms_rbpf(_words(TOP, TOP, TOP, TOP))
    assert lo[0][0] == lo[1][0] == 2.0 ** -54 and hi[0][0] == hi[1][0] == 1.0
    assert nr.uniforms_rbpf(_words(0x7FFFFFFF, TOP, 0, 0))[0][0] == (2.0 ** 52 - 0.5) * 2.0 ** -53
    # a pair of zeros at the top input of those two, and nothing else there
    for uni in (nr.uniforms_narrow, nr.uniforms_rbpf):
        a, b = nr.box_muller(*uni(_words(TOP, TOP, TOP, TOP)))
        assert a[0] == 0 and b[0] == 0
    # no input gives a NaN or an infinity: every combination of edge words in all four places
    g = np.array(np.meshgrid(EDGE_WORDS, EDGE_WORDS, EDGE_WORDS, EDGE_WORDS, indexing="ij"), dtype=np.uint64).reshape(4, -1).T
    for uni in (nr.uniforms_wide, nr.uniforms_narrow, nr.uniforms_rbpf):
        u1, u2 = uni(g)
        assert np.all(u1 > 0) and np.all(u1 <= 1) and np.all(u2 > 0) and np.all(u2 <= 1)
        a, b = nr.box_muller(u1, u2)
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
        if uni is nr.uniforms_wide:
            assert np.all(u1 < 1) and np.all(u2 < 1)
    # the largest magnitudes: the smallest u1, at an angle where the cosine is 1 to rounding
    for uni, w, sigma in ((nr.uniforms_wide, _words(0, 0, 0, 0), 8.57), (nr.uniforms_rbpf, _words(0, 0, 0, 0), 8.65),
                          (nr.uniforms_narrow, _words(0, 0, 0, 0), 5.89)):
        a, b = nr.box_muller(*uni(w))
        rad = float(np.hypot(a[0], b[0]))
        assert abs(rad - sigma) < 0.005, (uni.__name__, rad)
        assert abs(float(a[0])) > rad * (1 - 1e-6)
    assert abs(math.sqrt(2 * 53 * math.log(2)) - 8.57) < 0.005 and abs(math.sqrt(2 * 54 * math.log(2)) - 8.65) < 0.005
    assert abs(math.sqrt(2 * 25 * math.log(2)) - 5.89) < 0.005


def test_exact_angle_reduction_at_the_quarter_turns():
    x = np.array([0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0])
    sn, cs = nr.sincos_turns(x)
    h = LD(0.5) ** LD(0.5)
    want_s = [0, h, 1, h, 0, -h, -1, -h, 0]
    want_c = [1, h, 0, -h, -1, -h, 0, h, 1]
    assert np.all(np.abs(sn - np.array(want_s, dtype=LD)) <= 2 * np.finfo(LD).eps)
    assert np.all(np.abs(cs - np.array(want_c, dtype=LD)) <= 2 * np.finfo(LD).eps)
    assert sn[0] == 0 and sn[4] == 0 and sn[8] == 0 and cs[2] == 0 and cs[6] == 0   # exact zeros at the axes
    # next to the zero of the cosine the result keeps its full relative precision
    import mpmath
    for u in (0.25 + 2.0 ** -53, 0.25 - 2.0 ** -54, 0.75 + 2.0 ** -52):
        _, c = nr.sincos_turns(np.array([u]))
        with mpmath.workprec(200):
            want = mpmath.cospi(2 * mpmath.mpf(u))
            assert abs(_ld_to_mp(c[0]) / want - 1) < mpmath.mpf(2) ** -60


def _ld_to_mp(v):
    import mpmath
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - LD(hi)))   # a 64-bit significand is two doubles exactly


def test_longdouble_box_muller_against_mpmath_at_200_bits():
    """A sample of each construction's draws, with the smallest and the largest results of a larger one and the edge uniforms among
    them: 2^-60 relative (the longdouble steps leave about 2e-19, a factor of 4 below)."""
    import mpmath
    rng = np.random.default_rng(5)
    words = rng.integers(0, 2 ** 32, size=(60000, 4), dtype=np.uint64)
    worst = 0.0
    for uni in (nr.uniforms_wide, nr.uniforms_narrow, nr.uniforms_rbpf):
        u1, u2 = uni(words)
        a, b = nr.box_muller(u1, u2)
        order = np.argsort(np.minimum(np.abs(a), np.abs(b)).astype(np.float64))
        big = np.argsort(np.maximum(np.abs(a), np.abs(b)).astype(np.float64))
        pick = np.unique(np.r_[order[:100], big[-50:], np.arange(350)])
        e1, e2 = uni(np.array([[0, 0, 0x3FFFFFFF, TOP], [TOP, 0xFFFFF000, 0x40000000, 0x00001000], [0, 0, 0xBFFFFFFF, TOP - 0x1000],
                               [TOP, 0xFFFFEFFF, 0xC0000000, 0x00000100]], dtype=np.uint64))   # u1 at both ends, u2 next to the cosine's zeros
        U1, U2 = np.r_[u1[pick], e1], np.r_[u2[pick], e2]
        A, B = nr.box_muller(U1, U2)
        for j in range(len(U1)):
            wa, wb = nr.box_muller_mp(U1[j], U2[j])
            with mpmath.workprec(200):
                for got, want in ((A[j], wa), (B[j], wb)):
                    if want == 0:
                        assert got == 0
                        continue
                    worst = max(worst, float(abs(_ld_to_mp(got) / want - 1)))
    print(f"[noise restatement] longdouble Box-Muller against mpmath, worst relative error {worst:.3g}")
    assert worst < 2.0 ** -60


# ---- counter spaces --------------------------------------------------------------------------------------------------------------
def _interval(row, tick, shard):
    """The counters of one handle's tick as a half-open interval, after checking on the array that they ARE one."""
    first, kg = shard if shard is not None else (0, row.K)
    lo = nr.mppi_counter(tick, row.T, kg, first, 0, 0)
    return lo, lo + row.K * row.T


@pytest.mark.parametrize("shape", nc.MPPI_SHAPES + [nc.MPPI_LARGE], ids=lambda s: f"K{s[0]}-T{s[1]}")
def test_mppi_counters_of_ticks_and_shards_are_disjoint_and_contiguous(shape):
    K, T = shape
    rows = [r for r in nc.MPPI_ROWS if (r.K, r.T) == shape]
    assert rows
    # k*T + i runs through 0 .. K*T - 1 once: a handle's counters of a tick are one interval
    c = nr.mppi_counters(0, T, K)
    assert np.array_equal(np.sort(c.ravel()), np.arange(K * T, dtype=np.uint64))
    assert int(c[T - 1, K - 1]) == nr.mppi_counter(0, T, K, 0, K - 1, T - 1) == K * T - 1
    for row in rows:
        kg = row.shard[1] if row.shard else K
        assert kg % K == 0
        firsts = list(range(0, kg, K))
        spans = []
        for tick in (row.tick, row.tick + 1):
            for f in firsts:                       # all shards of the ensemble, in order
                spans.append(_interval(row, tick, (f, kg)))
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
            assert a1 == b0                        # disjoint and together contiguous: shard after shard, tick after tick
        assert spans[0][0] == row.tick * T * kg and spans[-1][1] == (row.tick + 2) * T * kg < 2 ** 64
        lo, hi = _interval(row, row.tick, row.shard)   # the row's own shard lies inside its tick
        assert row.tick * T * kg <= lo and hi <= (row.tick + 1) * T * kg
        got = nr.mppi_counters(row.tick, T, K, *(row.shard or (0, K)))
        assert int(got.min()) == lo and int(got.max()) == hi - 1


def test_rbpf_scans_never_share_a_counter():
    # the largest ensemble the C-ABI accepts: 2^24 particles, 646 samples
    assert 2 ** 24 * (3 * 646 + 3) + 1 < 2 ** 41         # elements: pairs stay below 2^40, the next scan's first counter
    for row in nc.RBPF_ROWS:
        seen = {}
        for s, (seed, scan) in enumerate(nc.rbpf_schedule(row)):
            g = nr.rbpf_elements(row.N, nc.rbpf_stride(row, s), row.shard)
            ctr = {nr.rbpf_counter(scan, int(p)) for p in np.unique(g >> np.uint64(1))}
            assert all(nr.rbpf_counter(scan, 0) <= v < nr.rbpf_counter(scan + 1, 0) for v in ctr)
            for (seed0, scan0), other in seen.items():
                if seed0 == seed and scan0 != scan:
                    assert not (ctr & other)
            seen.setdefault((seed, scan), ctr)


def test_rbpf_shards_tile_the_ensemble_stream():
    """The sharded rows: the shards of an ensemble, first_particle = 0, N, 2N .., draw the unsharded filter's elements between them
    and all the same resampling offset; the odd / even edges the table claims are there."""
    for row in nc.RBPF_ROWS:
        if row.shard is None:
            g = nr.rbpf_elements(row.N, 9)
            assert np.array_equal(g, np.arange(row.N * 9 + 1, dtype=np.uint64))
            continue
        first, ng = row.shard
        stride = nc.rbpf_stride(row, 0)
        g = nr.rbpf_elements(row.N, stride, row.shard)
        assert int(g[0]) == first * stride and int(g[-2]) == (first + row.N) * stride - 1 and int(g[-1]) == ng * stride
        assert ("odd-base" in row.id) == bool(g[0] & np.uint64(1)) and ("odd-offset" in row.id) == bool(g[-1] & np.uint64(1))
    whole = nr.rbpf_elements(10, 9)
    parts = [nr.rbpf_elements(5, 9, (f, 10)) for f in (0, 5)]
    assert np.array_equal(np.r_[parts[0][:-1], parts[1][:-1]], whole[:-1]) and parts[0][-1] == parts[1][-1] == whole[-1]
    za, _ = nr.rbpf_normals(10, 9, 77, 1)
    zb = [nr.rbpf_normals(5, 9, 77, 1, (f, 10))[0] for f in (0, 5)]
    assert np.array_equal(np.r_[zb[0][:-1], zb[1][:-1], zb[1][-1:]], za)


# ---- the restated streams against the normal law ---------------------------------------------------------------------------------
def _ks(z):
    z = np.sort(np.asarray(z, dtype=np.float64))
    n = z.size
    cdf = 0.5 * np.array([math.erfc(-v / math.sqrt(2.0)) for v in z])
    d = max(np.max(np.arange(1, n + 1) / n - cdf), np.max(cdf - np.arange(n) / n))
    return d * math.sqrt(n)


KS_SEEDS = {"rbpf": 0x5EED, "wide": 77, "narrow": 77}


@pytest.mark.parametrize("sampler", ["rbpf", "wide", "narrow"])
def test_restated_stream_follows_the_normal_law(sampler):
    """2^20 restated values per sampler from a fixed seed: D * sqrt(n) < 1.63 (the 1 % critical value of Kolmogorov-Smirnov), and
    the two halves of a pair are uncorrelated.  With these seeds: RBPF (0x5EED, scan 0) 0.794, fp64 sampler 0.624, fp32 sampler
    0.664."""
    n = 2 ** 20
    if sampler == "rbpf":
        _, z = nr.rbpf_normals(1, n - 1, KS_SEEDS[sampler], 0)   # one stream of 2^20 elements: scan 0
        a, b = z[0::2], z[1::2]
    else:
        d = nr.mppi_noise(2 ** 13, 2 ** 6, KS_SEEDS[sampler], 0, 1.0, 1.0, sampler)
        a, b = d["duL64"].ravel(), d["duR64"].ravel()
        z = np.r_[a, b]
    assert z.size == n
    stat = _ks(z)
    corr = float(np.corrcoef(a, b)[0, 1])
    print(f"[noise restatement] {sampler}: KS D*sqrt(n) = {stat:.3f}, correlation of the halves {corr:.2e}")
    assert stat < 1.63
    assert abs(corr) < 4.0 / math.sqrt(n / 2)    # 4 sigma of the sample correlation of 2^19 independent pairs


# ---- the mutation proof ----------------------------------------------------------------------------------------------------------
FAR = {"wide": 1e-9, "rbpf": 1e-9, "narrow": 1e-3}


def _small_rows():
    return [r for r in nc.MPPI_ROWS if r.K * r.T <= 64 * 50]


@pytest.mark.parametrize("mutation", nr.MUTATIONS)
def test_every_mutation_changes_some_table_row(mutation):
    """What a kernel with this error would store differs from the contract's values in at least one row, by far more than the GPU
    test can allow (FAR: the fp64 producers are held to at most 16 ulp, 3e-14 at 8 sigma; the fp32 sampler to at most
    1e-5 * sigma * (1 + rad) < 7e-5); which rows see it is stated, not just that one does."""
    mut = frozenset([mutation])
    hit = []
    for row in _small_rows():
        good = nr.mppi_noise(*row)
        bad = nr.mppi_noise(*row, mut=mut)
        far = max(np.max(np.abs(good["duL"] - bad["duL"])), np.max(np.abs(good["duR"] - bad["duR"]))) > FAR[row.sampler]
        if far:
            hit.append(row)
    rb = []
    if mutation in ("nine_rounds", "drop_counter_high", "drop_key_high", "swap_sin_cos"):   # the ones the RBPF source has a place for
        for row in nc.RBPF_ROWS:
            for s, (seed, scan) in enumerate(nc.rbpf_schedule(row)):
                good, _ = nr.rbpf_normals(row.N, nc.rbpf_stride(row, s), seed, scan, row.shard)
                bad, _ = nr.rbpf_normals(row.N, nc.rbpf_stride(row, s), seed, scan, row.shard, mut=mut)
                if np.max(np.abs(good - bad)) > FAR["rbpf"]:
                    rb.append((row.id, s))
        assert rb, mutation
    assert hit, mutation
    want = {  # which rows must see it
        "nine_rounds": lambda r: True,
        "counter_i_major": lambda r: r.K > 1 and r.T > 1,
        "drop_counter_high": lambda r: r.tick >= 2 ** 32,
        "drop_key_high": lambda r: r.seed >= 2 ** 32,
        "swap_sin_cos": lambda r: True,
        "swap_sigmas": lambda r: True,
        "no_shift_12": lambda r: r.sampler == "wide",
    }[mutation]
    assert [r for r in _small_rows() if want(r)] == hit
    if mutation == "drop_counter_high":
        assert all(s >= 1 for _, s in rb) and {i for i, _ in rb} >= {r.id for r in nc.RBPF_ROWS if r.reseed is None}
    if mutation == "drop_key_high":
        assert {i for i, _ in rb} == {r.id for r in nc.RBPF_ROWS if r.seed is not None and r.seed >= 2 ** 32}
