"""The device noise source, restated from the headers alone (include/tbnav_mppi.h, "Noise drawn ON the device" and
tbnav_mppi_set_rng_shard; include/tbnav_rbpf.h, tbnav_rbpf_set_seed / tbnav_rbpf_set_rng_shard / tbnav_rbpf_slam):

  Philox4x32-10 (Salmon et al., SC'11; the Random123 distribution's known-answer vectors are in test_noise_restatement.py)
    counter words (low 32 bits of the 64-bit counter, high 32 bits, 0, 0), key words (low, high 32 bits of the seed)
  MPPI  counter = tick*T*rollouts_global + (first_rollout + k)*T + i          -> one (duL, duR) pair for rollout k, time step i
  RBPF  counter = scan * 2^40 + pair; stream element g is pair g >> 1, half g & 1 (even: rad * cos, odd: rad * sin)
  three constructions of the two uniforms from the four output words, in the device's own arithmetic (IEEE operations on
    integers below 2^53 or 2^24: reproducible bit for bit in numpy), then
  Box-Muller  rad = sqrt(-2 ln u1), angle = 2 pi u2  in numpy.longdouble (64-bit significand), the angle reduced EXACTLY
    first: u2 is dyadic, so the quarter turn and the remainder are exact, the remainder is folded into [0, 1/8] of a turn by
    1/4 - r (exact), and only then sin / cos are called, on an angle in [0, pi/4] formed with a two-part pi.  Without the fold
    the reference itself loses digits near the zeros of the cosine; a plain float64 cos(2 * pi * u) is 1e5 ulp off there.

Every function takes `mut`, a set of names of deliberate errors (MUTATIONS): the mutation proof of test_noise_restatement.py
shows that the case table of noise_cases.py tells each of them from the contract.  Nothing else passes a non-empty set.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
MUTATIONS = ("nine_rounds", "counter_i_major", "drop_counter_high", "drop_key_high", "swap_sin_cos", "swap_sigmas", "no_shift_12")
NONE = frozenset()


# ---- Philox4x32-10 ---------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter_words, key_words, rounds=10):
    """Plain Python integers: four 32-bit counter words, two key words -> four output words."""
    c0, c1, c2, c3 = (int(w) & M32 for w in counter_words)
    k0, k1 = (int(w) & M32 for w in key_words)
    for _ in range(rounds):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def philox4x32_10_vec(counter_words, key_words, rounds=10):
    """The same over uint64 arrays holding 32-bit words (products of two of them fit a uint64): counter_words[..., 4],
    key_words[..., 2] (broadcast against each other) -> [..., 4]."""
    c = np.asarray(counter_words, dtype=np.uint64)
    k = np.asarray(key_words, dtype=np.uint64)
    m32, s32 = np.uint64(M32), np.uint64(32)
    c0, c1, c2, c3 = (c[..., j] & m32 for j in range(4))
    k0, k1 = k[..., 0] & m32, k[..., 1] & m32
    for _ in range(rounds):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & m32, (k1 + np.uint64(PHILOX_W1)) & m32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def device_words(counters, seed, mut=NONE):
    """Output words [n][4] for 64-bit counters (Python integers or a uint64 array) under a 64-bit seed, as the headers key it."""
    ctr = np.asarray([int(v) for v in counters] if not isinstance(counters, np.ndarray) else counters, dtype=np.uint64)
    hi = np.zeros_like(ctr) if "drop_counter_high" in mut else ctr >> np.uint64(32)
    cw = np.stack([ctr & np.uint64(M32), hi, np.zeros_like(ctr), np.zeros_like(ctr)], axis=-1)
    seed = int(seed)
    kw = np.array([seed & M32, 0 if "drop_key_high" in mut else (seed >> 32) & M32], dtype=np.uint64)
    return philox4x32_10_vec(cw, kw, rounds=9 if "nine_rounds" in mut else 10)


# ---- counters, as the headers word them ------------------------------------------------------------------------------------------
def mppi_counter(tick, T, K_global, first_rollout, k, i):
    """tbnav_mppi.h: tick*T*rollouts_global + (first_rollout + k)*T + i (unsharded: first_rollout = 0, rollouts_global = K)."""
    return tick * T * K_global + (first_rollout + k) * T + i


def mppi_counters(tick, T, K, first_rollout=0, K_global=None, mut=NONE):
    """All of a handle's counters of one tick as a uint64 array [T][K] (element [i][k]: time step i, rollout k)."""
    K_global = K if K_global is None else K_global
    i = np.arange(T, dtype=np.uint64)[:, None]
    k = np.arange(K, dtype=np.uint64)[None, :]
    base = mppi_counter(int(tick), T, K_global, first_rollout, 0, 0)
    assert base + K * T < 2 ** 64
    off = i * np.uint64(K) + k if "counter_i_major" in mut else k * np.uint64(T) + i
    return np.uint64(base) + off


def rbpf_counter(scan, P):
    """tbnav_rbpf.h: scan count * 2^40 + pair index."""
    return (scan << 40) + P


def rbpf_elements(N, stride, shard=None):
    """Ensemble stream elements of a handle's N*stride + 1 normals of one scan, in the handle's order.  shard = (first_particle,
    particles_global): local element j < n - 1 is element first_particle*stride + j, the last one (the resampling offset) is
    element particles_global*stride; None: elements 0 .. N*stride."""
    n = N * stride + 1
    g = np.arange(n, dtype=np.uint64)
    if shard is not None:
        first, n_global = shard
        g = g + np.uint64(first * stride)
        g[-1] = n_global * stride
    return g


# ---- the three uniform constructions (the device's arithmetic, bit for bit) ------------------------------------------------------
def uniforms_wide(r, mut=NONE):
    """MPPI fp64 sampler: ((r0 << 20 | r1 >> 12) + 0.5) * 2^-52, likewise r2, r3: 52 bits and the half fit a double, so
    u in [2^-53, 1 - 2^-53]."""
    r = np.asarray(r, dtype=np.uint64)
    sh = np.uint64(0 if "no_shift_12" in mut else 12)
    b1 = (r[..., 0] << np.uint64(20)) | (r[..., 1] >> sh)
    b2 = (r[..., 2] << np.uint64(20)) | (r[..., 3] >> sh)
    return (b1.astype(np.float64) + 0.5) * 2.0 ** -52, (b2.astype(np.float64) + 0.5) * 2.0 ** -52


def uniforms_narrow(r):
    """MPPI fp32 sampler: ((float)(r0 >> 8) + 0.5f) * 2^-24 in float32, likewise r1.  From r >> 8 = 2^23 on the half is not
    representable and the sum rounds to even: u in (0, 1], 1.0 at the top value."""
    r = np.asarray(r, dtype=np.uint64)
    h, s = np.float32(0.5), np.float32(2.0 ** -24)
    u1 = ((r[..., 0] >> np.uint64(8)).astype(np.float32) + h) * s
    u2 = ((r[..., 1] >> np.uint64(8)).astype(np.float32) + h) * s
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    return u1, u2


def uniforms_rbpf(r):
    """RBPF: (((r0 << 32 | r1) >> 11) + 0.5) * 2^-53 in float64, likewise r2, r3.  From 2^52 on the half is not representable
    and the sum rounds to even: u in (0, 1], 1.0 at the top value."""
    r = np.asarray(r, dtype=np.uint64)
    a = ((r[..., 0] << np.uint64(32)) | r[..., 1]) >> np.uint64(11)
    b = ((r[..., 2] << np.uint64(32)) | r[..., 3]) >> np.uint64(11)
    return (a.astype(np.float64) + 0.5) * 2.0 ** -53, (b.astype(np.float64) + 0.5) * 2.0 ** -53


# ---- Box-Muller in extended precision --------------------------------------------------------------------------------------------
# pi in two parts, pi = 0x C90FDAA2 2168C234 C4C6628B 80DC1CD1 ... * 2^-126: the first 64 bits (a longdouble) and the next 64, each
# put together from 32-bit integers so that no conversion rounds on the way (test_noise_restatement.py checks both against mpmath)
PI_HI = (LD(0xC90FDAA2) * LD(2) ** 32 + LD(0x2168C234)) / LD(2) ** 62
PI_LO = (LD(0xC4C6628B) * LD(2) ** 32 + LD(0x80DC1CD1)) / LD(2) ** 126


def sincos_turns(x):
    """(sin, cos)(2 pi x) for x in [0, 1] given exactly (float32 / float64 values): longdouble arrays."""
    x = np.asarray(x).astype(LD)
    q = np.floor(x * 4)                      # quarter turn 0..4 (exact: x has at most 53 bits)
    r = x - q / 4                            # [0, 1/4), exact
    fold = r > LD(0.125)
    r = np.where(fold, LD(0.25) - r, r)      # [0, 1/8], exact
    ang = r * (2 * PI_HI) + r * (2 * PI_LO)  # [0, pi/4]
    s, c = np.sin(ang), np.cos(ang)
    s, c = np.where(fold, c, s), np.where(fold, s, c)
    qi = q.astype(np.int64) & 3
    sn = np.choose(qi, [s, c, -s, -c])
    cs = np.choose(qi, [c, -s, -c, s])
    return sn, cs


def box_muller(u1, u2, mut=NONE):
    """(rad * cos, rad * sin) with rad = sqrt(-2 ln u1), angle 2 pi u2, in longdouble from exactly given uniforms."""
    rad = np.sqrt(-2 * np.log(np.asarray(u1).astype(LD)))
    sn, cs = sincos_turns(u2)
    if "swap_sin_cos" in mut:
        sn, cs = cs, sn
    return rad * cs, rad * sn


def box_muller_mp(u1, u2, bits=200):
    """One pair by mpmath at `bits` bits (the check of box_muller itself): mpf values."""
    import mpmath
    with mpmath.workprec(bits):
        a, b = mpmath.mpf(float(u1)), mpmath.mpf(float(u2))
        rad = mpmath.sqrt(-2 * mpmath.log(a))
        return rad * mpmath.cospi(2 * b), rad * mpmath.sinpi(2 * b)


# ---- the producers' streams ------------------------------------------------------------------------------------------------------
def mppi_noise(K, T, seed, tick, ul_var, ur_var, sampler, shard=None, mut=NONE):
    """What tbnav_mppi_sample_noise stores: dict of duL, duR (longdouble [T][K]), their roundings to double duL64, duR64, and
    rad [T][K] (the fp32 sampler's error unit needs it).  sampler "wide" (fp64, TBNAV_MPPI_OPT_SAMPLER = 1) or "narrow" (fp32);
    shard = (first_rollout, rollouts_global) or None.  The sigmas are sqrt(var) rounded to double, which is what the device is
    handed."""
    first, kg = shard if shard is not None else (0, K)
    r = device_words(mppi_counters(tick, T, K, first, kg, mut).ravel(), seed, mut)
    u1, u2 = uniforms_wide(r, mut) if sampler == "wide" else uniforms_narrow(r)
    a, b = box_muller(u1, u2, mut)
    sl, sr = LD(np.sqrt(np.float64(ul_var))), LD(np.sqrt(np.float64(ur_var)))
    if "swap_sigmas" in mut:
        sl, sr = sr, sl
    dl, dr = (sl * a).reshape(T, K), (sr * b).reshape(T, K)
    rad = np.sqrt(-2 * np.log(np.asarray(u1).astype(LD))).reshape(T, K)
    return dict(duL=dl, duR=dr, duL64=dl.astype(np.float64), duR64=dr.astype(np.float64), rad=rad, sig=(float(sl), float(sr)))


def rbpf_normals(N, stride, seed, scan, shard=None, mut=NONE):
    """The N*stride + 1 standard normals of one scan (stride = 3k + 3 with ICP ok, 3 without): (longdouble, double) arrays."""
    g = rbpf_elements(N, stride, shard)
    pairs, inv = np.unique(g >> np.uint64(1), return_inverse=True)
    ctr = np.uint64(rbpf_counter(int(scan), 0)) + pairs
    u1, u2 = uniforms_rbpf(device_words(ctr, seed, mut))
    a, b = box_muller(u1, u2, mut)
    z = np.where((g & np.uint64(1)) == 0, a[inv], b[inv])
    return z, z.astype(np.float64)


def ulp_error(got, ref_ld):
    """|got - ref| in units of the spacing of doubles at ref; where ref is exactly 0 the value must be 0 (inf otherwise)."""
    got = np.asarray(got, dtype=np.float64)
    ref64 = np.asarray(ref_ld).astype(np.float64)
    err = np.abs(got.astype(LD) - ref_ld) / np.spacing(np.abs(ref64)).astype(LD)
    zero = np.asarray(ref_ld) == 0
    return np.where(zero, np.where(got == 0, LD(0), LD(np.inf)), err)
