"""mppi_combine<KEEP, 0> and mppi_combine_wide alone, on synthetic records, and through whole ticks (tests/mppi_cases.py).

tbnav_mppi_shard_combine takes any n_shards > 0 and the caller's buffer [G][T][S][8], so shardCombine(ptr, G) on a small handle runs
the production single-process combine at any record count: its straight form (G == 1, S == KEEP * 64), the register-resident general
form, the re-reading loop (more records than KEEP * 64), the sub-wave form (fewer than 64 records: several time steps per wave) and
the division r / S of G > 1.  The reference is combine_reference below: mppi.cpp:112-137 over records (include/tbnav_mppi.h,
"Sharded soft-min") in extended precision (numpy.longdouble, 64-bit significand), skipping records with n <= 0 as the three device
forms do.  Tolerances are tests/test_mppi_gpu.py's: controls 1e-9 relative / 1e-12 absolute, J 1e-12 relative."""
import numpy as np
import pytest

import mppi_cases as mc
import oracle_api as orc
from cases import WAYPOINTS, make_mppi, mppi_cfg, rel_err

pytestmark = pytest.mark.gpu

J_RTOL = 1e-12      # tests/test_mppi_gpu.py
U_RTOL = 1e-9
U_ATOL = 1e-12
UINIT = (0.3, -0.2)
LD = np.longdouble


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def softmin_weights(rec, lam=mc.LAMBDA):
    """rec [T][R][8] -> (s [T][R] in extended precision: exp(((m_r - M) * -1) / lambda) over the records with n > 0, 0 for the
    others; live [T][R])."""
    rec = np.asarray(rec, dtype=np.float64)
    live = rec[..., 6] > 0.0
    m = np.where(live, rec[..., 0], np.inf).astype(LD)
    M = m.min(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        s = np.where(live, np.exp(((m - M) * LD(-1.0)) / LD(lam)), LD(0.0))
    return s, live


def combine_reference(rec, u, uinit, lam=mc.LAMBDA, umax=mc.UMAX):
    """One combine (mppi.cpp:112-137) of rec [T][R][8] onto the warm start u [2][T], in extended precision.
    Returns (u_upd [2][T] before the shift, u_next [2][T] shifted with uinit in the last column, (ul, ur), clamped [2][T])."""
    rec = np.asarray(rec, dtype=np.float64)
    s, live = softmin_weights(rec, lam)
    f = [np.where(live, rec[..., q], 0.0).astype(LD) for q in range(7)]
    floor = LD(1e-8)
    W = (s * f[1]).sum(axis=1) + floor * f[6].sum(axis=1)
    raw = np.stack([np.asarray(u[0], dtype=LD) + ((s * f[2]).sum(axis=1) + floor * f[4].sum(axis=1)) / W,
                    np.asarray(u[1], dtype=LD) + ((s * f[3]).sum(axis=1) + floor * f[5].sum(axis=1)) / W])
    clamped = (raw < -umax) | (raw > umax)
    upd = np.where(raw < -umax, -umax, np.where(raw > umax, umax, raw)).astype(np.float64)    # std::clamp: a NaN stays a NaN
    nxt = np.concatenate([upd[:, 1:], np.array([[uinit[0]], [uinit[1]]])], axis=1)
    return upd, nxt, (float(upd[0, 0]), float(upd[1, 0])), clamped


# ---- records drawn like real ones ------------------------------------------------------------------------------------------------
def draw_records(seed, G, T, S):
    """[G][T][S][8]: m in [50, 500] with (where there are that many) three records per step within 0.02 of the minimum, n in
    1 ... 2048, A in [1, n], B and C = A * N(0, 1), D and E = n * N(0, 1)."""
    rng = np.random.default_rng(seed)
    R = G * S
    rec = np.zeros((T, R, 8))
    rec[..., 0] = rng.uniform(50.0, 500.0, (T, R))
    for i in range(T):
        near = rng.choice(R, size=min(3, R), replace=False)
        rec[i, near, 0] = rec[i, :, 0].min() + rng.uniform(0.0, 0.02, near.size)   # (the step's minimum can only have moved up, and not past them)
    n = rng.integers(1, 2049, (T, R)).astype(np.float64)
    rec[..., 6] = n
    rec[..., 1] = rng.uniform(1.0, n)
    rec[..., 2] = rec[..., 1] * rng.standard_normal((T, R))
    rec[..., 3] = rec[..., 1] * rng.standard_normal((T, R))
    rec[..., 4] = n * rng.standard_normal((T, R))
    rec[..., 5] = n * rng.standard_normal((T, R))
    return to_device_layout(rec, G, S)


def to_device_layout(rec_t, G, S):
    """[T][G * S][8], record r = g * S + s  ->  [G][T][S][8]."""
    T = rec_t.shape[0]
    return np.ascontiguousarray(rec_t.reshape(T, G, S, 8).transpose(1, 0, 2, 3))


def by_step(rec):
    """[G][T][S][8] -> [T][G * S][8]."""
    G, T, S, _ = rec.shape
    return rec.transpose(1, 0, 2, 3).reshape(T, G * S, 8)


def warm_start(seed, T):
    return np.random.default_rng(seed + 7919).uniform(-0.5, 0.5, (2, T))


def two_calls_reference(rec, u0):
    """The reference over two consecutive combines of the same records: the second reads the first's controls shifted."""
    r = by_step(rec)
    upd1, nxt1, out1, cl1 = combine_reference(r, u0, UINIT)
    upd2, nxt2, out2, cl2 = combine_reference(r, nxt1, UINIT)
    return dict(nxt1=nxt1, out1=out1, nxt2=nxt2, out2=out2, clamped=cl1 | cl2, upd1=upd1)


def well_posed(rec):
    """What the ordinary cases promise: at least three records (all, where there are fewer) of weight > 1e-3 at every step."""
    s, live = softmin_weights(by_step(rec))
    return bool(np.all((s > 1e-3).sum(axis=1) >= min(3, s.shape[1])))


# ---- the special record sets (each changes the reference's answer, or provably must not: tests/test_mppi_cases.py) ---------------------
def special_records(kind, seed, G, T, S):
    rec = draw_records(seed, G, T, S)
    if kind == "clamp":             # B pushed far out, one way at even steps and the other at odd ones; C the other way round
        sign = np.where(np.arange(T) % 2 == 0, 1.0, -1.0)[None, :, None]
        rec[..., 2] = rec[..., 1] * 20.0 * sign
        rec[..., 3] = rec[..., 1] * -20.0 * sign
        rec[:, T // 2, :, 2:4] = rec[:, T // 2, :, 1:2] * 0.25       # (and one step that stays inside)
    elif kind in ("empty_groups", "empty_groups_low_m"):   # whole groups that hold no rollouts: every other group
        rec[1::2] = 0.0
        if kind == "empty_groups_low_m":
            rec[1::2, ..., 0] = -1e300                      # would be the minimum, were it looked at
    elif kind == "one_left":        # all records but one empty (the last: the highest lane's)
        keep = rec[-1, :, -1].copy()
        rec[:] = 0.0
        rec[-1, :, -1] = keep
    elif kind == "overflowed":      # what mppi_partials writes for a slice whose rollouts all overflowed — in place of each step's
        for i in range(T):          # cheapest record, so that a reader who gave it any weight would be far off
            g, s = divmod(int(np.argmin(by_step(rec)[i, :, 0])), S)
            rec[g, i, s, 0] = np.inf
            rec[g, i, s, 1:4] = 0.0
    else:
        raise KeyError(kind)
    return rec


SPECIAL_KINDS = ("clamp", "empty_groups", "empty_groups_low_m", "one_left", "overflowed")
SPECIAL_SHAPES = [(64, 33, 5), (2049, 65, 5), (64, 300, 70)]    # (handle's K, G, T): sub-wave <2, 0>, <4, 0> with r / S, the re-reading loop


def seed_of(K, G, T, kind=""):
    return 1000003 * K + 1009 * G + T + 17 * SPECIAL_KINDS.index(kind) + 17 if kind else 1000003 * K + 1009 * G + T


# ---- on the device ---------------------------------------------------------------------------------------------------------------
_handles = {}


def _handle(gpu_pkg, K, T):
    """One handle per (K, T) for the whole module: the combine reads nothing of it but the warm start, uinit, lambda and the clamp."""
    if (K, T) not in _handles:
        m = make_mppi(gpu_pkg, mppi_cfg(K, mc.horizon(T)))
        assert m.steps == T and m.records_per_step == -(-K // 2048)
        m.setInitialControls(*UINIT)
        _handles[(K, T)] = m
    return _handles[(K, T)]


def _run_two_calls(m, rec, G, u0):
    import torch
    d = torch.from_numpy(rec).cuda()
    m.setControls(u0)                                  # the first call reads them unshifted
    m.shardCombine(d.data_ptr(), G)
    name1, out1 = m.lastKernelNames()[1], m.lastControls()
    m.shardCombine(d.data_ptr(), G)                    # the second reads the first's shifted, uinit in the last column
    out2, nxt2 = m.lastControls(), m.getControls()
    m.setControls(u0)
    m.shardCombine(d.data_ptr(), G)
    nxt1 = m.getControls()                             # (the getter applies the owed shift for real: asked for on a run of its own)
    torch.cuda.synchronize()
    return dict(name=name1, out1=out1, out2=out2, nxt1=nxt1, nxt2=nxt2)


def _assert_two_calls(got, ref):
    for k in ("out1", "out2", "nxt1", "nxt2"):
        assert np.allclose(got[k], ref[k], rtol=U_RTOL, atol=U_ATOL, equal_nan=False), (k, got[k], ref[k])


@pytest.mark.parametrize("T", mc.COMBINE_T)
@pytest.mark.parametrize("K,G", [(K, G) for K, Gs in mc.COMBINE_G.items() for G in Gs])
def test_combine_on_synthetic_records_at_every_record_count(gpu_pkg, K, G, T):
    S = -(-K // 2048)
    seed = seed_of(K, G, T)
    print(f"[combine] K={K} G={G} T={T} records/step={G * S} seed={seed}")
    rec, u0 = draw_records(seed, G, T, S), warm_start(seed, T)
    ref = two_calls_reference(rec, u0)
    assert well_posed(rec) and not ref["clamped"].any()      # the reference alone: the case is what it is meant to be
    got = _run_two_calls(_handle(gpu_pkg, K, T), rec, G, u0)
    assert got["name"] == mc.combine_name(G * S), got["name"]
    _assert_two_calls(got, ref)


@pytest.mark.parametrize("kind", SPECIAL_KINDS)
@pytest.mark.parametrize("K,G,T", SPECIAL_SHAPES)
def test_combine_on_special_records(gpu_pkg, K, G, T, kind):
    """Clamps on both sides; whole groups with n = 0 (fields 0, then m = -1e300); all records but one empty; one record
    m = +inf, A = B = C = 0, n > 0."""
    S = -(-K // 2048)
    seed = seed_of(K, G, T, kind)
    print(f"[combine {kind}] K={K} G={G} T={T} records/step={G * S} seed={seed}")
    rec, u0 = special_records(kind, seed, G, T, S), warm_start(seed, T)
    ref = two_calls_reference(rec, u0)
    assert np.all(np.isfinite(ref["nxt2"]))
    if kind == "clamp":
        assert (ref["upd1"] == mc.UMAX).any() and (ref["upd1"] == -mc.UMAX).any() and (np.abs(ref["upd1"]) < mc.UMAX).any()
    got = _run_two_calls(_handle(gpu_pkg, K, T), rec, G, u0)
    assert got["name"] == mc.combine_name(G * S), got["name"]
    _assert_two_calls(got, ref)


def _noise(seed, K, T, var=0.9):
    return orc.normal_stream(seed, K * T * 2, 0.0, np.sqrt(var)).reshape(K, T, 2)


@pytest.mark.parametrize("case", [c for c in mc.combine_tick_cases()], ids=lambda c: c.id)
def test_combine_through_whole_ticks(gpu_pkg, case):
    """The fused kernel with 4 rollouts per workgroup leaves S = ceil(K / 4) records per step: every body of mppi_combine<KEEP, 0>
    and mppi_combine_wide behind real records, against the oracle's tick over three warm-started ticks."""
    from rtn_amd import capi
    d = mppi_cfg(case.K, mc.horizon(case.T))
    m = make_mppi(gpu_pkg, d)
    for name, value in case.opts:
        m.setOption(getattr(capi, "MPPI_OPT_" + name), value)
    assert m.steps == case.T == orc.mppi_steps(d)
    xd = WAYPOINTS[2]
    m.setWaypoint(*xd)
    u = np.zeros((2, case.T)); x0 = (0.5, 0.2, 1.0)
    for tick in range(3):
        nz = _noise(case.K + tick, case.K, case.T)
        ref = orc.mppi_new_controls(d, u, (0, 0), xd, x0, nz)
        got = m.newControls(*x0, nz)
        assert m.lastKernelNames()[:2] == (case.rollout, case.combine), m.lastKernelNames()
        assert rel_err(m.costToGo(), ref["J"]) < J_RTOL
        assert np.allclose(got, ref["out"], rtol=U_RTOL, atol=U_ATOL)
        assert np.allclose(m.getControls(), ref["u"], rtol=U_RTOL, atol=U_ATOL)
        u = ref["u"]
        x0 = (x0[0] + 0.002, x0[1] - 0.001, x0[2] + 0.003)
    m.close()
