"""mppi_rollout_fused after the dead vector work went (csrc/mppi_rollout.hip): small_sincos's full-range fallback is a real
wave-uniform branch again, the padding lanes (i >= T) carry step T - 1's controls instead of zeros, and a record's rollout count is
min(R, K - k0) instead of a seventh reduction.  Everything against the oracle at test_mppi_gpu.py's tolerances, on the controls and
on J (keep_j), with resident noise where the inputs have to be planted.

The branch: a lane is `big` when |d| = |h/2 * r/b * (ur - ul)| > 2^-5 with the kernel's own roundings (w = r/b * (ur - ul),
d = h * (0.5 * w)); a wave (= one rollout, its lanes over the time steps) enters the block when one of its lanes is.  Cases: no
lane big; one lane at exactly 2^-5 (not big: no wave may need the block); the same lane one ulp above (one wave of eight enters);
dt = 0.1 with drawn noise (most waves enter, a few do not).  The number of big lanes of each case is asserted in numpy before it
runs: a case that does not bite is an error.

Padding lanes and the count: T = 1 (the smallest a handle accepts), 49, 50, 63, 64 (one step per lane), 65, 100 (two), K = 8, 9, 12
(K = 9: the second workgroup has one live wave and seven shadows; its count must be 1.  The library has no getter for the
workgroups' own records, so the count is seen in the K-slice record tbnav_mppi_shard_partials folds them into: n == K, which a
count of R in the ragged workgroup would make 16), resident and device noise at K = 9.  T = 65: the last live lane holds a live and
a padding step."""
import numpy as np
import pytest

import oracle_api as orc
from cases import WAYPOINTS, make_mppi, mppi_cfg, rel_err

pytestmark = pytest.mark.gpu

J_RTOL, U_RTOL, U_ATOL = 1e-12, 1e-9, 1e-12   # tests/test_mppi_gpu.py's

XD = WAYPOINTS[2]
X0 = (0.5, 0.2, 1.0)
LIMIT = 0.03125   # 2^-5


def _cfg(K, T, dt=0.01):
    d = mppi_cfg(K, (T + 0.5) * dt, dt=dt)   # (+ half a step: int(horizon / dt) is T whatever the division rounds to)
    assert orc.mppi_steps(d) == T
    return d


def _noise(seed, K, T, var=0.9):
    return orc.normal_stream(seed, K * T * 2, 0.0, np.sqrt(var)).reshape(K, T, 2)


def _d(d, noise):
    """The small angle of every (k, i) as the kernel forms it from a fresh handle's controls (u = 0: ul, ur are the perturbations)."""
    rb = np.float64(d["wheel_radius"]) / np.float64(d["wheel_base"])
    w = rb * (noise[:, :, 1] - noise[:, :, 0])
    return np.float64(d["dt"]) * (0.5 * w)


def _plant(d, target):
    """A right-wheel perturbation (left = 0) whose small angle is exactly `target`."""
    rb = np.float64(d["wheel_radius"]) / np.float64(d["wheel_base"])
    x = np.float64(target) / (np.float64(d["dt"]) * 0.5 * rb)
    cand = [x]
    for _ in range(16):
        cand = [np.nextafter(cand[0], -np.inf)] + cand + [np.nextafter(cand[-1], np.inf)]
    hit = [c for c in cand if np.float64(d["dt"]) * (0.5 * (rb * (c - 0.0))) == target]
    assert hit, "no perturbation within 16 ulp gives the wanted angle"
    return hit[0]


def _tick_resident(gpu_pkg, d, noise):
    import torch
    K, T = noise.shape[:2]
    m = make_mppi(gpu_pkg, d)
    assert (m.steps, m.rollouts) == (T, K) and m.rollout_kernel.startswith("mppi_rollout_fused<8 "), m.rollout_kernel
    m.setWaypoint(*XD)
    tz = torch.from_numpy(noise).cuda()
    a, b = tz[:, :, 0].t().contiguous(), tz[:, :, 1].t().contiguous()
    got = m.newControlsDev(X0, a.data_ptr(), b.data_ptr())
    assert m.lastKernelNames()[0] == f"mppi_rollout_fused<2, 8, {1 if T <= 64 else 2}, 0>", m.lastKernelNames()
    return m, got, (a, b)


def _against_oracle(d, noise, m, got):
    T = noise.shape[1]
    ref = orc.mppi_new_controls(d, np.zeros((2, T)), (0, 0), XD, X0, noise)
    ej = rel_err(m.costToGo(), ref["J"])
    print(f"K={noise.shape[0]} T={T}: J rel err {ej:.3e}, out {got} against {ref['out']}")
    assert ej < J_RTOL
    assert np.allclose(got, ref["out"], rtol=U_RTOL, atol=U_ATOL)
    assert np.allclose(m.getControls(), ref["u"], rtol=U_RTOL, atol=U_ATOL)


PLANT_AT = (3, 17)   # (rollout, time step): one lane of one wave


@pytest.mark.parametrize("case", ["none", "at_limit", "one_ulp_above"])
def test_fallback_branch_shipped_parameters(gpu_pkg, case):
    K, T = 8, 50
    d = _cfg(K, T)
    noise = _noise(11, K, T)
    if case != "none":
        target = LIMIT if case == "at_limit" else np.nextafter(np.float64(LIMIT), 1.0)
        noise[PLANT_AT[0], PLANT_AT[1]] = (0.0, _plant(d, target))
        assert _d(d, noise)[PLANT_AT] == target
    big = np.abs(_d(d, noise)) > LIMIT
    assert int(big.sum()) == (1 if case == "one_ulp_above" else 0), big.sum()
    assert big.any(axis=1).tolist() == [case == "one_ulp_above" and k == PLANT_AT[0] for k in range(K)]
    m, got, _keep = _tick_resident(gpu_pkg, d, noise)
    _against_oracle(d, noise, m, got)


def test_fallback_branch_taken_by_most_waves(gpu_pkg):
    K, T = 16, 50
    d = _cfg(K, T, dt=0.1)
    noise = _noise(12, K, T)
    waves = (np.abs(_d(d, noise)) > LIMIT).any(axis=1)
    assert K // 2 < int(waves.sum()) < K, waves   # most waves enter the block, and some skip it
    m, got, _keep = _tick_resident(gpu_pkg, d, noise)
    _against_oracle(d, noise, m, got)


@pytest.mark.parametrize("K", [8, 9, 12])
@pytest.mark.parametrize("T", [1, 49, 50, 63, 64, 65, 100])
def test_padding_lanes_and_record_count_resident_noise(gpu_pkg, K, T):
    import torch
    d = _cfg(K, T)
    noise = _noise(100 * K + T, K, T)
    m, got, (a, b) = _tick_resident(gpu_pkg, d, noise)
    _against_oracle(d, noise, m, got)
    m2 = make_mppi(gpu_pkg, d)
    m2.setWaypoint(*XD)
    rec = torch.zeros(T, m2.records_per_step, 8, dtype=torch.float64, device="cuda")
    m2.shardPartials(X0, a.data_ptr(), b.data_ptr(), rec.data_ptr())
    torch.cuda.synchronize()
    assert m2.records_per_step == 1 and np.array_equal(rec[:, 0, 6].cpu().numpy(), np.full(T, float(K)))


@pytest.mark.parametrize("T", [1, 49, 50, 63, 64, 65, 100])
def test_padding_lanes_and_record_count_device_noise(gpu_pkg, T):
    import torch
    K = 9
    d = _cfg(K, T)
    m, m_ref = make_mppi(gpu_pkg, d), make_mppi(gpu_pkg, d)
    for h in (m, m_ref):
        h.setWaypoint(*XD)
    got = m.newControlsRng(X0, 77, 3)
    assert m.lastKernelNames()[0] == f"mppi_rollout_fused<2, 8, {1 if T <= 64 else 2}, 2>", m.lastKernelNames()
    m_ref.sampleNoise(77, 3)
    a, b = m_ref.getNoise()   # [T][K] each: what the kernel drew
    _against_oracle(d, np.stack([a.T, b.T], axis=2), m, got)
    rec = torch.zeros(T, m_ref.records_per_step, 8, dtype=torch.float64, device="cuda")
    m_ref.shardPartialsRng(X0, 77, 3, rec.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(rec[:, 0, 6].cpu().numpy(), np.full(T, float(K)))
