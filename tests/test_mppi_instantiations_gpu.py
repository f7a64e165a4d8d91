"""Every instantiation csrc/mppi.hip can launch of mppi_rollout_fused, mppi_rollout_scan and mppi_rollout_cost, by name, against
the oracle (tests/mppi_cases.py is the table; tests/test_mppi_cases.py holds it complete against the shipped listing), the
rejections of TBNAV_MPPI_OPT_KERNEL, and the overflow rule — a rollout whose cost overflows to +inf weighs nothing — in every
producer of records.  Tolerances are tests/test_mppi_gpu.py's: J <= 1e-12 relative by rel_err, controls 1e-9 relative / 1e-12
absolute; the overflow cases' controls 1e-6 relative / 1e-9 absolute, test_prefix_form_across_lambda_and_an_overflowing_rollout's
own bound for such a tick."""
import numpy as np
import pytest

import mppi_cases as mc
import oracle_api as orc
from cases import WAYPOINTS, make_mppi, mppi_cfg, rel_err

pytestmark = pytest.mark.gpu

J_RTOL = 1e-12      # tests/test_mppi_gpu.py
U_RTOL = 1e-9
U_ATOL = 1e-12
OVF_RTOL, OVF_ATOL = 1e-6, 1e-9     # tests/test_mppi_gpu.py, the overflowing rollout of the prefix form
XD = WAYPOINTS[2]
UINIT = (2.0, 3.5)      # a turning warm start (the arc dynamics' heading sweeps)


def _noise(seed, K, T, var=0.9):
    return orc.normal_stream(seed, K * T * 2, 0.0, np.sqrt(var)).reshape(K, T, 2)


def _handle(gpu_pkg, case, opts=None, uinit=UINIT):
    from rtn_amd import capi
    d = mppi_cfg(case.K, mc.horizon(case.T))
    m = make_mppi(gpu_pkg, d)
    for name, value in (case.opts if opts is None else opts):
        m.setOption(getattr(capi, "MPPI_OPT_" + name), value)
    m.setDynamics(case.dyn)
    assert m.steps == case.T == orc.mppi_steps(d)
    m.setWaypoint(*XD)
    m.setInitialControls(*uinit)
    return m, d


def _three_ticks_against_the_oracle(gpu_pkg, case):
    m, d = _handle(gpu_pkg, case)
    u = np.zeros((2, case.T)); u[0], u[1] = UINIT
    x0 = (0.5, 0.2, 1.0)
    for tick in range(3):
        nz = _noise(1000 * case.T + case.K + tick, case.K, case.T)
        ref = orc.mppi_new_controls(d, u, UINIT, XD, x0, nz, dyn=1 if case.dyn == "arc" else 0)
        got = m.newControls(*x0, nz)
        assert m.lastKernelNames()[:2] == (case.rollout, case.combine), m.lastKernelNames()
        assert rel_err(m.costToGo(), ref["J"]) < J_RTOL
        assert np.allclose(got, ref["out"], rtol=U_RTOL, atol=U_ATOL)
        assert np.allclose(m.getControls(), ref["u"], rtol=U_RTOL, atol=U_ATOL)
        u = ref["u"]
        x0 = (x0[0] + 0.002, x0[1] - 0.001, x0[2] + 0.003)
    m.close()


@pytest.mark.parametrize("case", mc.fused_resident_cases(), ids=lambda c: c.id)
def test_fused_kernel_with_resident_noise(gpu_pkg, case):
    _three_ticks_against_the_oracle(gpu_pkg, case)


@pytest.mark.parametrize("case", mc.scan_cases(), ids=lambda c: c.id)
def test_time_parallel_kernel(gpu_pkg, case):
    _three_ticks_against_the_oracle(gpu_pkg, case)


@pytest.mark.parametrize("case", mc.sequential_cases(), ids=lambda c: c.id)
def test_sequential_kernel(gpu_pkg, case):
    _three_ticks_against_the_oracle(gpu_pkg, case)


@pytest.mark.parametrize("case", mc.fused_rng_cases(), ids=lambda c: c.id)
def test_fused_kernel_with_in_kernel_noise(gpu_pkg, case):
    """newControlsRng on one handle == sampleNoise + newControlsDev on a second handle forced to the same rollouts per workgroup,
    over three ticks; the second handle's <TR, R, TL, 0> is held to the oracle by test_fused_kernel_with_resident_noise."""
    m_rng, _ = _handle(gpu_pkg, case)
    m_ref, _ = _handle(gpu_pkg, case, opts=[o for o in case.opts if o[0] != "NOISE_AHEAD"])
    resident = case.rollout[:case.rollout.rindex(",")] + ", 0>"
    x0 = (0.1, -0.2, 0.3)
    for tick in range(3):
        got = m_rng.newControlsRng(x0, 77, tick)
        m_ref.sampleNoise(77, tick)
        want = m_ref.newControlsDev(x0, 0, 0)
        assert m_rng.lastKernelNames()[:2] == (case.rollout, case.combine), m_rng.lastKernelNames()
        assert m_ref.lastKernelNames()[:2] == (resident, case.combine), m_ref.lastKernelNames()
        assert got == want, (tick, got, want)
        assert np.array_equal(m_rng.costToGo(), m_ref.costToGo())
        assert np.array_equal(m_rng.getControls(), m_ref.getControls())
        x0 = (x0[0] + 0.002, x0[1], x0[2] + 0.001)
    assert np.all(np.isfinite(m_rng.getControls()))
    m_rng.close(); m_ref.close()


@pytest.mark.parametrize("T,value,why", mc.REJECTIONS)
def test_kernel_option_rejections_leave_the_handle_as_it_was(gpu_pkg, T, value, why):
    capi = gpu_pkg.capi
    d = mppi_cfg(70, mc.horizon(T))
    a, b = make_mppi(gpu_pkg, d), make_mppi(gpu_pkg, d)
    assert a.steps == T
    for m in (a, b):
        m.setWaypoint(*XD)
    assert capi.lib().tbnav_mppi_set_option(a._h, capi.MPPI_OPT_KERNEL, value) == capi.ERR_INVALID_ARG, why
    nz = _noise(T, 70, T)
    x0 = (0.5, 0.2, 1.0)
    for tick in range(2):
        assert a.newControls(*x0, nz) == b.newControls(*x0, nz)
        assert a.lastKernelNames() == b.lastKernelNames() and a.lastKernelNames()[0]
        assert np.array_equal(a.costToGo(), b.costToGo())
    assert np.array_equal(a.getControls(), b.getControls())
    a.close(); b.close()


# ---- the overflow rule --------------------------------------------------------------------------------------------------------
def _overflow_tick(gpu_pkg, kernel, K, T, rollouts, rollout_name):
    """One tick with `rollouts` overflowing.  Returns (J, out, controls, oracle's dict)."""
    from rtn_amd import capi
    d = mppi_cfg(K, mc.horizon(T))
    m = make_mppi(gpu_pkg, d)
    if kernel is not None:
        m.setOption(capi.MPPI_OPT_KERNEL, kernel)
    assert m.steps == T
    m.setWaypoint(*XD)
    x0 = (0.3, -0.2, 0.7)
    bad = mc.overflow_noise(_noise(K + T, K, T), rollouts)
    with np.errstate(all="ignore"):
        ref = orc.mppi_new_controls(d, np.zeros((2, T)), (0, 0), XD, x0, bad)
    out = m.newControls(*x0, bad)
    assert m.lastKernelNames()[0] == rollout_name, m.lastKernelNames()
    J, u = m.costToGo(), m.getControls()
    return m, d, bad, x0, J, out, u, ref


def _assert_overflow(J, out, u, ref, rollouts, K):
    fine = np.setdiff1d(np.arange(K), rollouts)
    assert np.all(J[:, rollouts] == np.inf), J[:, rollouts]
    if len(fine):
        assert np.all(np.isfinite(J[:, fine])) and rel_err(J[:, fine], ref["J"][:, fine]) < J_RTOL
        assert np.all(np.isfinite(ref["u"]))            # (the oracle: weight exp(-inf) = 0)
        assert np.all(np.isfinite(out)) and np.all(np.isfinite(u)), (out, u)
        assert np.allclose(out, ref["out"], rtol=OVF_RTOL, atol=OVF_ATOL) and np.allclose(u, ref["u"], rtol=OVF_RTOL, atol=OVF_ATOL)
    else:                                               # every rollout overflowed: inf - inf in the reference itself
        assert np.all(np.isnan(ref["u"][:, :-1])) and np.all(np.isnan(ref["out"]))
        assert np.all(np.isnan(u[:, :-1])) and np.all(np.isnan(out)), (out, u)


@pytest.mark.parametrize("which", ["last", "middle", "all", "mixed"])
@pytest.mark.parametrize("name,kernel,R,K,T,rollout", mc.OVERFLOW_PRODUCERS, ids=[p[0] for p in mc.OVERFLOW_PRODUCERS])
def test_overflowing_rollouts_weigh_nothing_in_every_rollout_kernel(gpu_pkg, name, kernel, R, K, T, rollout, which):
    """K = 2R + 1: the last workgroup's only live rollout overflows; all R rollouts of the middle workgroup; every rollout; one
    rollout among finite ones.
    J is +inf in those columns and the oracle's elsewhere, the controls are the oracle's (NaN on both sides when nothing is left)."""
    rollouts = mc.overflow_sets(K, R)[which]
    m, d, bad, x0, J, out, u, ref = _overflow_tick(gpu_pkg, kernel, K, T, rollouts, rollout)
    _assert_overflow(J, out, u, ref, rollouts, K)
    m.close()


@pytest.mark.parametrize("which", ["last", "middle", "mixed"])
@pytest.mark.parametrize("R,T", [(4, 50), (8, 100), (16, 50)])
def test_overflowing_rollouts_through_the_merged_slice_records(gpu_pkg, R, T, which):
    """tbnav_mppi_shard_partials on a fused handle: mppi_merge_records folds the fine records — one of them with m = +inf and
    A = B = C = 0 — into the slice's record, and the combine of that record gives the oracle's controls."""
    import torch
    from rtn_amd import capi
    K = 2 * R + 1
    rollouts = mc.overflow_sets(K, R)[which]
    d = mppi_cfg(K, mc.horizon(T))
    m = make_mppi(gpu_pkg, d, kernel=-R)
    m.setWaypoint(*XD)
    x0 = (0.3, -0.2, 0.7)
    bad = mc.overflow_noise(_noise(K + T, K, T), rollouts)
    ref = orc.mppi_new_controls(d, np.zeros((2, T)), (0, 0), XD, x0, bad)
    nz = torch.from_numpy(bad).cuda()
    duL, duR = nz[:, :, 0].t().contiguous(), nz[:, :, 1].t().contiguous()
    rec = torch.full((T, m.records_per_step, 8), float("nan"), dtype=torch.float64, device="cuda")
    m.shardPartials(x0, duL.data_ptr(), duR.data_ptr(), rec.data_ptr())
    torch.cuda.synchronize()
    assert m.lastKernelNames()[0] == f"mppi_rollout_fused<2, {R}, {1 if T <= 64 else 2}, 0>"
    r = rec.cpu().numpy()
    print(f"[merged record, R={R} T={T} {which}] step {T - 1}: {r[T - 1, 0]}")
    assert np.all(np.isfinite(r[:, 0, :6])) and np.all(r[:, 0, 6] == K), r[:, 0]
    m.shardCombine(rec.data_ptr(), 1)
    out, u = m.lastControls(), m.getControls()
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(u))
    assert np.allclose(out, ref["out"], rtol=OVF_RTOL, atol=OVF_ATOL) and np.allclose(u, ref["u"], rtol=OVF_RTOL, atol=OVF_ATOL)
    m.close()


def test_one_overflowing_rollout_alone_in_the_last_workgroup_at_the_handles_own_choice(gpu_pkg):
    """K = 1025 at the default 8 rollouts per workgroup: rollout 1024 is the only live one of workgroup 128."""
    K, T, rollout = mc.OVERFLOW_DEFAULT
    m, d, bad, x0, J, out, u, ref = _overflow_tick(gpu_pkg, None, K, T, [K - 1], rollout)
    _assert_overflow(J, out, u, ref, [K - 1], K)
    m.close()
