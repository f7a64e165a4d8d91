"""The straight-line form of mppi_combine<KEEP, 0> (csrc/mppi_softmin.hip: 16-byte record loads, no predicates, and its six wave
sums side by side on full-mask DPP moves whose lanes below 63 hold no prefix sums — csrc/wave.hpp, wave_sums_dpp) against the
general form of the same kernel template, bit for bit, on the records of real ticks.

tbnav_mppi_debug_combine_general runs the last tick's combine once more through mppi_combine<KEEP, 1> with one group — the text the
sharded ticks run: predicated 8-byte loads, six wave_sum_dpp (the masked scan) one after the other — over the same fused records
and the same warm start, into a scratch vector.  Column 0 of it is what the tick returned, column i + 1 what getControls gives as
column i.

Shapes: K = 1024 (128 records per step, mppi_combine<2, 0>) and K = 2048 (256 records, <4, 0>); T = 1, 3, 5 leave waves past the
last time step in the last workgroup of four, T = 4 fills one exactly, T = 50 is the shipped horizon (13 workgroups).  Three
consecutive device-noise ticks each, on two handles: one is never asked for its controls between ticks, so ticks 2 and 3 read the
warm start shifted on the fly; the other is asked after every tick, so they read a vector shifted on the host.  Both must agree.
One case at lambda = 1e-3 (weights spread over many binades), one with rollouts whose cost overflows (tests/mppi_cases.py's
overflow_noise through resident noise: a whole workgroup of eight, whose record is m = +inf, A = B = C = 0, and one rollout among
finite ones).

Equality is `==` on the float64 values.  Against the oracle the tolerances are tests/test_mppi_combine_gpu.py's (controls 1e-9
relative / 1e-12 absolute) at the shipped lambda, and 1e-6 / 1e-9 — what tests/test_mppi_gpu.py and
tests/test_mppi_instantiations_gpu.py hold such ticks to — at lambda = 1e-3 and with overflowing rollouts."""
import numpy as np
import pytest

import mppi_cases as mc
import oracle_api as orc
from cases import WAYPOINTS, make_mppi, mppi_cfg

pytestmark = pytest.mark.gpu

U_RTOL, U_ATOL = 1e-9, 1e-12         # tests/test_mppi_combine_gpu.py
WIDE_RTOL, WIDE_ATOL = 1e-6, 1e-9    # tests/test_mppi_gpu.py (lambda = 1e-3), tests/test_mppi_instantiations_gpu.py (overflow)
UINIT = (0.3, -0.2)
XD = WAYPOINTS[2]
SEED = 42
COMBINE = {1024: "mppi_combine<2, 0>", 2048: "mppi_combine<4, 0>"}


def _handle(gpu_pkg, d, T, opts=()):
    m = make_mppi(gpu_pkg, d)
    for name, value in opts:
        m.setOption(getattr(gpu_pkg.capi, "MPPI_OPT_" + name), value)
    assert m.steps == T == orc.mppi_steps(d)
    m.setWaypoint(*XD)
    m.setInitialControls(*UINIT)
    return m


def _same_bits(general, out, controls):
    """`general` [2][T] before the shift against the tick's own answer: `out` and, where given, the shifted vector."""
    assert np.all(np.isfinite(general)), general
    assert (general[0, 0], general[1, 0]) == tuple(out), (general[:, 0], out)
    if controls is not None:
        assert np.array_equal(general[:, 1:], controls[:, :-1]), np.argwhere(general[:, 1:] != controls[:, :-1])[:8]
        assert tuple(controls[:, -1]) == UINIT


def _three_ticks(gpu_pkg, d, K, T, tick_fn, noise_fn, rtol, atol, opts=(), combine=None):
    """tick_fn(handle, x0, tick, noise) -> (ul, ur); noise_fn(tick) -> [K][T][2] for the oracle (and for resident-noise ticks)."""
    on_the_fly, on_the_host = _handle(gpu_pkg, d, T, opts), _handle(gpu_pkg, d, T, opts)
    combine = combine or COMBINE[K]
    u_ref = np.zeros((2, T)); u_ref[0], u_ref[1] = UINIT
    x0 = (0.5, 0.2, 1.0)
    general = None
    for tick in range(3):
        nz = noise_fn(tick)
        with np.errstate(all="ignore"):
            ref = orc.mppi_new_controls(d, u_ref, UINIT, XD, x0, nz)
        out = tick_fn(on_the_fly, x0, tick, nz)
        assert on_the_fly.lastKernelNames()[1] == combine, on_the_fly.lastKernelNames()
        general = on_the_fly.debugCombineGeneral()
        _same_bits(general, out, None)
        out_h = tick_fn(on_the_host, x0, tick, nz)
        assert on_the_host.lastKernelNames()[1] == combine, on_the_host.lastKernelNames()
        general_h, u_h = on_the_host.debugCombineGeneral(), on_the_host.getControls()
        _same_bits(general_h, out_h, u_h)
        assert out_h == out and np.array_equal(general_h, general)
        print(f"[chains] K={K} T={T} tick={tick} out={out} |out - oracle|={np.abs(np.asarray(out) - np.asarray(ref['out'])).max():.3e} "
              f"|u - oracle|={np.abs(u_h - ref['u']).max():.3e}")
        assert np.all(np.isfinite(ref["u"]))
        assert np.allclose(out, ref["out"], rtol=rtol, atol=atol), (out, ref["out"])
        assert np.allclose(u_h, ref["u"], rtol=rtol, atol=atol)
        u_ref = ref["u"]
        x0 = (x0[0] + 0.002, x0[1] - 0.001, x0[2] + 0.003)
    u = on_the_fly.getControls()
    _same_bits(general, out, u)
    assert np.array_equal(u, u_h)
    on_the_fly.close(); on_the_host.close()


def _device_noise_case(gpu_pkg, K, T, rtol=U_RTOL, atol=U_ATOL, opts=(), combine=None, **cfg):
    d = mppi_cfg(K, mc.horizon(T), **cfg)
    sampler = _handle(gpu_pkg, d, T, opts)      # only ever draws: the perturbations of (SEED, tick) as the ticking handles' kernels draw them

    def noise(tick):
        sampler.sampleNoise(SEED, tick)
        du_l, du_r = sampler.getNoise()   # [T][K] each
        return np.ascontiguousarray(np.stack([du_l.T, du_r.T], axis=2))

    _three_ticks(gpu_pkg, d, K, T, lambda m, x0, tick, nz: m.newControlsRng(x0, SEED, tick), noise, rtol, atol, opts, combine)
    sampler.close()


@pytest.mark.parametrize("T", [1, 3, 4, 5, 50])
@pytest.mark.parametrize("K", [1024, 2048])
def test_straight_form_equals_the_general_form_bit_for_bit(gpu_pkg, K, T):
    _device_noise_case(gpu_pkg, K, T)


def test_straight_form_with_eight_records_a_lane(gpu_pkg):
    """The third instantiation that holds the form: four rollouts per workgroup leave 512 records per step, mppi_combine<8, 0>
    with the four-wave combine switched off."""
    _device_noise_case(gpu_pkg, 2048, 5, opts=(("KERNEL", -4), ("WIDE_COMBINE", 0)), combine="mppi_combine<8, 0>")


def test_straight_form_with_weights_over_many_binades(gpu_pkg):
    _device_noise_case(gpu_pkg, 1024, 50, rtol=WIDE_RTOL, atol=WIDE_ATOL, lam=1e-3)


def test_straight_form_with_overflowed_records(gpu_pkg):
    """Rollouts 8 .. 15 are one workgroup of the fused kernel: their record is m = +inf, A = B = C = 0, n = 8 — a weight of
    exp(-inf) = 0 that must never be multiplied into anything; rollout 100 overflows among seven finite ones."""
    K, T = 1024, 50
    d = mppi_cfg(K, mc.horizon(T))
    bad = list(range(8, 16)) + [100]

    def noise(tick):
        clean = orc.normal_stream(K + T + tick, K * T * 2, 0.0, np.sqrt(0.9)).reshape(K, T, 2)
        return mc.overflow_noise(clean, bad)

    def tick_fn(m, x0, tick, nz):
        out = m.newControls(*x0, nz)
        J = m.costToGo()
        assert np.all(J[:, bad] == np.inf) and np.all(np.isfinite(np.delete(J, bad, axis=1)))
        return out

    _three_ticks(gpu_pkg, d, K, T, tick_fn, noise, WIDE_RTOL, WIDE_ATOL)
