"""Noise ahead (TBNAV_MPPI_OPT_NOISE_AHEAD): the combine of a device-noise tick draws the next tick's perturbations and the next
fused kernel takes them from there when their tag is its own.  Every check runs the same ticks on two handles, the option on
(the default) and off (each fused kernel draws its own), and wants the same controls and control sequence bit for bit: graph
replays across chunks, synchronous ticks, gaps in the tick numbers, a seed change, a sampler toggle, a shard of an ensemble,
ragged K, two steps per lane, the arc dynamics."""
import numpy as np
import pytest

from cases import WAYPOINTS, make_mppi, mppi_cfg

pytestmark = pytest.mark.gpu

X0 = (0.05, -0.02, 0.3)


def _pair(pkg, K=1024, horizon=0.5, dyn=None):
    from rtn_amd import capi
    d = mppi_cfg(K, horizon)
    on, off = make_mppi(pkg, d), make_mppi(pkg, d)
    off.setOption(capi.MPPI_OPT_NOISE_AHEAD, 0)
    for m in (on, off):
        m.setWaypoint(*WAYPOINTS[1])
        if dyn:
            m.setDynamics(dyn)
    return on, off


def _same(on, off, st=0):
    assert on.lastControls(st) == off.lastControls(st)
    assert np.array_equal(on.getControls(), off.getControls())


def test_batches_across_graph_chunks_and_short_graphs(gpu_pkg):
    """250 ticks in one batch (two replays of the 100-tick chunk graph, then a graph of its own length for the rest) and blocks
    of 20 (the short graph from the second block on); the kernel names stay those of the parent build."""
    import torch
    on, off = _pair(gpu_pkg)
    st = torch.cuda.Stream().cuda_stream
    first = 0
    for n in (250, 20, 20, 20, 250):
        on.enqueueRngBatch(X0, 42, first, n, st)
        off.enqueueRngBatch(X0, 42, first, n, st)
        torch.cuda.synchronize()
        assert on.lastControls(st) == off.lastControls(st), (first, n)
        first += n
    assert on.graphReplayedTicks() > 0
    assert on.lastKernelNames() == off.lastKernelNames() == ("mppi_rollout_fused<2, 8, 1, 2>", "mppi_combine<2, 0>")
    _same(on, off, st)
    on.close(); off.close()


def test_synchronous_ticks_gaps_seed_and_sampler_changes(gpu_pkg):
    """newControlsRng tick by tick: consecutive ticks (hits), a gap (t, then t + 5), a new seed in mid-run, the sampler switched
    to fp32 and back (each a miss for the tick after it, then hits again)."""
    from rtn_amd import capi
    on, off = _pair(gpu_pkg)
    plan = [(7, t) for t in range(6)] + [(7, 10), (7, 11), (7, 12), (8, 13), (8, 14), (9, 14), ("fp32", None),
                                         (9, 15), (9, 16), ("fp64", None), (9, 17), (9, 18), (9, 3)]
    for seed, tick in plan:
        if seed in ("fp32", "fp64"):
            for m in (on, off):
                m.setOption(capi.MPPI_OPT_SAMPLER, 1 if seed == "fp64" else 0)
            continue
        a = on.newControlsRng(X0, seed, tick)
        b = off.newControlsRng(X0, seed, tick)
        assert a == b, (seed, tick)
    _same(on, off)
    on.close(); off.close()


def test_rng_shard(gpu_pkg):
    """A handle that is one shard of a larger ensemble (tbnav_mppi_set_rng_shard): the counters of its rollouts start at k0 * T
    of every tick; plain ticks, then a batch, then another shard."""
    import torch
    on, off = _pair(gpu_pkg)
    st = torch.cuda.Stream().cuda_stream
    for k0, kg in ((2048, 8192), (1024, 4096)):
        for m in (on, off):
            m.setRngShard(k0, kg)
        for t in range(4):
            on.enqueueRng(X0, 5, t, st)
            off.enqueueRng(X0, 5, t, st)
        on.enqueueRngBatch(X0, 5, 4, 130, st)
        off.enqueueRngBatch(X0, 5, 4, 130, st)
        torch.cuda.synchronize()
        _same(on, off, st)
    on.close(); off.close()


@pytest.mark.parametrize("K,horizon,dyn", [(100, 0.5, None), (1000, 0.5, None), (1024, 1.0, None), (1024, 0.5, "arc"),
                                           (2048, 0.3, None)])
def test_sizes_and_dynamics(gpu_pkg, K, horizon, dyn):
    """Ragged K (a workgroup whose last waves shadow a valid rollout), T = 100 (two steps per lane), the exact-arc dynamics and
    the largest K with eight rollouts per workgroup: plain ticks and a batch."""
    import torch
    on, off = _pair(gpu_pkg, K, horizon, dyn)
    st = torch.cuda.Stream().cuda_stream
    for t in range(3):
        on.enqueueRng(X0, 11, t, st)
        off.enqueueRng(X0, 11, t, st)
    on.enqueueRngBatch(X0, 11, 3, 120, st)
    off.enqueueRngBatch(X0, 11, 3, 120, st)
    torch.cuda.synchronize()
    _same(on, off, st)
    on.close(); off.close()


def test_option_toggle_in_mid_run(gpu_pkg):
    """Switching the option on a running handle (off -> on -> off) changes nothing in the results."""
    import torch
    from rtn_amd import capi
    on, off = _pair(gpu_pkg)
    st = torch.cuda.Stream().cuda_stream
    first = 0
    for v in (0, 1, 0, 1):
        on.setOption(capi.MPPI_OPT_NOISE_AHEAD, v)
        on.enqueueRngBatch(X0, 3, first, 40, st)
        off.enqueueRngBatch(X0, 3, first, 40, st)
        first += 40
        torch.cuda.synchronize()
        assert on.lastControls(st) == off.lastControls(st), v
    _same(on, off, st)
    on.close(); off.close()
