#!/usr/bin/env python
"""What the MPPI cost field (include/tbnav_mppi.h, COST FIELD) costs per tick, measured in ONE process.

At (K, T) = (1024, 50), (8192, 100), (65536, 100), device noise, a 400 x 400 field:
  a  a handle with the field                                   the feature's headline
  b  the same handle with weight = 0                            the lookup's price when it cannot matter
  c  a handle without a field, forced to TBNAV_MPPI_OPT_KERNEL = 0   the field-less sequential tick: what the lookup adds to its own kernel shape
  d  the default handle without a field                         what a user gives up at that size
Each case: blocks of `ticks` production ticks through tbnav_mppi_enqueue_rng_batch on a non-default stream, a host clock round
the block that ends in a device synchronise; warm-up blocks first; the cases alternate inside every repeat; median and p10-p90
of the per-tick time over the blocks.  Also the per-kernel durations of tbnav_mppi_profile_kernels_rng and the kernel names.
  python tools/mppi_field_time.py [--out FILE] [--blocks N] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

g.load_package()
from rtn_amd import capi  # noqa: E402
from rtn_amd.mppi import MPPI, CartModel, LossFunc, cost_field_from_distance  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--blocks", type=int, default=15)
ap.add_argument("--quick", action="store_true", help="a tenth of the ticks per block (a rehearsal, or a run under a profiler)")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"

X0, XD = (0.0, 0.0, 0.0), (2.0, 0.0, 0.0)
SHAPES = [(1024, 0.5, 1000), (8192, 1.0, 400), (65536, 1.0, 200)]   # K, horizon (dt 0.01), ticks per block


def field_400():
    """400 x 400 cells of 0.05 m from (-10, -10) (640 KB): a few discs inflated as a node would inflate the filter's distance
    field; the rollouts from the origin toward (2, 0) cross the band round the nearest one."""
    c = -10.0 + (np.arange(400) + 0.5) * 0.05
    X, Y = np.meshgrid(c, c, indexing="ij")
    d = np.full(X.shape, 10.0)
    for cx, cy, r in ((1.0, 0.04, 0.15), (-2.0, 3.0, 0.5), (4.0, -1.0, 0.3), (0.5, 1.5, 0.2)):
        d = np.minimum(d, np.maximum(np.hypot(X - cx, Y - cy) - r, 0.0))
    return cost_field_from_distance(d, 0.10, 0.45)


def make(K, horizon, kernel=None):
    m = MPPI(CartModel(0.033, 0.16), LossFunc([1e4, 1e4, 1.0], [0.1, 0.1], [1e3, 1e3, 1e3]), 0.01, 6.35495, 0.9, 0.9, horizon, 0.01, K,
             keep_j=False, kernel=kernel)
    m.setWaypoint(*XD)
    return m


stream = torch.cuda.Stream()
st = stream.cuda_stream
values = field_400()
results = []
for K, horizon, ticks in SHAPES:
    if args.quick:
        ticks = max(20, ticks // 10)
    cases = {"a_field": make(K, horizon), "b_field_weight_0": make(K, horizon), "c_no_field_kernel_0": make(K, horizon, kernel=0),
             "d_no_field_default": make(K, horizon)}
    cases["a_field"].setCostField(values, -10.0, -10.0, 0.05, 2e4)
    cases["b_field_weight_0"].setCostField(values, -10.0, -10.0, 0.05, 0.0)
    first = {name: 0 for name in cases}
    per_tick = {name: [] for name in cases}
    for rep in range(2 + args.blocks):           # two warm-up blocks of every case, then the timed ones, the cases in turn
        for name, m in cases.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.enqueueRngBatch(X0, 42, first[name], ticks, st)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            first[name] += ticks
            if rep >= 2:
                per_tick[name].append(dt / ticks * 1e6)
    for name, m in cases.items():
        v = np.array(per_tick[name])
        names = m.lastKernelNames()
        replayed = m.graphReplayedTicks()
        ms = m.profileKernelsRng(X0, 42, first[name], st, reps=100)
        row = dict(K=K, T=m.steps, case=name, ticks_per_block=ticks, blocks=len(v), us_per_tick_median=round(float(np.median(v)), 3),
                   us_per_tick_p10=round(float(np.percentile(v, 10)), 3), us_per_tick_p90=round(float(np.percentile(v, 90)), 3),
                   rollout_kernel=names[0], combine_kernel=names[1], graph_replayed_ticks=replayed,
                   kernel_us=dict(rollout=round(ms[0] * 1e3, 3), partials=round(ms[1] * 1e3, 3), combine=round(ms[2] * 1e3, 3)))
        results.append(row)
        print(json.dumps(row), flush=True)
        m.close()
out = dict(tool="tools/mppi_field_time.py", device=torch.cuda.get_device_name(0), field="400 x 400 float32 (640 KB), resolution 0.05",
           clock="host clock round a block of tbnav_mppi_enqueue_rng_batch ticks ending in a device synchronise; device noise",
           quick=bool(args.quick), results=results)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
