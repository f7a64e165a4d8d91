#!/usr/bin/env python
"""What the planner's cost grid costs when it is taken from the filter's map (include/tbnav_nav.h G7-G9, csrc/nav_from_map.hip),
measured in ONE process on the bench room's map after 20 scans of the bench workload (device noise):

  device   tbnav_nav_set_cost_from_rbpf of the best particle, from call to return
  host     the route it replaces: tbnav_rbpf_get_occ_dist + nav_cost_from_distance + tbnav_nav_set_cost — its first call (which
           allocates the stored field of EVERY particle) and its steady state; where the filter refuses it, the status instead
  kernel   nav_cost_from_occ alone, by events round 20 launches in a row with the slot named (tbnav_nav_profile_cost_from_rbpf)
at 400 x 400 with 1000 particles, 2000 x 2000 with 64, and 2000 x 2000 with 12 500 (one GPU's share of BASELINE configs[4]).
Each figure: a host clock round the synchronous call, device idle before and after; two warm-up calls; the two routes alternate inside
every repeat; median and p10-p90 over the repeats.  The grids of the two routes are compared with == before anything is timed.
  python tools/nav_from_map_time.py [--out FILE] [--reps N] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402

g.load_package()
import bench_rbpf  # noqa: E402
from rtn_amd import capi  # noqa: E402
from rtn_amd.nav import GoalField, nav_cost_from_distance  # noqa: E402
from rtn_amd.rbpf import ParticleFilter, default_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--quick", action="store_true", help="skip the 12 500-particle case")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"

RES, R_ROBOT, R_INFLATE, K = 0.05, 0.10, 0.45, 8.0
N_SCANS = 20


def stats(us):
    v = np.array(us)
    return dict(us_median=round(float(np.median(v)), 1), us_p10=round(float(np.percentile(v, 10)), 1), us_p90=round(float(np.percentile(v, 90)), 1),
                reps=len(v))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def host_route(pf, nav, p):
    nav.setCost(nav_cost_from_distance(pf.occDist(p).reshape(pf.xsize, pf.xsize), R_ROBOT, R_INFLATE, K))


results = []
cases = [("400x400_N1000", 10.0, 1000), ("2000x2000_N64", 50.0, 64)] + ([] if args.quick else [("2000x2000_N12500", 50.0, 12500)])
steps, scans = bench_rbpf.workload(N_SCANS)
for name, half, N in cases:
    pf = ParticleFilter(default_params(N=N, k=50, map_min=-half, map_max=half))
    pf.setSeed(2026)
    for s, (prev, cur, t_icp, u) in enumerate(steps):
        pf.SLAM(scans[s], u, cur, prev, True, t_icp, None)
    best = pf.getRobotState()[1]
    side = pf.xsize
    nav = GoalField(side, side, -half, -half, RES)
    base = dict(case=name, side=side, particles=N, scans=N_SCANS, occupied_cells_of_best=int(pf.occupiedCount()[best]))
    nav.setCostFrom(pf, R_ROBOT, R_INFLATE, K)
    from_device = nav.cost()
    base["blocked_cells"] = int((from_device == 0).sum())
    # the host route: its first call allocates, and may be refused
    host_status, first_us = capi.OK, None
    try:
        first_us = timed(lambda: host_route(pf, nav, best))
    except capi.TbnavError as e:
        host_status = e.status
    if host_status == capi.OK:
        assert np.array_equal(nav.cost(), from_device), "the two routes disagree"
    forms = {"device": lambda: nav.setCostFrom(pf, R_ROBOT, R_INFLATE, K)}
    if host_status == capi.OK:
        forms["host"] = lambda: host_route(pf, nav, best)
    us = {f: [] for f in forms}
    for rep in range(2 + args.reps):
        for f, fn in forms.items():
            t = timed(fn)
            if rep >= 2:
                us[f].append(t)
    kernel_us = [nav.profileCostFrom(pf, R_ROBOT, R_INFLATE, K, 20, particle=best) for _ in range(2 + args.reps)][2:]     # (the slot named: no arg-max launch in between)
    rows = [dict(measure="device_route", kernel=nav.lastCostKernel(), **base, **stats(us["device"])),
            dict(measure="kernel_by_events", kernel=nav.lastCostKernel(), launches_per_rep=20, **base, **stats(kernel_us))]
    if host_status == capi.OK:
        rows.append(dict(measure="host_route_first_call", **base, us=round(first_us, 1)))
        rows.append(dict(measure="host_route_steady", **base, **stats(us["host"])))
        rows.append(dict(measure="host_over_device", **base, ratio_of_medians=round(float(np.median(us["host"]) / np.median(us["device"])), 1)))
    else:
        rows.append(dict(measure="host_route_refused", **base, status=int(host_status), status_text=capi.lib().tbnav_status_string(host_status).decode()))
    for row in rows:
        results.append(row)
        print(json.dumps(row), flush=True)
    nav.close()
    pf.close()

out = dict(tool="tools/nav_from_map_time.py", device=torch.cuda.get_device_name(0),
           clock="host clock round one synchronous call, device idle before and after; kernel_by_events: HIP events round 20 launches",
           parameters=dict(resolution=RES, r_robot=R_ROBOT, r_inflate=R_INFLATE, k=K), results=results)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
