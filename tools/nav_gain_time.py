#!/usr/bin/env python
"""What ranking the exploration frontiers by information gain costs (include/tbnav_nav.h G17-G20, csrc/nav_gain.hip), measured in ONE
process on the map after 20 scans (device noise) of SURVEY 8-d's room on its own trajectory — tools/nav_frontier_time.py's settings: 400 x 400
with 1000 particles and 2000 x 2000 with 64 — at R = 32 and R = 70 (either side of the kernels' threshold):

  find            tbnav_nav_find_frontiers of the best particle, from call to return (host clock, device idle before and after)
  find_gain       tbnav_nav_find_frontiers_gain, the same find and the gain of every seed cell
  gain_stage      the gain's kernels alone (nav_gain_classes, nav_gain_list, nav_frontier_gain<RMAX>), HIP events on the filter's stream
                  (tbnav_nav_profile_find_frontiers_gain's fifth stage)
  solve_frontiers tbnav_nav_solve_frontiers (every seed starts at 0) against
  solve_ranked    tbnav_nav_solve_frontiers_ranked at gain_weight 2 from the same find
Two warm-up calls; the forms alternate inside every repeat; median and p10-p90 over 31 repeats.
  python tools/nav_gain_time.py [--out FILE] [--reps N]"""
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
from rtn_amd.nav import GoalField  # noqa: E402
from rtn_amd.rbpf import ParticleFilter, default_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=31)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"

RES, R_ROBOT, R_INFLATE, K, MIN_CELLS, GAIN_WEIGHT = 0.05, 0.10, 0.45, 8.0, 8, 2
N_SCANS = 20
RANGES = (32, 70)


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


def survey_workload(n_scans):
    world = bench_rbpf._world()
    steps, poses = world.trajectory(n_scans, inc=bench_rbpf.TRAJ_SURVEY)
    rng = np.random.default_rng(7)
    return steps, [bench_rbpf._room_scan(poses[s], rng, bench_rbpf.ROOM_SURVEY) for s in range(n_scans)]


results = []
steps, scans = survey_workload(N_SCANS)
for name, half, N in (("400x400_N1000", 10.0, 1000), ("2000x2000_N64", 50.0, 64)):
    pf = ParticleFilter(default_params(N=N, k=50, map_min=-half, map_max=half))
    pf.setSeed(2026)
    for s, (prev, cur, t_icp, u) in enumerate(steps):
        pf.SLAM(scans[s], u, cur, prev, True, t_icp, None)
    side = pf.xsize
    nav = GoalField(side, side, -half, -half, RES)
    nav.setCostFrom(pf, R_ROBOT, R_INFLATE, K)
    for R in RANGES:
        info, gi = nav.findFrontiersGain(pf, R, MIN_CELLS)
        assert info["seed_cells"] > 0, "SURVEY's room leaves frontiers"
        base = dict(case=name, room="survey", side=side, particles=N, scans=N_SCANS, min_cells=MIN_CELLS, range_cells=R, rays=gi["rays"],
                    viewpoints=gi["viewpoints"], gain_min=gi["gain_min"], gain_max=gi["gain_max"], gain_weight=GAIN_WEIGHT,
                    kernels=";".join(nav.lastGainKernels()))
        forms = {"find": lambda: nav.findFrontiers(pf, MIN_CELLS), "find_gain": lambda: nav.findFrontiersGain(pf, R, MIN_CELLS),
                 "solve_frontiers": nav.solveFrontiers, "solve_ranked": lambda: nav.solveFrontiersRanked(GAIN_WEIGHT)}       # (the solves follow find_gain)
        us = {f: [] for f in forms}
        stage_us = []
        for rep in range(2 + args.reps):
            for f, fn in forms.items():
                t = timed(fn)
                if rep >= 2:
                    us[f].append(t)
            torch.cuda.synchronize()
            _, _, st = nav.profileFindFrontiersGain(pf, R, MIN_CELLS)
            if rep >= 2:
                stage_us.append(st["gain"])
        rows = [dict(measure=f, **base, **stats(v)) for f, v in us.items()]
        rows.append(dict(measure="gain_stage", **base, **stats(stage_us)))
        nav.findFrontiersGain(pf, R, MIN_CELLS)
        nav.solveFrontiers(); plain_rounds = nav.lastSolve()["rounds"]
        nav.solveFrontiersRanked(GAIN_WEIGHT)
        rows.append(dict(measure="solve_rounds", **base, solve_frontiers_rounds=plain_rounds, solve_ranked_rounds=nav.lastSolve()["rounds"]))
        for row in rows:
            results.append(row)
            print(json.dumps(row), flush=True)
    nav.close()
    pf.close()

out = dict(tool="tools/nav_gain_time.py", device=torch.cuda.get_device_name(0),
           clock="host clock round one synchronous call, device idle before and after; gain_stage: HIP events on the filter's stream round the gain's kernels of one find",
           parameters=dict(resolution=RES, r_robot=R_ROBOT, r_inflate=R_INFLATE, k=K, min_cells=MIN_CELLS, gain_weight=GAIN_WEIGHT), results=results)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
