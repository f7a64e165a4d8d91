#!/usr/bin/env python
"""What finding the exploration frontiers costs (include/tbnav_nav.h G10-G16, csrc/nav_frontier.hip), measured in ONE process on the
map after 20 scans (device noise), at 400 x 400 with 1000 particles and 2000 x 2000 with 64, in two rooms: the bench room
(bench_rbpf.workload), which the scanner sees whole — no frontier cell is left, so this is the find's floor — and SURVEY 8-d's room on
its own trajectory, where 114 of 360 beams do not return and the map ends in long frontiers along the 3.5 m range limit:

  find            tbnav_nav_find_frontiers of the best particle, from call to return (host clock, device idle before and after)
  find_by_stage   the same find with HIP events on the filter's stream between its stages (tbnav_nav_profile_find_frontiers): mark,
                  the label rounds WITH the host's reads of their records, sizes, seeds — and the labelling's rounds and launches
  solve_frontiers tbnav_nav_solve_frontiers (all seed cells as goals) against
  solve_one       tbnav_nav_solve to one of those cells on the same grid
  host_floor      what the host route cannot go below: tbnav_rbpf_particle_map's download of the int8 map alone (the search on the
                  host comes on top)
Two warm-up calls; the forms alternate inside every repeat; median and p10-p90 over 31 repeats.
  python tools/nav_frontier_time.py [--out FILE] [--reps N]"""
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

RES, R_ROBOT, R_INFLATE, K, MIN_CELLS = 0.05, 0.10, 0.45, 8.0, 8
N_SCANS = 20
STAGES = ("mark", "label", "sizes", "seeds")


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
WORK = dict(bench=bench_rbpf.workload(N_SCANS), survey=survey_workload(N_SCANS))
for room, name, half, N in [(r, n, h, c) for r in ("bench", "survey") for n, h, c in (("400x400_N1000", 10.0, 1000), ("2000x2000_N64", 50.0, 64))]:
    steps, scans = WORK[room]
    pf = ParticleFilter(default_params(N=N, k=50, map_min=-half, map_max=half))
    pf.setSeed(2026)
    for s, (prev, cur, t_icp, u) in enumerate(steps):
        pf.SLAM(scans[s], u, cur, prev, True, t_icp, None)
    best = pf.getRobotState()[1]
    side = pf.xsize
    nav = GoalField(side, side, -half, -half, RES)
    nav.setCostFrom(pf, R_ROBOT, R_INFLATE, K)
    info = nav.findFrontiers(pf, MIN_CELLS)
    min_cells = MIN_CELLS
    seeds = info["seed_cells"] > 0
    assert seeds or room == "bench", "SURVEY's room leaves frontiers"
    one = max(nav.frontiers(), key=lambda f: f["size"])["root"] if seeds else None          # a cell of the largest cluster: a seed
    base = dict(case=name, room=room, side=side, particles=N, scans=N_SCANS, min_cells=min_cells, frontier_cells=info["cells"], clusters=info["clusters"],
                seed_clusters=info["seed_clusters"], seed_cells=info["seed_cells"], label_rounds=info["rounds"], label_launches=info["launches"],
                label_tile_visits=info["tile_visits"])
    forms = {"find": lambda: nav.findFrontiers(pf, min_cells), "host_floor": lambda: pf.particleMap(best)}
    if seeds:
        forms.update(solve_frontiers=nav.solveFrontiers, solve_one=lambda: nav.solve(*one))
    us = {f: [] for f in forms}
    stage_us = {s: [] for s in STAGES}
    for rep in range(2 + args.reps):
        for f, fn in forms.items():
            t = timed(fn)
            if rep >= 2:
                us[f].append(t)
        torch.cuda.synchronize()
        _, st = nav.profileFindFrontiers(pf, min_cells)
        if rep >= 2:
            for s in STAGES:
                stage_us[s].append(st[s])
    rows = [dict(measure=f, **base, **stats(v)) for f, v in us.items()]
    rows += [dict(measure="find_by_stage", stage=s, kernel="nav_frontier_" + s, **base, **stats(stage_us[s])) for s in STAGES]
    if seeds:
        rounds = {}
        nav.findFrontiers(pf, min_cells)
        nav.solveFrontiers(); rounds["solve_frontiers_rounds"] = nav.lastSolve()["rounds"]
        nav.solve(*one); rounds["solve_one_rounds"] = nav.lastSolve()["rounds"]
        rows.append(dict(measure="solve_rounds", **base, **rounds))
    for row in rows:
        results.append(row)
        print(json.dumps(row), flush=True)
    nav.close()
    pf.close()

out = dict(tool="tools/nav_frontier_time.py", device=torch.cuda.get_device_name(0),
           clock="host clock round one synchronous call, device idle before and after; find_by_stage: HIP events on the filter's stream between the stages of one find",
           parameters=dict(resolution=RES, r_robot=R_ROBOT, r_inflate=R_INFLATE, k=K, min_cells=MIN_CELLS), results=results)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
