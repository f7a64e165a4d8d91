#!/usr/bin/env python
"""What the goal field (include/tbnav_nav.h, csrc/nav.hip) costs, measured in ONE process.

  solve     tbnav_nav_solve (synchronous) on an empty 400 x 400 grid from the corner, a 400 x 400 room with discs, the 96 x 96
            serpentine at cost 64 and a 2000 x 2000 room: wall time, rounds, launches, tile visits
  handover  tbnav_nav_apply_to_mppi (G5 on the device + a device-to-device copy) against tbnav_nav_get_field +
            tbnav_mppi_set_cost_field (G5 on the device, down to the host, finiteness check, up again), at 400 x 400 and 2000 x 2000
Each figure: a host clock round the call (every one of these calls ends with the device idle); two warm-up calls first; where two
forms are compared they alternate inside every repeat; median and p10-p90 over the repeats.
  python tools/nav_time.py [--out FILE] [--reps N]"""
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
from rtn_amd.mppi import MPPI, CartModel, LossFunc  # noqa: E402
from rtn_amd.nav import GoalField, nav_cost_from_distance  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=15)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"

RES = 0.05


def room(n, discs, seed=5):
    """An n x n room of 0.05 m cells: nav_cost_from_distance (r_robot 0.10, r_inflate 0.45, k 8) of the distance to the room's
    walls and to `discs` drawn discs, as a node would inflate the filter's distance field."""
    c = (np.arange(n) + 0.5) * RES
    X, Y = np.meshgrid(c, c, indexing="ij")
    side = n * RES
    d = np.minimum(np.minimum(X, side - X), np.minimum(Y, side - Y))
    rng = np.random.default_rng(seed)
    for _ in range(discs):
        cx, cy = rng.uniform(0.15, 0.85, 2) * side
        r = rng.uniform(0.02, 0.06) * side
        d = np.minimum(d, np.maximum(np.hypot(X - cx, Y - cy) - r, 0.0))
    return nav_cost_from_distance(d, 0.10, 0.45, 8.0)


def serpentine(n=96):
    c = np.full((n, n), 64, dtype=np.uint8)
    for k in range(n // 2):
        c[2 * k + 1, :] = 0
        if 2 * k + 1 < n - 1:
            c[2 * k + 1, n - 1 if k % 2 == 0 else 0] = 64
    return c


def free_near(cost, near):
    ix, iy = np.nonzero(cost)
    k = int(np.argmin((ix - near[0]) ** 2 + (iy - near[1]) ** 2))
    return int(ix[k]), int(iy[k])


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


room_400, room_2000 = room(400, 12), room(2000, 60)
SOLVES = [("empty_400", np.ones((400, 400), dtype=np.uint8), (0, 0)), ("room_400", room_400, free_near(room_400, (350, 380))),
          ("serpentine_96", serpentine(), (0, 0)), ("room_2000", room_2000, free_near(room_2000, (1750, 1900)))]
results = []
navs = {}
for name, cost, goal in SOLVES:
    nav = GoalField(cost.shape[0], cost.shape[1], 0.0, 0.0, RES)
    nav.setCost(cost)
    us = [timed(lambda: nav.solve(*goal)) for _ in range(2 + args.reps)][2:]
    info = nav.lastSolve()
    d = nav.costToGo()
    row = dict(measure="solve", case=name, nx=cost.shape[0], ny=cost.shape[1], goal=list(goal), blocked_fraction=round(float((cost == 0).mean()), 4),
               reached_cells=int((d != 0xFFFFFFFF).sum()), kernel=info["kernel"], rounds=info["rounds"], launches=info["launches"],
               tiles=list(info["tiles"]), tile_visits=info["tile_visits"], **stats(us))
    results.append(row)
    print(json.dumps(row), flush=True)
    navs[name] = nav

for name in ("room_400", "room_2000"):
    nav = navs[name]
    m = MPPI(CartModel(0.033, 0.16), LossFunc([0.0, 0.0, 1.0], [0.1, 0.1], [1e3, 1e3, 1e3]), 0.01, 6.35495, 0.9, 0.9, 0.5, 0.01, 1024, keep_j=False)
    forms = {"apply_to_mppi": lambda: nav.applyTo(m, 10.0, 1e4),
             "get_field_then_set_cost_field": lambda: m.setCostField(nav.field(10.0), 0.0, 0.0, RES, 1e4)}
    us = {f: [] for f in forms}
    for rep in range(2 + args.reps):
        for f, fn in forms.items():
            t = timed(fn)
            if rep >= 2:
                us[f].append(t)
    for f in forms:
        row = dict(measure="handover", case=name, nx=nav.nx, ny=nav.ny, form=f, field_bytes=4 * nav.nx * nav.ny, **stats(us[f]))
        results.append(row)
        print(json.dumps(row), flush=True)
    m.close()
for nav in navs.values():
    nav.close()
out = dict(tool="tools/nav_time.py", device=torch.cuda.get_device_name(0),
           clock="host clock round one synchronous call (tbnav_nav_solve; the hand-over's calls), device idle before and after",
           results=results)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
