#!/usr/bin/env python
"""What the correlative search against the filter's map costs (include/tbnav_icp.h MAP SEARCH M1-M9, csrc/icp_search_map.hip),
measured in ONE process on the bench room's map after 20 scans of the bench workload (device noise), at 400 x 400 with 1000
particles and at 2000 x 2000 with 64, with scans of 360 and of 1080 beams taken at the best particle's pose:

  search_map      tbnav_icp_search_map against the best particle's map, from call to return (default parameters: n = 160, +-6 cells,
                  +-20 steps), the guess 0.1 m and 0.05 rad off the pose
  search_scan     tbnav_icp_search (scan against scan) on the same scan, the same guess relative to it: what the table of a scan costs
  table_hook      tbnav_icp_search_map_table: the table kernel, its download and one synchronisation (NOT the kernel alone)
  batch_<n>       tbnav_icp_search_map_batch over n = 1, 64, 1000 pairs, particle i % N against its own map
  map_download    tbnav_rbpf_best_map: the int8 map to the host, the floor of any host route to the same table
Each figure: a host clock round the synchronous call, device idle before and after; warm-up calls first; the routes alternate inside
every repeat; median and p10-p90.  The map search's result is compared with tests/icp_search_map_restatement.py before anything is
timed.  Kernel times (icp_search_table_from_occ against icp_search_table) come from a separate `rocprofv3 --kernel-trace --stats`
run of this script with --quick, not from this script.
  python tools/icp_map_time.py [--out FILE] [--reps N] [--quick]"""
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
import icp_restatement as R  # noqa: E402
import icp_search_map_restatement as M  # noqa: E402
import icp_search_restatement as S  # noqa: E402
import oracle_api as orc  # noqa: E402  (the synthetic room only: room_scan is numpy)
import rbpf_cases as rc  # noqa: E402
from rtn_amd import icp  # noqa: E402
from rtn_amd.rbpf import ParticleFilter, default_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--quick", action="store_true", help="a few repeats and the small map only (what a rocprofv3 run of this script needs)")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
reps = 5 if args.quick else args.reps
N_SCANS, OFF = 20, (0.05, 0.1, -0.1)


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


results = []
cases = [("400x400_N1000", 10.0, 1000)] + ([] if args.quick else [("2000x2000_N64", 50.0, 64)])
steps, scans = bench_rbpf.workload(N_SCANS)
for name, half, N in cases:
    pf = ParticleFilter(default_params(N=N, k=50, map_min=-half, map_max=half))
    pf.setSeed(2026)
    for s, (prev, cur, t_icp, u) in enumerate(steps):
        pf.SLAM(scans[s], u, cur, prev, True, t_icp, None)
    pose, best = pf.getRobotState()
    geom = M.Geom(-half, -half, 0.05, pf.xsize)
    base = dict(case=name, side=pf.xsize, particles=N, scans=N_SCANS, occupied_cells_of_best=int(pf.occupiedCount()[best]))
    guess = tuple(p + o for p, o in zip(pose, OFF))
    rows = [dict(measure="map_download", **base, **stats([timed(pf.newMap) for _ in range(2 + reps)][2:]))]
    for n_beams, dd in ((360, 1.0), (1080, 1.0 / 3.0)):
        prm = icp.default_params(beam_delta_deg=dd)
        a = icp.ScanAlignment(prm)
        rng = np.random.default_rng(5)
        scan = orc.room_scan(pose, n_beams=n_beams, beam_delta_deg=dd, walls=rc.ROOM_BENCH, rng=rng)
        prev_scan = orc.room_scan(pose, n_beams=n_beams, beam_delta_deg=dd, walls=rc.ROOM_BENCH, rng=rng)
        # == before anything is timed (the occupancy as the filter reads it back; the stored field exists at these sizes)
        acc, T, info = a.searchMap(pf, guess, scan)
        occ = (pf.occDist(best).reshape(pf.xsize, pf.xsize) == 0.0)
        laser = R.Laser(prm.beam_min, prm.beam_max, prm.beam_delta, prm.range_min, prm.range_max)
        want = M.search(occ, geom, R.cloud(scan, laser)[0], guess, S.Params()).outcome.info
        assert tuple(info["T"]) == tuple(want.T) and info["score"] == want.score and info["accepted"] == want.accepted, (info, want)
        forms = {"search_map": lambda: a.searchMap(pf, guess, scan),
                 "search_scan": lambda: a.search(OFF, prev_scan, scan),
                 "table_hook": lambda: a.searchMapTable(pf, guess)}
        us = {f: [] for f in forms}
        for rep in range(5 + reps):
            for f, fn in forms.items():
                t = timed(fn)
                if rep >= 5:
                    us[f].append(t)
        for f in forms:
            rows.append(dict(measure=f, n_beams=n_beams, **base, **stats(us[f])))
        rows[-3].update(kernel=a.lastMapKernel(), quality=round(info["quality"], 3), accepted=info["accepted"],
                        error=[round(info["T"][j] - pose[j], 4) for j in range(3)])
        if n_beams == 360:
            for n in (1, 64, 1000):
                particles = np.arange(n, dtype=np.int32) % N
                Ts = np.tile(np.array(guess), (n, 1))
                b_reps = max(reps // (1 if n < 1000 else 10), 3)
                t = [timed(lambda: a.searchMapBatch(pf, Ts, scan, particles)) for _ in range(2 + b_reps)][2:]
                st = stats(t)
                rows.append(dict(measure=f"batch_{n}", n_beams=n_beams, pairs=n, us_per_pair=round(st["us_median"] / n, 2), **base, **st))
        a.close()
    for row in rows:
        results.append(row)
        print(json.dumps(row), flush=True)
    pf.close()

out = dict(tool="tools/icp_map_time.py", device=torch.cuda.get_device_name(0),
           clock="host clock round one synchronous call, device idle before and after", guess_off=OFF, results=results)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
