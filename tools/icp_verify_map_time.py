#!/usr/bin/env python
"""What the check of a pose against the filter's map costs (include/tbnav_icp.h MAP CHECK V1-V10, csrc/icp_verify_map.hip), measured
in ONE process on the bench room's map at 400 x 400 with 1000 particles after 20 scans of the bench workload (device noise), with
scans of 360 and of 1080 beams taken at the best particle's pose and the pose taken from alignMap:

  verify_map            tbnav_icp_verify_map against the best particle's map, from call to return (the defaults: H = 96, k = 2)
  verify_map_no_points  the same call with a scan whose ranges are all below range_min: the launch, the staging of the three bitmaps
                        and the record, and no walk.  verify_map minus this is the walk, BY DIFFERENCE (the entry has no timed form)
  align_map, search_map tbnav_icp_align_map and tbnav_icp_search_map on the same scan from a guess half a cell and half a degree off,
                        in the same loop: the links before this one
  batch_<n>             tbnav_icp_verify_map_batch over n = 64 and 1000 pairs, particle i % N against its own map, the poses spread
                        over +-half a cell and +-half a degree
  relocalize_map_checked, relocalize_map   ScanAlignment.relocalizeMapChecked whole, beside relocalizeMap
Each figure: a host clock round the synchronous call, device idle before and after; warm-up calls first; the routes alternate inside
every repeat; median and p10-p90.  The check's record is compared with tests/icp_verify_map_restatement.py before anything is timed.
NOT measured here: the kernel or its stages between events; LDS use and occupancy.
  python tools/icp_verify_map_time.py [--out FILE] [--reps N]"""
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
import icp_verify_map_restatement as V  # noqa: E402
import oracle_api as orc  # noqa: E402  (the synthetic room only: room_scan is numpy)
import rbpf_cases as rc  # noqa: E402
from rtn_amd import icp  # noqa: E402
from rtn_amd.rbpf import ParticleFilter, default_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
reps = args.reps
N_SCANS, N, HALF = 20, 1000, 10.0
OFF = (0.5 * np.pi / 180.0, 0.025, -0.025)


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
steps, scans = bench_rbpf.workload(N_SCANS)
pf = ParticleFilter(default_params(N=N, k=50, map_min=-HALF, map_max=HALF))
pf.setSeed(2026)
for s, (prev, cur, t_icp, u) in enumerate(steps):
    pf.SLAM(scans[s], u, cur, prev, True, t_icp, None)
pose, best = pf.getRobotState()
geom = V.Geom(-HALF, -HALF, 0.05, pf.xsize)
base = dict(case="400x400_N1000", side=pf.xsize, particles=N, scans=N_SCANS, occupied_cells_of_best=int(pf.occupiedCount()[best]))
guess = tuple(p + o for p, o in zip(pose, OFF))
for n_beams, dd in ((360, 1.0), (1080, 1.0 / 3.0)):
    prm = icp.default_params(beam_delta_deg=dd)
    a = icp.ScanAlignment(prm)
    scan = orc.room_scan(pose, n_beams=n_beams, beam_delta_deg=dd, walls=rc.ROOM_BENCH, rng=np.random.default_rng(5))
    nothing = np.full(n_beams, 0.05, dtype=np.float32)
    ok, T, ainfo = a.alignMap(pf, guess, scan)
    # == before anything is timed (the classes as the filter reads them back; the stored field exists at this size)
    info, beams = a.verifyMapBeams(pf, T, scan)
    occ = (pf.occDist(best).reshape(pf.xsize, pf.xsize) == 0.0)
    laser = R.Laser(prm.beam_min, prm.beam_max, prm.beam_delta, prm.range_min, prm.range_max)
    cloud, beam = R.cloud(scan, laser)
    want = V.verify(V.Classes.from_export(pf.particleMap(best), occ, pf.xsize), geom, cloud, beam, scan.size, T, V.Params())
    assert info == want.info and all(np.array_equal(beams[f], want.beams[f]) for f in V.BEAM_FIELDS), (info, want.info)
    forms = {"verify_map": lambda: a.verifyMap(pf, T, scan), "verify_map_no_points": lambda: a.verifyMap(pf, T, nothing),
             "align_map": lambda: a.alignMap(pf, guess, scan), "search_map": lambda: a.searchMap(pf, guess, scan),
             "relocalize_map_checked": lambda: a.relocalizeMapChecked(pf, scan), "relocalize_map": lambda: a.relocalizeMap(pf, scan)}
    us = {f: [] for f in forms}
    for rep in range(5 + reps):
        for f, fn in forms.items():
            t = timed(fn)
            if rep >= 5:
                us[f].append(t)
    rows = [dict(measure=f, n_beams=n_beams, **base, **stats(us[f])) for f in forms]
    rows[0].update(kernel=a.lastVerifyMapKernel(), pose_from_align_map=ok, record=info,
                   walk_us_by_difference=round(rows[0]["us_median"] - rows[1]["us_median"], 1))
    verified, rT, rrec = a.relocalizeMapChecked(pf, scan)
    rows[4].update(verified=verified, localize_accepted=rrec["localize"]["accepted"], aligned=rrec["aligned"], record=rrec["verify"],
                   error=[round(rT[j] - pose[j], 5) for j in range(3)])
    if n_beams == 360:
        rng = np.random.default_rng(9)
        for n in (64, 1000):
            particles = (np.arange(n, dtype=np.int32) % N).astype(np.int32)
            Ts = np.array(pose)[None, :] + rng.uniform(-1.0, 1.0, (n, 3)) * np.abs(np.array(OFF))[None, :]
            b_reps = max(reps // (1 if n < 1000 else 10), 3)
            t = [timed(lambda: a.verifyMapBatch(pf, Ts, scan, particles)) for _ in range(2 + b_reps)][2:]
            acc = [r["accepted"] for r in a.verifyMapBatch(pf, Ts, scan, particles)]
            st = stats(t)
            rows.append(dict(measure=f"batch_{n}", n_beams=n_beams, pairs=n, us_per_pair=round(st["us_median"] / n, 2), accepted=int(sum(acc)), **base, **st))
    a.close()
    for row in rows:
        results.append(row)
        print(json.dumps(row), flush=True)
pf.close()

out = dict(tool="tools/icp_verify_map_time.py", device=torch.cuda.get_device_name(0),
           clock="host clock round one synchronous call, device idle before and after",
           not_measured="the kernel and its stages between events (the walk is given by difference only); LDS use and occupancy", results=results)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
