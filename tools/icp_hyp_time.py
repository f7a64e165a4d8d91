#!/usr/bin/env python
"""What the global search's rival poses cost (include/tbnav_icp.h HYPOTHESES H1-H10, csrc/icp_hyp.hip behind csrc/icp_global.hip),
measured in ONE process on the bench room's map after 20 scans of the bench workload (device noise): at 400 x 400 with scans of 360 beams
and at 2000 x 2000 with 1080, 360 headings of one degree, pooling q = 3 and 4, the defaults otherwise, the scan taken at the best
particle's pose and NO guess given.  In the same loop, one after the other:

  localize_q<q>      tbnav_icp_localize_map from call to return by the host clock (median, p10-p90)
  hypotheses_q<q>    tbnav_icp_localize_map_hyp the same way, with floor_blocks, candidates, n_peaks and refined_blocks beside it
  checked_q<q>       relocalizeMapChecked whole (global search, one alignment, one check)
  rel_hyp_q<q>       relocalizeMapHypotheses whole (hypotheses, one alignment batch, one check batch), with how many were verified

Before anything is timed the hypotheses over a 64 x 64 region round the pose are compared with tests/icp_hyp_restatement.py.  NOT
measured: the kernels between events, and a corridor map where many blocks reach the floor.
  python tools/icp_hyp_time.py [--out FILE] [--reps N] [--quick]"""
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

pkg = g.load_package()
import bench_rbpf  # noqa: E402
import icp_global_restatement as G  # noqa: E402
import icp_hyp_restatement as H  # noqa: E402
import icp_restatement as R  # noqa: E402
import icp_search_restatement as S  # noqa: E402
import oracle_api as orc  # noqa: E402  (the synthetic room only: room_scan is numpy)
import rbpf_cases as rc  # noqa: E402
from rtn_amd import icp  # noqa: E402
from rtn_amd.rbpf import ParticleFilter, default_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--quick", action="store_true", help="a few repeats and the small map only")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
N_SCANS = 20


def stats(us):
    v = np.array(us)
    return dict(us_median=round(float(np.median(v)), 1), us_p10=round(float(np.percentile(v, 10)), 1), us_p90=round(float(np.percentile(v, 90)), 1),
                reps=len(v))


def err(T, pose):
    d = (T[0] - pose[0] + np.pi) % (2.0 * np.pi) - np.pi
    return [round(float(d), 4), round(T[1] - pose[1], 4), round(T[2] - pose[2], 4)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


results = []
cases = [("400x400", 10.0, 16, 360, 1.0, 5 if args.quick else args.reps)]
if not args.quick:
    cases.append(("2000x2000", 50.0, 4, 1080, 1.0 / 3.0, max(args.reps // 5, 5)))
steps, scans = bench_rbpf.workload(N_SCANS)
for name, half, N, n_beams, dd, reps in cases:
    pf = ParticleFilter(default_params(N=N, k=50, map_min=-half, map_max=half))
    pf.setSeed(2026)
    for s, (prev, cur, t_icp, u) in enumerate(steps):
        pf.SLAM(scans[s], u, cur, prev, True, t_icp, None)
    pose, best = pf.getRobotState()
    side = pf.xsize
    geom = G.Geom(-half, -half, 0.05, side)
    prm = icp.default_params(beam_delta_deg=dd)
    a = icp.ScanAlignment(prm)
    scan = orc.room_scan(pose, n_beams=n_beams, beam_delta_deg=dd, walls=rc.ROOM_BENCH, rng=np.random.default_rng(5))
    base = dict(case=name, side=side, n_beams=n_beams, headings=360, occupied_cells_of_best=int(pf.occupiedCount()[best]))
    # == before anything is timed, over a region round the pose (the occupancy as the filter reads it back)
    cx, cy = int((pose[1] + half) / 0.05), int((pose[2] + half) / 0.05)
    region = (cx - 32, cy - 32, cx + 31, cy + 31)
    occ = pf.occDist(best).reshape(side, side) == 0.0
    laser = R.Laser(prm.beam_min, prm.beam_max, prm.beam_delta, prm.range_min, prm.range_max)
    check = G.Params(region=region, ang_count=40, ang_step=np.pi / 20)
    want = H.localize_hyp(occ, geom, R.cloud(scan, laser)[0], S.Params(), check, H.HypParams(sep_steps=2))
    hyps, info = a.localizeMapHypotheses(pf, scan, hyp=dict(sep_steps=2), region=region, ang_count=check.ang_count, ang_step=check.ang_step)
    assert [(y["ia"], y["tx"], y["ty"], y["score"], y["T"]) for y in hyps] == [(y.ia, y.tx, y.ty, y.score, y.T) for y in want.hyps], (hyps, want.hyps)
    assert all(info[k] == v for k, v in want.info.items()), (info, want.info)
    for q in (3, 4):
        loc, hyp, chk, rel = [], [], [], []
        for rep in range(2 + reps):
            loc.append(timed(lambda: a.localizeMap(pf, scan, pool_log2=q)))
            hyp.append(timed(lambda: a.localizeMapHypotheses(pf, scan, pool_log2=q)))
            chk.append(timed(lambda: a.relocalizeMapChecked(pf, scan, localize=dict(pool_log2=q))))
            rel.append(timed(lambda: a.relocalizeMapHypotheses(pf, scan, localize=dict(pool_log2=q))))
        loc, hyp, chk, rel = loc[2:], hyp[2:], chk[2:], rel[2:]
        _, T, ginfo = a.localizeMap(pf, scan, pool_log2=q)
        hyps, info = a.localizeMapHypotheses(pf, scan, pool_log2=q)
        out = a.relocalizeMapHypotheses(pf, scan, localize=dict(pool_log2=q))
        ver, Tc, _ = a.relocalizeMapChecked(pf, scan, localize=dict(pool_log2=q))
        met = dict(blocks=info["blocks"], floor_blocks=info["floor_blocks"], refined_blocks=info["refined_blocks"], candidates=info["candidates"],
                   n_peaks=info["n_peaks"], n=info["n"], rounds=info["rounds"])
        rows = [dict(measure=f"localize_q{q}", pool_log2=q, **base, **stats(loc), refined_blocks=ginfo["refined_blocks"], error=err(T, pose)),
                dict(measure=f"hypotheses_q{q}", pool_log2=q, **base, **stats(hyp), **met, qualities=[round(y["quality"], 3) for y in hyps],
                     over_localize=round(float(np.median(hyp) / np.median(loc)), 3), kernels=a.lastHypKernels()),
                dict(measure=f"checked_q{q}", pool_log2=q, **base, **stats(chk), verified=bool(ver), error=err(Tc, pose)),
                dict(measure=f"rel_hyp_q{q}", pool_log2=q, **base, **stats(rel), **met, verified_count=out["verified_count"], best=out["best"],
                     ambiguous=out["ambiguous"], error=err(out["T"], pose), over_checked=round(float(np.median(rel) / np.median(chk)), 3))]
        for row in rows:
            results.append(row)
            print(json.dumps(row), flush=True)
    a.close(); pf.close()
    del a, pf

out = dict(tool="tools/icp_hyp_time.py", device=torch.cuda.get_device_name(0),
           clock="host clock round one synchronous call, device idle before and after; the four calls of a row group alternate in one loop",
           not_measured="the kernels between events; a corridor map where many blocks reach the floor", results=results)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
