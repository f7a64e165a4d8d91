#!/usr/bin/env python
"""What finding the robot anywhere in the filter's map costs (include/tbnav_icp.h GLOBAL SEARCH L1-L10, csrc/icp_global.hip), measured
in ONE process on the bench room's map after 20 scans of the bench workload (device noise): at 400 x 400 with scans of 360 beams and at
2000 x 2000 with 1080, 360 headings of one degree, pooling q = 2, 3 and 4, the scan taken at the best particle's pose and NO guess given:

  localize_q<q>   tbnav_icp_localize_map from call to return by the host clock (median, p10-p90), with refined_blocks and rounds beside
                  it; then tbnav_icp_localize_map_timed's stages, each kernel between two events on the handle's stream (medians)
  tiled_wide      the only route there was: tbnav_icp_search_map_batch with the wide stage at (64 cells, 180 steps, ALWAYS) over guesses
                  tiled across the map at a pitch of 129 cells, heading 0; the best pair is its answer (at 2000 x 2000 the 16
                  guesses of the row of tiles that holds the robot are timed and the time scaled to all 256).  Its table reaches 4 m round
                  each guess (M9), so it is not the same search: it is what a caller without the global search would have run.
A configuration the contract refuses (more than 2^26 blocks: q = 2 at 2000 x 2000 with 360 headings) is recorded as refused.  Before
anything is timed the result over a 64 x 64 region round the pose is compared with tests/icp_global_restatement.py.
  python tools/icp_global_time.py [--out FILE] [--reps N] [--quick]"""
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
N_SCANS, PITCH = 20, 129


def stats(us):
    v = np.array(us)
    return dict(us_median=round(float(np.median(v)), 1), us_p10=round(float(np.percentile(v, 10)), 1), us_p90=round(float(np.percentile(v, 90)), 1),
                reps=len(v))


def err(T, pose):
    """(heading wrapped to +-pi, x, y) of T - pose"""
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
    cases.append(("2000x2000", 50.0, 4, 1080, 1.0 / 3.0, max(args.reps // 10, 3)))
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
    check = G.Params(region=region) if side <= 400 else G.Params(region=region, ang_count=40, ang_step=np.pi / 20)   # (the host's time)
    want = G.localize(occ, geom, R.cloud(scan, laser)[0], S.Params(), check).info
    _, _, info = a.localizeMap(pf, scan, region=region, ang_count=check.ang_count, ang_step=check.ang_step)
    assert all(info[f] == getattr(want, f) for f in ("T", "score", "points", "occupied", "quality", "accepted", "blocks")), (info, want)
    for q in (2, 3, 4):
        row = dict(measure=f"localize_q{q}", pool_log2=q, **base)
        try:
            acc, T, info = a.localizeMap(pf, scan, pool_log2=q)
        except pkg.capi.TbnavError as e:
            row.update(refused=e.status, why="more than 2^26 blocks (L1)" if e.status == pkg.capi.ERR_UNSUPPORTED else str(e))
            results.append(row)
            print(json.dumps(row), flush=True)
            continue
        us = [timed(lambda: a.localizeMap(pf, scan, pool_log2=q)) for _ in range(2 + reps)][2:]
        stages = [a.localizeMapTimed(pf, scan, pool_log2=q)[3] for _ in range(1 + max(reps // 3, 3))][1:]
        row.update(stats(us))
        row.update(blocks=info["blocks"], refined_blocks=info["refined_blocks"], rounds=info["rounds"], quality=round(info["quality"], 3),
                   accepted=info["accepted"], error=err(T, pose),
                   kernel_us={k: round(float(np.median([st[k] for st in stages])) * 1e3, 1) for k in stages[0]}, kernels=a.lastGlobalKernels())
        results.append(row)
        print(json.dumps(row), flush=True)
    # the tiled route: the wide stage always, in the first stage's place, over guesses tiled across the map
    b = icp.ScanAlignment(prm, search=True, wide=dict(lin_cells=64, ang_steps=180, when="always"))
    centres = [min(c, side - 1) for c in range(64, side + 64, PITCH)]
    all_guesses = len(centres) ** 2
    if all_guesses > 64:
        # 16 x 16 guesses at 1080 beams are minutes of device time: the row of tiles that holds the robot is timed and scaled
        row_x = min(centres, key=lambda c: abs(c - cx))
        Ts = np.array([(0.0, -half + (row_x + 0.5) * 0.05, -half + (iy + 0.5) * 0.05) for iy in centres])
    else:
        Ts = np.array([(0.0, -half + (ix + 0.5) * 0.05, -half + (iy + 0.5) * 0.05) for ix in centres for iy in centres])
    particles = np.full(len(Ts), best, dtype=np.int32)
    t_reps = max(reps // 3, 3)
    got = b.searchMapBatch(pf, Ts, scan, particles)
    top = max(got, key=lambda r: r[2]["score"])
    us = [timed(lambda: b.searchMapBatch(pf, Ts, scan, particles)) for _ in range(1 + t_reps)][1:]
    scaled = {} if len(Ts) == all_guesses else dict(guesses_to_cover_the_map=all_guesses,
                                                   us_median_scaled_to_the_map=round(float(np.median(us)) * all_guesses / len(Ts), 1))
    row = dict(measure="tiled_wide", guesses=len(Ts), **scaled, pitch_cells=PITCH, window=(64, 180), **base, **stats(us), quality=round(top[2]["quality"], 3),
               accepted=top[2]["accepted"], error=err(top[1], pose))
    results.append(row)
    print(json.dumps(row), flush=True)
    a.close(); b.close(); pf.close()
    del a, b, pf

out = dict(tool="tools/icp_global_time.py", device=torch.cuda.get_device_name(0),
           clock="host clock round one synchronous call, device idle before and after; kernel_us between two events on the handle's stream",
           results=results)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
