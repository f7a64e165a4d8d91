"""Timing of the device ICP (include/tbnav_icp.h) on the GPU:
python tools/icp_time.py [--out FILE] [--quick] [--metric point|line|both] [--max-iter N] [--search] [--shape] [--wide [--when W]]
  - latency of one synchronous tbnav_icp_step (host clock around the call, which ends in a stream synchronise) at 360 beams
    (1 deg) and 1080 beams (1/3 deg): median / p10 / p90 of 500 scans after 20 of warm-up, a robot driving round a room;
  - tbnav_icp_step_batch over 2000 scans of the same kind of run: median of 5 calls (after one of warm-up), per call and
    per scan, with the launches it made;
  --metric: the point metric (default), the line metric (tbnav_icp_set_metric, default window and gap), or both: the two are then
    timed in the same process on the same scans, each record under its metric's name with its mean iteration count, and
    "line_over_point" holds the ratios of the medians and of the iteration counts;
  --max-iter: tbnav_icp_params.max_iter (default 100, the reference's): a launch of step_batch lasts as long as its slowest
    pair, so a pair that runs to the cap sets the batch's time;
  --search: the correlative search in front of the ICP (tbnav_icp_set_search, default parameters), in the same process on the
    same scans: every record above with the search off (the parent's rows) and again with it on under "<name>_search", and
    "search_alone_360" / "_1080": tbnav_icp_search by itself on consecutive scans of the same run;
  --shape (with --search): the shape of the search's score volume on top of the search (tbnav_icp_set_search_shape, default
    parameters), in the same process on the same scans: every "<name>_search" record again under "<name>_search_shape", and
    "search_shape_alone_360" / "_1080": tbnav_icp_search with the shape on; "shape_over_search" holds the differences of the
    medians (what the shape adds);
  --wide (with --search): the search's wide second stage (tbnav_icp_set_search_wide, default window, --when reject |
    reject_or_edge | always, default reject), in the same process on the same scans: every "<name>_search" record again under
    "<name>_search_wide" (with the robot's good guesses and `reject` the wide stage never runs: "wide_ran" counts), and
    "wide_over_search" holds the differences of the medians; "wide_alone_<W>_<A>_<beams>": tbnav_icp_search with when = always
    (the wide stage's own cost, the table included) at (W, A) = (48, 45), (64, 20), (64, 180), with its ratio to
    "search_alone_<beams>"; "escalated_step_360" / "_1080": tbnav_icp_step with every guess slipped by 1.6 m (first stage
    rejected, wide stage, ICP) as one wall time;
  --quick: a few scans only (what a `rocprofv3 --kernel-trace --stats` run of this script needs).
Kernel times come from a separate rocprofv3 run, not from this script."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402

g.load_package()
import oracle_api as orc  # noqa: E402  (the synthetic room only: room_scan is numpy)
import rbpf_cases as rc  # noqa: E402
from rtn_amd import icp  # noqa: E402


def loop_run(n, n_beams, beam_delta_deg, seed=1):
    """a robot driving an ellipse in ROOM_BENCH, 500 scans per lap: poses (theta, x, y) and LDS-01-like scans"""
    phi = 2 * math.pi * np.arange(n) / 500.0
    poses = np.stack([phi + math.pi / 2, 1.0 * np.cos(phi), 0.8 * np.sin(phi)], axis=1)
    rng = np.random.default_rng(seed)
    scans = np.stack([orc.room_scan(p, n_beams=n_beams, beam_delta_deg=beam_delta_deg, walls=rc.ROOM_BENCH, rng=rng) for p in poses])
    T_init = np.array([icp.init_guess(poses[s], poses[s - 1] if s else poses[0]) for s in range(n)])
    return scans, T_init


def step_latency(n_beams, beam_delta_deg, n_warm, n_time, metric="point", max_iter=100, search=None, shape=None, wide=None, slip=0.0):
    a = icp.ScanAlignment(icp.default_params(beam_delta_deg=beam_delta_deg, max_iter=max_iter), metric=metric, search=search, shape=shape,
                          wide=wide)
    scans, T_init = loop_run(n_warm + n_time, n_beams, beam_delta_deg)
    T_init[1:, 1] += slip                                      # every guess off by `slip` metres in x
    ts, iters, fails, accepted, ran = [], [], 0, 0, 0
    for s in range(n_warm + n_time):
        t0 = time.perf_counter()
        ok, T, info = a.pclICPWrapper(T_init[s], scans[s])
        t1 = time.perf_counter()
        if s >= n_warm:
            ts.append((t1 - t0) * 1e6)
            iters.append(info["iterations"])
            fails += 0 if ok else 1
            accepted += a.lastSearch()["accepted"] if search else 0
            ran += a.lastSearchWide()["ran"] if wide else 0
    a.close()
    ts = np.array(ts)
    rec = dict(n_beams=n_beams, scans=n_time, median_us=float(np.median(ts)), p10_us=float(np.percentile(ts, 10)),
               p90_us=float(np.percentile(ts, 90)), mean_iterations=float(np.mean(iters)), max_iterations=int(np.max(iters)),
               at_max_iter=int(np.sum(np.array(iters) >= max_iter)), failures=fails)
    if search:
        rec["searches_accepted"] = accepted
    if wide:
        rec["wide_ran"] = ran
    return rec


def search_latency(n_beams, beam_delta_deg, n_warm, n_time, shape=None, wide=None):
    """tbnav_icp_search alone (default parameters): each scan of the run against the one before it"""
    a = icp.ScanAlignment(icp.default_params(beam_delta_deg=beam_delta_deg), shape=shape, wide=wide)
    scans, T_init = loop_run(n_warm + n_time + 1, n_beams, beam_delta_deg)
    ts, acc, qual = [], 0, []
    for s in range(1, n_warm + n_time + 1):
        t0 = time.perf_counter()
        ok, T, info = a.search(T_init[s], scans[s - 1], scans[s])
        t1 = time.perf_counter()
        if s > n_warm:
            ts.append((t1 - t0) * 1e6)
            acc += int(ok)
            qual.append(info["quality"])
    a.close()
    ts = np.array(ts)
    return dict(n_beams=n_beams, scans=n_time, median_us=float(np.median(ts)), p10_us=float(np.percentile(ts, 10)),
                p90_us=float(np.percentile(ts, 90)), accepted=acc, mean_quality=float(np.mean(qual)))


def batch_time(n_scans, reps, n_beams=360, beam_delta_deg=1.0, metric="point", max_iter=100, search=None, shape=None, wide=None):
    a = icp.ScanAlignment(icp.default_params(beam_delta_deg=beam_delta_deg, max_iter=max_iter), metric=metric, search=search, shape=shape,
                          wide=wide)
    scans, T_init = loop_run(n_scans, n_beams, beam_delta_deg, seed=2)
    ts = []
    for r in range(reps + 1):
        a.reset()
        t0 = time.perf_counter()
        ok, T, info = a.wrapperBatch(T_init, scans)
        t1 = time.perf_counter()
        if r > 0:
            ts.append((t1 - t0) * 1e3)
    launches = a.lastBatchLaunches()
    a.close()
    med = float(np.median(ts))
    return dict(n_beams=n_beams, scans=n_scans, median_ms=med, min_ms=float(np.min(ts)), per_scan_us=med * 1e3 / n_scans,
                launches=launches, failures=int(n_scans - ok.sum()), mean_iterations=float(np.mean([i["iterations"] for i in info[1:]])),
                max_iterations=int(np.max([i["iterations"] for i in info[1:]])),
                at_max_iter=int(np.sum([i["criterion"] == 1 for i in info[1:]])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--metric", choices=("point", "line", "both"), default="point")
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--shape", action="store_true")
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--when", choices=("reject", "reject_or_edge", "always"), default="reject")
    a = ap.parse_args()
    if a.shape and not a.search:
        ap.error("--shape measures what it adds to the search: give --search too")
    if a.wide and not a.search:
        ap.error("--wide measures what it adds to the search: give --search too")
    n_warm, n_time, reps = (2, 10, 1) if a.quick else (20, 500, 5)

    def run(metric):
        res = dict(step_360=step_latency(360, 1.0, n_warm, n_time, metric, a.max_iter),
                   step_1080=step_latency(1080, 1.0 / 3.0, n_warm, n_time, metric, a.max_iter),
                   batch_2000=batch_time(2000, reps, metric=metric, max_iter=a.max_iter))
        if a.search:
            res.update(step_360_search=step_latency(360, 1.0, n_warm, n_time, metric, a.max_iter, search=True),
                       step_1080_search=step_latency(1080, 1.0 / 3.0, n_warm, n_time, metric, a.max_iter, search=True),
                       batch_2000_search=batch_time(2000, reps, metric=metric, max_iter=a.max_iter, search=True))
        if a.shape:
            res.update(step_360_search_shape=step_latency(360, 1.0, n_warm, n_time, metric, a.max_iter, search=True, shape=True),
                       step_1080_search_shape=step_latency(1080, 1.0 / 3.0, n_warm, n_time, metric, a.max_iter, search=True, shape=True),
                       batch_2000_search_shape=batch_time(2000, reps, metric=metric, max_iter=a.max_iter, search=True, shape=True))
            res["shape_over_search"] = {key: res[key + "_search_shape"][t] - res[key + "_search"][t]
                                        for key, t in (("step_360", "median_us"), ("step_1080", "median_us"), ("batch_2000", "median_ms"))}
        if a.wide:
            w = dict(when=a.when)
            res.update(step_360_search_wide=step_latency(360, 1.0, n_warm, n_time, metric, a.max_iter, search=True, wide=w),
                       step_1080_search_wide=step_latency(1080, 1.0 / 3.0, n_warm, n_time, metric, a.max_iter, search=True, wide=w),
                       batch_2000_search_wide=batch_time(2000, reps, metric=metric, max_iter=a.max_iter, search=True, wide=w),
                       escalated_step_360=step_latency(360, 1.0, n_warm, n_time, metric, a.max_iter, search=True, wide=w, slip=1.6),
                       escalated_step_1080=step_latency(1080, 1.0 / 3.0, n_warm, n_time, metric, a.max_iter, search=True, wide=w, slip=1.6))
            res["wide_over_search"] = {key: res[key + "_search_wide"][t] - res[key + "_search"][t]
                                       for key, t in (("step_360", "median_us"), ("step_1080", "median_us"), ("batch_2000", "median_ms"))}
        return res

    if a.metric == "both":
        res = dict(point=run("point"), line=run("line"))
        res["line_over_point"] = {
            key: dict(time=res["line"][key][t] / res["point"][key][t],
                      iterations=res["line"][key]["mean_iterations"] / res["point"][key]["mean_iterations"])
            for key, t in (("step_360", "median_us"), ("step_1080", "median_us"), ("batch_2000", "median_ms"))}
    else:
        res = run(a.metric)
    if a.search:
        res["search_alone_360"] = search_latency(360, 1.0, n_warm, n_time)
        res["search_alone_1080"] = search_latency(1080, 1.0 / 3.0, n_warm, n_time)
    if a.shape:
        res["search_shape_alone_360"] = search_latency(360, 1.0, n_warm, n_time, shape=True)
        res["search_shape_alone_1080"] = search_latency(1080, 1.0 / 3.0, n_warm, n_time, shape=True)
    if a.wide:
        for lin, ang in ((48, 45), (64, 20), (64, 180)):
            for n_beams, dd in ((360, 1.0), (1080, 1.0 / 3.0)):
                rec = search_latency(n_beams, dd, n_warm, n_time if ang < 180 else max(n_time // 5, 5),
                                     wide=dict(lin_cells=lin, ang_steps=ang, when="always"))
                rec["over_search_alone"] = rec["median_us"] / res["search_alone_%d" % n_beams]["median_us"]
                res["wide_alone_%d_%d_%d" % (lin, ang, n_beams)] = rec
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
