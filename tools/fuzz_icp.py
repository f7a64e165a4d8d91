"""Dev: randomized sweep of the device ICP (include/tbnav_icp.h, csrc/icp.hip) against the numpy restatements
(tests/icp_restatement.py, tests/icp_line_restatement.py), bit for bit (run on the GPU box; tests/test_icp_fuzz_gpu.py runs a
bounded sweep from a fixed seed inside the suite).

usage: python tools/fuzz_icp.py [--shape] [n_cases] [seed] [case]      (case: re-run that one case alone, verbosely)
Every case draws its beam count (1 ... 4096, half of the draws k * 256 + {-1, 0, 1}), metric, laser, valid fraction, kind of
scan (a room pair; a wrapped-ray pair with exact distance ties; one target point), Trs, max_corr_dist, both epsilons, max_iter
and the error of its guess from (seed, case), and goes through tbnav_icp_match twice (the second run must give the same bits);
every fourth also runs six scans through tbnav_icp_step_batch against the restatement's wrapper.  Prints one line per failing
case with what is needed to reproduce it, and one summary line with the totals: cases per instantiation and per criterion,
cases that held ties.

--shape: the sweep of the shape of the correlative search's score volume instead (include/tbnav_icp.h, items F1-F6;
csrc/icp_search_shape.hip) against tests/icp_search_shape_restatement.py with ==: every case draws a room or a corridor at a
random heading and width, the robot's step, the error of the guess, the window, slack_q10, drop_q10 and flat_cells2
(draw_shape), goes through tbnav_icp_search_with_shape, and every third through tbnav_icp_match with the search, the shape and
the line metric on.  The summary line counts the cases per kind.  tests/test_icp_search_shape_fuzz_gpu.py imports draw_shape.
"""
import math
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g
g.load_package()
import icp_cases as ic
import icp_line_restatement as LR
import icp_restatement as R
import icp_search_restatement as S
import icp_search_shape_restatement as F
import oracle_api as orc
from rtn_amd import icp

n_cases, seed, only = 200, 0, -1     # set by main()

totals = dict(point_P={}, line_P={}, criterion={}, with_ties=0, batches=0, matches=0)


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64).tolist()


def _same(got, want, where):
    ok, T, info = got
    have = (ok, info["iterations"], info["criterion"], info["correspondences"], _bits(info["mse"]), _bits(T))
    need = (want.ok, want.iterations, want.criterion, want.correspondences, _bits(want.mse), _bits(want.T))
    assert have == need, (where, "kernel", got, "restatement", want)


def _count(d, key):
    d[key] = d.get(key, 0) + 1


def draw(i):
    r = np.random.default_rng([seed, 5, i])
    if r.random() < 0.5:
        n = int(np.clip(256 * int(r.integers(1, 17)) + int(r.integers(-1, 2)), 1, ic.MAX_BEAMS))
    else:
        n = int(r.integers(1, ic.MAX_BEAMS + 1))
    metric = "line" if r.random() < 0.4 and n <= LR.MAX_BEAMS else "point"
    kind = str(r.choice(["room", "room", "room", "rays", "rays", "one_point"]))
    if kind == "rays" and n < 2 * 135:
        kind = "room"
    kw = dict(max_corr_dist=float(r.uniform(0.05, 2.0)), max_iter=int(r.choice([1, 2, 30, 100])))
    te, fe = float(r.choice([0.0, 1e-14, 1e-8])), float(r.choice([0.0, 1e-14, 1e-6]))
    kw.update(transform_eps=te, fitness_eps=fe)
    if n > 2048 and te == 0.0 and fe == 0.0:
        kw["max_iter"] = min(kw["max_iter"], 30)       # (the restatement's time on the CPU)
    if r.random() < 0.5 and kind != "one_point":
        kw["Trs"] = (float(r.uniform(-0.4, 0.4)), float(r.uniform(-0.05, 0.05)), float(r.uniform(-0.05, 0.05)))
    frac = float(r.choice([1.0, 1.0, 0.9, 0.5, 0.05]))
    err = (float(r.uniform(-1, 1)) * math.radians(10.0), float(r.uniform(-0.3, 0.3)), float(r.uniform(-0.3, 0.3)))
    if kind == "room":
        bd = float(r.choice([360.0 / max(n, 4), 1.0]))
        kw["beam_delta_deg"] = bd
        motion = (float(r.uniform(-0.05, 0.05)), float(r.uniform(-0.08, 0.08)), float(r.uniform(-0.08, 0.08)))
        walls = ic.UNIT_ROOM if r.random() < 0.3 else (-2.2, 2.2, -2.0, 2.0)
        srng = np.random.default_rng([seed, 6, i])
        tgt = orc.room_scan((0.0, 0.0, 0.0), n_beams=n, beam_delta_deg=bd, walls=walls, rng=srng)
        src = orc.room_scan(motion, n_beams=n, beam_delta_deg=bd, walls=walls, rng=srng)
        T = tuple(m + e * float(r.choice([0.0, 0.1, 1.0])) for m, e in zip(motion, err))
    elif kind == "rays":
        bd, W = (1.0, 361) if n >= 2 * 361 and r.random() < 0.7 else (8.0 / 3.0, 135)
        kw["beam_delta_deg"] = bd
        tgt, src = ic.tie_scans(n, W, seed=int(r.integers(0, 1 << 30)))
        T = (0.0, 0.0, 0.0) if r.random() < 0.6 else tuple(0.1 * e for e in err)
    else:
        tgt = np.full(n, ic.NAN, dtype=np.float32)
        src = np.full(n, ic.NAN, dtype=np.float32)
        tgt[0] = 1.0
        k = min(n, int(r.integers(1, 7)))
        src[:k] = (1.0 + r.integers(-3, 4, k) / 16.0).astype(np.float32)
        T = (0.0, 0.0, 0.0)
    if frac < 1.0 and kind != "one_point":
        tgt = np.where(r.random(n) < frac, tgt, ic.NAN).astype(np.float32)
        src = np.where(r.random(n) < frac, src, ic.NAN).astype(np.float32)
    return ic.Case(f"fuzz{i}", kw, tgt.astype(np.float32), src.astype(np.float32), T), metric, kind, frac, r


def one_case(i, verbose=False):
    case, metric, kind, frac, r = draw(i)
    n = case.tgt.size
    desc = dict(case=i, seed=seed, n_beams=n, metric=metric, kind=kind, frac=frac, T=case.T, **case.kw)
    if verbose:
        print(desc)
    P = ic.beams_per_thread(n, metric)
    a = icp.ScanAlignment(icp.default_params(**case.kw), metric=metric)
    try:
        want = ic.restate(case, metric)
        got = a.pclICP(case.T, case.tgt, case.src)
        if verbose:
            print("kernel", got, "\nrestatement", want)
        _same(got, want, ("match", desc))
        again = a.pclICP(case.T, case.tgt, case.src)
        assert (again[0], _bits(again[1]), again[2]) == (got[0], _bits(got[1]), got[2]), ("second run", desc, got, again)
        _count(totals["point_P" if metric == "point" else "line_P"], P)
        _count(totals["criterion"], want.criterion)
        totals["matches"] += 1
        if kind == "rays" and tuple(case.T) == (0.0, 0.0, 0.0) and ic.count_ties(case, ic.chains(P))[0] > 0:
            totals["with_ties"] += 1
        if i % 4 == 0:
            # six scans as a logged run: the pair, the pair again the other way round, an all-invalid scan, the target twice
            scans = np.stack([case.tgt, case.src, case.tgt, np.full(n, ic.NAN, dtype=np.float32), case.src, case.src])
            back = (-case.T[0], -case.T[1], -case.T[2])
            T_init = np.array([(0.0, 0.0, 0.0), case.T, back, (0.0, 0.0, 0.0), case.T, (0.0, 0.0, 0.0)])
            ok, T, info = a.wrapperBatch(T_init, scans)
            w = LR.Wrapper(ic.laser(case.kw), tuple(case.kw.get("Trs", (0.0, 0.0, 0.0))), metric=metric,
                           **{k: v for k, v in ic.ref_kw(case.kw).items() if k != "Trs"})
            for s in range(len(scans)):
                with np.errstate(all="ignore"):
                    ws = w.step(scans[s], T_init[s])
                _same((bool(ok[s]), tuple(T[s]), info[s]), ws, ("batch", s, desc))
                _count(totals["criterion"], ws.criterion)
            totals["batches"] += 1
    finally:
        a.close()


SHAPE_FIELDS = ("resolution", "half_extent", "sigma", "ang_step", "min_quality", "stamp_cells", "lin_cells", "ang_steps", "slack_q10")
shape_totals = dict(kind={}, accepted=0, matches=0)


def draw_shape(i, seed):
    """case i of the --shape sweep -> (target scan, source scan, search Params, ShapeParams, guess, "room" | "corridor")"""
    r = np.random.default_rng([seed, 7, i])
    scene = "corridor" if r.random() < 0.5 else "room"
    if scene == "corridor":
        half = float(r.uniform(0.7, 1.3))
        walls = (-50.0, 50.0, -half, half)
        th = float(r.uniform(-math.pi, math.pi))
        p0 = (th, 0.0, float(r.uniform(-0.2, 0.2)))
        p1 = (th + float(r.normal(0, 0.01)), float(r.uniform(-0.15, 0.15)), p0[2] + float(r.normal(0, 0.01)))
    else:
        walls = (-2.2, 2.2, -2.0, 2.0) if r.random() < 0.5 else (-3.0, 3.0, -2.5, 2.5)
        p0 = (float(r.uniform(-math.pi, math.pi)), float(r.uniform(-0.3, 0.3)), float(r.uniform(-0.3, 0.3)))
        p1 = (p0[0] + float(r.normal(0, 0.05)), p0[1] + float(r.uniform(-0.1, 0.1)), p0[2] + float(r.uniform(-0.1, 0.1)))
    srng = np.random.default_rng([seed, 8, i])
    tgt = orc.room_scan(p0, walls=walls, rng=srng)
    src = orc.room_scan(p1, walls=walls, rng=srng)
    c, sn = math.cos(p0[0]), math.sin(p0[0])                   # the truth in the target scan's frame
    dx, dy = p1[1] - p0[1], p1[2] - p0[2]
    truth = (p1[0] - p0[0], c * dx + sn * dy, -sn * dx + c * dy)
    e = float(r.choice([0.0, 0.5, 1.0]))
    guess = (truth[0] + e * float(r.normal(0, 0.03)), truth[1] + e * float(r.normal(0, 0.1)), truth[2] + e * float(r.normal(0, 0.1)))
    sp = S.Params(lin_cells=int(r.choice([3, 6, 6, 6, 10, 16])), ang_steps=int(r.choice([0, 5, 20])),
                  slack_q10=int(r.choice([0, 0, 0, 32, 64])), stamp_cells=int(r.choice([3, 3, 5])))
    fp = F.ShapeParams(drop_q10=int(r.choice([64, 256, 256, 256, 512, 1023])), flat_cells2=float(r.choice([0.5, 2.0, 2.0, 2.0, 4.0])))
    return tgt, src, sp, fp, guess, scene


def shape_case(i, verbose=False):
    tgt, src, sp, fp, guess, scene = draw_shape(i, seed)
    desc = dict(case=i, seed=seed, scene=scene, guess=guess, search=sp, shape=fp)
    if verbose:
        print(desc)
    p = icp.default_params()
    L = R.Laser(p.beam_min, p.beam_max, p.beam_delta, p.range_min, p.range_max)
    a = icp.ScanAlignment(p, metric="line", search={f: getattr(sp, f) for f in SHAPE_FIELDS},
                          shape=dict(drop_q10=fp.drop_q10, flat_cells2=fp.flat_cells2))
    try:
        want, wsh = F.search(tgt, src, L, guess, sp, fp)
        acc, T, info, sh = a.searchWithShape(guess, tgt, src)
        if verbose:
            print("kernel", info, sh, "\nrestatement", want, wsh)
        for f in ("T", "quality", "score", "points", "candidates", "ia", "iy", "ix", "at_edge", "accepted", "searched"):
            assert info[f] == getattr(want, f), (f, desc, info, want)
        for f in ("S0", "Sx", "Sy", "Sxx", "Sxy", "Syy", "l1", "l2", "ex", "ey", "T_raw", "cells", "kind", "computed"):
            assert sh[f] == getattr(wsh, f), (f, desc, sh, wsh)
        assert acc == bool(want.accepted) and T == want.T, desc
        _count(shape_totals["kind"], wsh.kind)
        shape_totals["accepted"] += want.accepted
        if i % 3 == 0:
            res, _, _ = F.match(tgt, src, L, guess, sp, fp, icp=LR.match, found=(want, wsh))
            _same(a.pclICP(guess, tgt, src), res, ("match", desc))
            assert a.lastSearchShape() == sh, desc
            shape_totals["matches"] += 1
    finally:
        a.close()


def main():
    global n_cases, seed, only
    args = [v for v in sys.argv[1:] if v != "--shape"]
    shape = "--shape" in sys.argv[1:]
    n_cases = int(args[0]) if len(args) > 0 else 200
    seed = int(args[1]) if len(args) > 1 else 0
    only = int(args[2]) if len(args) > 2 else -1
    flag = "--shape " if shape else ""
    fails = 0
    t0 = time.perf_counter()
    for i in range(n_cases):
        if only >= 0 and i != only:
            continue
        try:
            (shape_case if shape else one_case)(i, verbose=only >= 0)
        except Exception as e:  # noqa: BLE001
            fails += 1
            print(f"[FAIL] icp case {i} (seed {seed}; replay: python tools/fuzz_icp.py {flag}{n_cases} {seed} {i}): {type(e).__name__}: {str(e)[:900]}")
            if fails <= 3:
                traceback.print_exc(limit=2)
    for k in ("point_P", "line_P", "criterion"):
        totals[k] = dict(sorted(totals[k].items()))
    print(f"icp: {n_cases} cases done, failures so far {fails}; {shape_totals if shape else totals}", flush=True)
    print(f"icp: wall time {time.perf_counter() - t0:.1f} s", flush=True)
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
