"""Dev: randomized sweep of the device ICP (include/tbnav_icp.h, csrc/icp.hip) against the numpy restatements
(tests/icp_restatement.py, tests/icp_line_restatement.py), bit for bit (run on the GPU box; tests/test_icp_fuzz_gpu.py runs a
bounded sweep from a fixed seed inside the suite).

usage: python tools/fuzz_icp.py [n_cases] [seed] [case]      (case: re-run that one case alone, verbosely)
Every case draws its beam count (1 ... 4096, half of the draws k * 256 + {-1, 0, 1}), metric, laser, valid fraction, kind of
scan (a room pair; a wrapped-ray pair with exact distance ties; one target point), Trs, max_corr_dist, both epsilons, max_iter
and the error of its guess from (seed, case), and goes through tbnav_icp_match twice (the second run must give the same bits);
every fourth also runs six scans through tbnav_icp_step_batch against the restatement's wrapper.  Prints one line per failing
case with what is needed to reproduce it, and one summary line with the totals: cases per instantiation and per criterion,
cases that held ties.
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
import oracle_api as orc
from rtn_amd import icp

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
only = int(sys.argv[3]) if len(sys.argv) > 3 else -1

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


fails = 0
t0 = time.perf_counter()
for i in range(n_cases):
    if only >= 0 and i != only:
        continue
    try:
        one_case(i, verbose=only >= 0)
    except Exception as e:  # noqa: BLE001
        fails += 1
        print(f"[FAIL] icp case {i} (seed {seed}; replay: python tools/fuzz_icp.py {n_cases} {seed} {i}): {type(e).__name__}: {str(e)[:900]}")
        if fails <= 3:
            traceback.print_exc(limit=2)
for k in ("point_P", "line_P", "criterion"):
    totals[k] = dict(sorted(totals[k].items()))
print(f"icp: {n_cases} cases done, failures so far {fails}; {totals}", flush=True)
print(f"icp: wall time {time.perf_counter() - t0:.1f} s", flush=True)
sys.exit(1 if fails else 0)
