"""Dev: randomized parity sweep of both hot paths against the oracle (run on the GPU box; not part of the suite).

usage: python tools/fuzz_parity.py [n_mppi] [n_rbpf] [seed] [only] [n_batch]
(n_batch: cases of the pipelined replay, tbnav_rbpf_slam_batch, against one synchronous call per scan — bit for bit)
Every case draws its own sizes, gains, start poses (incl. headings near +-pi), cell sizes, sensor offsets, sampling spreads,
gated beams, dynamics model, scan-matching on/off ...; the assertions are the test suite's.  Prints one line per
failing case with the parameters needed to reproduce it.
"""
import os, sys, traceback
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, __graft_entry__ as g
g.load_package()
import oracle_api as orc, rbpf_cases as rc
from cases import MPPI_BASE, WAYPOINTS, make_mppi, rel_err
from rtn_amd.rbpf import ParticleFilter, default_params

n_mppi = int(sys.argv[1]) if len(sys.argv) > 1 else 100
n_rbpf = int(sys.argv[2]) if len(sys.argv) > 2 else 60
seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
only = sys.argv[4] if len(sys.argv) > 4 else ""   # e.g. "mppi:97" to re-run one case verbosely
rng = None  # set per case from (seed, kind, index): any case can be re-run on its own


def mppi_case(i):
    global rng
    rng = np.random.default_rng([seed, 1, i])
    K = int(rng.choice([1, 3, 8, 9, 17, 64, 100, 257, 1024, 1500, 2049, 5000]))
    T = int(rng.choice([1, 2, 5, 25, 50, 63, 64, 65, 100, 127, 128, 129, 200, 300]))
    if K * T > 400000:
        T = max(1, 400000 // K)
    dyn = int(rng.integers(0, 2))
    d = dict(MPPI_BASE, rollouts=K, horizon=T * 0.01 + 0.004, lam=float(rng.choice([0.01, 0.1, 1.0])),
             ul_var=float(rng.uniform(0.05, 2.0)), ur_var=float(rng.uniform(0.05, 2.0)))
    desc = dict(K=K, T=T, dyn=dyn, lam=d["lam"])
    m = make_mppi(None, d)
    assert m.steps == orc.mppi_steps(d) == T, (m.steps, T)
    m.setDynamics("arc" if dyn else "rk4")
    xd = WAYPOINTS[int(rng.integers(0, 5))]
    m.setWaypoint(*xd)
    ui = (float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)))
    m.setInitialControls(*ui)
    u = np.zeros((2, T)); u[0] = ui[0]; u[1] = ui[1]
    x0 = (float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2)), float(rng.choice([rng.uniform(-3.2, 3.2), 3.1415, -3.1415, 0.0])))
    for tick in range(2):
        nz = orc.normal_stream(1000 * i + tick, K * T * 2, 0.0, 1.0).reshape(K, T, 2) * np.sqrt([d["ul_var"], d["ur_var"]])
        ref = orc.mppi_new_controls(d, u, ui, xd, x0, nz, dyn=dyn)
        got = m.newControls(*x0, nz)
        J = m.costToGo()
        ej = rel_err(J, ref["J"])
        assert ej < 1e-10, ("J", ej, desc)
        # the soft-min amplifies a relative error eps of J by J / lambda (J up to 1e7 here, lambda down to 0.01): the bar
        # is the north star's 1e-5 on the control vector, asserted at 1e-6
        assert np.allclose(got, ref["out"], rtol=1e-6, atol=1e-8), ("out", got, ref["out"], desc)
        uu = m.getControls()
        assert np.allclose(uu, ref["u"], rtol=1e-6, atol=1e-8), ("u", desc, "max abs diff", float(np.abs(uu - ref["u"]).max()), "J rel", ej,
                                                                   "J max", float(np.abs(ref["J"]).max()))
        u = ref["u"]
        x0 = (x0[0] + 0.003, x0[1] - 0.002, x0[2] + 0.004)
    m.close()


def rbpf_case(i):
    global rng
    rng = np.random.default_rng([seed, 2, i])
    N = int(rng.choice([1, 2, 5, 16, 33]))
    k = int(rng.choice([1, 2, 7, 20, 50, 70]))
    half = float(rng.choice([2.0, 3.0, 5.0]))
    bd = float(rng.choice([1.0, 1.0, 0.5, 2.0]))
    spread = float(rng.choice([1e-8, 1e-6, 1e-4, 1e-3]))
    trs = [float(rng.choice([0.0, rng.uniform(-0.4, 0.4)])), float(rng.uniform(-0.05, 0.05)), float(rng.uniform(-0.05, 0.05))]
    icp_ok = bool(rng.random() < 0.8)
    sm = bool(rng.random() < 0.25) and icp_ok
    mode = str(rng.choice(["query", "query", "window", "full"]))
    # the cell size: the shipped one, or one of tests/raycast_cases.py's RES_TABLE (its own stream: the other draws stay as they were);
    # create wants an even side: a half-extent that gives an odd one at the drawn size falls back to 2.0 m, which is even at all of them
    res = float(np.random.default_rng([seed, 6, i]).choice([0.05, 0.05, 0.0394, 0.0625, 0.07, 0.3, 0.5]))
    if int(np.ceil(2 * half / res)) % 2:
        half = 2.0
    assert int(np.ceil(2 * half / res)) % 2 == 0
    desc = dict(N=N, k=k, half=half, res=res, bd=bd, spread=spread, trs=trs, icp_ok=icp_ok, sm=sm, mode=mode)
    extra = dict(sample_range=[spread * 0.1, spread, spread], Trs=trs, resolution=res)
    n_beams = int(round(360 / bd))
    # the matcher in query mode: on half of those cases nothing is injected and the oracle reads the exact field itself (its own
    # stream: the other draws stay as they were) — the matcher's lookups then go through the bitmap query, not a stored array
    exact = sm and mode == "query" and bool(np.random.default_rng([seed, 5, i]).random() < 0.5)
    desc["exact"] = exact
    pf_o = orc.PfAPI(orc.pf_params(N=N, k=k, map_min=-half, map_max=half, beam_delta_deg=bd, **extra), exact_field=exact)
    pf_d = ParticleFilter(default_params(N=N, k=k, map_min=-half, map_max=half, beam_delta_deg=bd, **extra), df_mode=mode)
    band_rows = int(np.random.default_rng([seed, 3, i]).choice([0, 0, 3, 7, 20]))  # (its own stream: the other draws stay as they were)
    if band_rows:
        from rtn_amd import capi
        pf_d.setOption(capi.RBPF_OPT_RAYCAST_BAND_ROWS, band_rows)
    desc["band_rows"] = band_rows
    inc = (float(rng.uniform(-0.06, 0.06)), float(rng.uniform(0.01, 0.06)), float(rng.uniform(-0.04, 0.04)))
    steps, poses = rc.trajectory(4, inc=inc, start=(float(rng.uniform(-3.1, 3.1)), 0.0, 0.0))
    walls = (-1.2, 1.1, -1.0, 1.3)
    srng = np.random.default_rng(i)
    # compare against the oracle only on runs whose distance fields are injected from the first scan on: without that the
    # two filters legitimately drift apart (exact EDT vs the reference's brushfire) and so do their maps
    inject = ((mode == "query" and bool(rng.random() < 0.7)) or sm) and not exact
    for s, (prev, cur, t_icp, u) in enumerate(steps):
        scan = orc.room_scan(poses[s], n_beams=n_beams, beam_delta_deg=bd, walls=walls, rng=srng)
        if rng.random() < 0.3:
            scan[srng.integers(0, n_beams, 20)] = 9.0      # gated beams
        normals = orc.normal_stream(77 * i + s, pf_o.normals_per_scan(icp_ok), 0.0, 1.0)
        use_sm = sm and s >= 2
        pf_o.set_scan_matching(use_sm); pf_d.setScanMatching(use_sm)
        if inject:
            for p in range(N):
                pf_d.setOccDist(p, pf_o.grid(p).dump()["occ_dist"])
        tr_o = pf_o.slam(scan, u, cur, prev, icp_ok, t_icp, normals)
        try:
            st = pf_d.SLAM(scan, u, cur, prev, icp_ok, t_icp, normals)
        except Exception as e:  # the wrapper raises on a non-zero status: the oracle must have refused the same scan
            assert getattr(e, "status", None) == tr_o["rc"] != 0, ("status", getattr(e, "status", None), tr_o["rc"], desc)
            break
        assert st.status == 0 and tr_o["rc"] == 0, ("status", st.status, tr_o["rc"], desc)
        tr_d = pf_d.trace()
        # log-odds are bit-exact whenever the poses that drive the raycast agree; compare through the oracle grid
        po, _, wo = pf_o.particles(); pd, _, wd = pf_d.particles()
        if inject or use_sm or exact:
            # k = 2 or 3 samples give a rank-deficient covariance: its LLT stops at a pivot whose SIGN is rounding noise
            # (particle_filter.cpp:214 draws from it all the same), so the drawn pose is only reproducible to ~sqrt(eps)
            if k >= 4 or k == 1:
                assert np.allclose(pd, po, rtol=1e-9, atol=1e-13), ("pose", s, desc, np.abs(pd - po).max())
            assert np.allclose(wd, wo, rtol=1e-8 if k >= 4 or k == 1 else 1e-2), ("weight", s, desc)
            # Neff = (int)(1 / sum w^2) sits on a knife edge when the weights are (nearly) uniform: 1/sq within 1e-9 of an
            # integer can go either way on a last-bit difference of the weights — the reference's own fragility
            inv = 1.0 / tr_o["sq_sum"]
            if abs(inv - round(inv)) > 1e-9:
                assert (st.neff, st.resampled) == (tr_o["neff"], tr_o["resampled"]), ("neff", desc, st.sq_sum, tr_o["sq_sum"])
            if k >= 4 or k == 1:
                for p in range(N):
                    lo_d, lo_o = pf_d.logOdds(p), pf_o.grid(p).dump()["log_odds"]
                    if not np.array_equal(lo_d, lo_o):
                        bad = np.flatnonzero(lo_d != lo_o)
                        xs = pf_d.xsize
                        # which beam ends near the first differing cell, and how close to a cell border?
                        th, x, y = po[p]
                        ang = th + trs[0] + np.deg2rad(bd) * np.arange(n_beams)
                        c0, s0 = np.cos(th), np.sin(th)
                        X, Y = c0 * trs[1] - s0 * trs[2] + x, s0 * trs[1] + c0 * trs[2] + y
                        ex, ey = X + scan * np.cos(ang), Y + scan * np.sin(ang)
                        qx, qy = (ex + half) / res, (ey + half) / res
                        near = np.argsort(np.minimum(np.abs(qx - np.round(qx)), np.abs(qy - np.round(qy))))[:3]
                        print("   nearest-to-border beams:", [(int(b), float(scan[b]), float(qx[b]), float(qy[b])) for b in near])
                        raise AssertionError(("log-odds", s, p, desc, "cells", [(int(b // xs), int(b % xs), float(lo_d[b]), float(lo_o[b])) for b in bad[:8]], len(bad),
                                              "pose diff", (pd[p] - po[p]).tolist(), "pose", po[p].tolist()))
            else:
                pf_o.set_particles(pose=pd, w=wd)
        else:
            # exact EDT vs the reference brushfire: results differ legitimately; check invariants instead
            # (after a resampling the weights are the parents' — the reference does not reset them, particle_filter.cpp:495)
            assert (st.resampled or abs(wd.sum() - 1.0) < 1e-12) and np.all(np.isfinite(pd)), ("health", desc, repr(wd.sum()))
            pf_o.set_particles(pose=pd, w=wd)   # keep the oracle on the device's trajectory for the next scan
    pf_d.close(); pf_o.close()


def batch_case(i):
    """tbnav_rbpf_slam_batch (two scans in the stream, gated speculation, noise drawn a chunk ahead) against one synchronous
    tbnav_rbpf_slam per scan: same seed, same scans -> the same filter bit for bit, whatever resamples or fails on the way."""
    from rtn_amd import capi
    r = np.random.default_rng([seed, 4, i])
    N = int(r.choice([1, 7, 48, 64, 200]))
    k = int(r.choice([1, 5, 10, 30]))
    n_scans = int(r.choice([2, 3, 9, 12, 17, 20]))
    bd = float(r.choice([1.0, 1.0, 2.0]))
    n_beams = int(round(360 / bd))
    sharp = bool(r.random() < 0.6)  # a sharp sensor model and wide sampling: the run resamples by itself
    kw = dict(sigma_hit=float(r.choice([0.02, 0.03])), sample_range=[1e-5, float(r.choice([1e-4, 3e-4])), float(r.choice([1e-4, 3e-4]))]) if sharp else {}
    sm = bool(r.random() < 0.3)
    band_rows = int(r.choice([0, 0, 5, 12]))
    icp = (r.random(n_scans) < 0.85).astype(np.int32)
    split = int(r.integers(1, n_scans))  # the replay arrives as two batches
    desc = dict(N=N, k=k, n_scans=n_scans, bd=bd, sharp=sharp, sm=sm, band_rows=band_rows, icp=icp.tolist(), split=split)
    inc = (float(r.uniform(-0.05, 0.05)), float(r.uniform(0.01, 0.04)), float(r.uniform(-0.03, 0.03)))
    steps, poses = rc.trajectory(n_scans, inc=inc)
    srng = np.random.default_rng(1000 + i)
    scans = np.stack([orc.room_scan(poses[s], n_beams=n_beams, beam_delta_deg=bd, walls=rc.ROOM_SMALL, rng=srng) for s in range(n_scans)])
    if r.random() < 0.15:
        scans[int(r.integers(0, n_scans)), :] = 3.0  # a scan that leaves the +-2 m world: the replay stops there
    odom = np.array([steps[0][0]] + [st[1] for st in steps], dtype=np.float64)
    u = np.array([st[3] for st in steps], dtype=np.float64)
    t_icp = np.array([st[2] for st in steps], dtype=np.float64)
    pfs = [ParticleFilter(default_params(N=N, k=k, beam_delta_deg=bd, **kw)) for _ in range(2)]
    for pf in pfs:
        pf.setSeed(900 + i)
        if sm: pf.setScanMatching(True)
        if band_rows: pf.setOption(capi.RBPF_OPT_RAYCAST_BAND_ROWS, band_rows)
    one = []
    for s in range(n_scans):
        st = pfs[0].SLAM(scans[s], steps[s][3], steps[s][1], steps[s][0], bool(icp[s]), steps[s][2], None, check=False)
        one.append(st)
        if st.status != 0:
            break
    many = list(pfs[1].SLAMBatch(scans[:split], u[:split], odom[:split + 1], t_icp[:split], icp_ok=icp[:split], check=False))
    if all(o.status == 0 for o in many):
        many += list(pfs[1].SLAMBatch(scans[split:], u[split:], odom[split:], t_icp[split:], icp_ok=icp[split:], check=False))
    for s, x in enumerate(one):
        y = many[s]
        assert (x.status, x.n_valid_beams) == (y.status, y.n_valid_beams), ("status", s, x.status, y.status, desc)
        if x.status == 0:
            # (a sharp sensor model overflows the motion-model branch's product of 360 factors — inf / nan in both, as in the reference)
            assert np.array_equal([x.neff, x.resampled, x.sum_w, x.sq_sum], [y.neff, y.resampled, y.sum_w, y.sq_sum], equal_nan=True), \
                ("stats", s, (x.neff, x.resampled, x.sum_w, x.sq_sum), (y.neff, y.resampled, y.sum_w, y.sq_sum), desc)
    if one[-1].status == 0:
        a, b = pfs[0].particles(), pfs[1].particles()
        for q in range(3):
            assert np.array_equal(a[q], b[q], equal_nan=True), ("particles", q, desc)
        for m in sorted(set([0, N // 2, N - 1])):
            assert np.array_equal(pfs[0].logOdds(m), pfs[1].logOdds(m)), ("log-odds", m, desc)
        assert pfs[0].poolStats() == pfs[1].poolStats(), ("pool", desc)
    for pf in pfs:
        pf.close()
    return sum(o.resampled for o in one)


n_batch = int(sys.argv[5]) if len(sys.argv) > 5 else 0
fails = 0
events = 0
for name, fn, n in (("mppi", mppi_case, n_mppi), ("rbpf", rbpf_case, n_rbpf), ("batch", batch_case, n_batch)):
    for i in range(n):
        if only and only != f"{name}:{i}":
            continue
        try:
            ret = fn(i)
            if isinstance(ret, (int, np.integer)):
                events += int(ret)
        except Exception as e:  # noqa: BLE001
            fails += 1
            print(f"[FAIL] {name} case {i} (seed {seed}): {type(e).__name__}: {str(e)[:600]}")
            if fails <= 3:
                traceback.print_exc(limit=2)
    print(f"{name}: {n} cases done, failures so far {fails}" + (f" ({events} scans resampled on the way)" if name == "batch" and n else ""), flush=True)
sys.exit(1 if fails else 0)
