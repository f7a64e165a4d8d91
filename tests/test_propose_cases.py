"""The proposal kernel's case table (tests/propose_cases.py) on the CPU, with the oracle alone: the restated host expressions are
csrc/rbpf.hip's and give the instantiation each case names; every case reaches what it is there for (unstable counts by the kernel's
own rule, empty segments, staging forms, settled and unsettled lookups, tiers, statuses); the rule's premise holds (a beam some sample
moves out of the centre's cell is never called stable); the two rotation cases can tell the rule from its mutants; and no end point
of any case lies so near a cell border that the device's other rounding could put it in the neighbouring cell.  No device."""
import os
import re
import time

import numpy as np
import pytest

import propose_cases as pc
import rbpf_cases as rc
import scanmatch_cases as smc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "csrc")
STATUS_OUT_OF_WORLD, STATUS_ETA_ZERO = 4, 5


def _analyse(c, kind, pf, sc, before, after, occ, tr):
    """One scan of one oracle run, per particle: the restated kernel rules over the oracle's numbers."""
    lookups = c.group in ("lookups", "res")
    half = pc.occ_half(c, "query")
    Bv = pc.n_valid(c, sc.scan)
    row = dict(s=sc.s, rc=tr["rc"], Bv=Bv, icp_ok=sc.icp_ok, nocc=[len(o) for o in occ], border=np.inf, parts=[], eta=tr["eta"].copy(),
               p_scan=tr["p_scan"].copy(), resampled=tr["resampled"], nt=pc.threads(c.k, Bv, pc.slice_bytes(c, "query")))
    stride = 3 * c.k + 3 if sc.icp_ok else 3
    for p in range(c.N):
        g = pf.grid(p)
        part = dict()
        if sc.icp_ok:
            centre = rc.compose(before[p], sc.guess)
            z = sc.normals[p * stride:p * stride + 3 * c.k].reshape(c.k, 3)
            if tr["rc"] == 0:
                samples = tr["sampled"][p]
                raw = centre[None] + np.sqrt(np.array(c.var))[None] * z
                assert np.allclose(samples[:, 1:], raw[:, 1:], rtol=0, atol=1e-13), (c.id, sc.s, p)
                assert np.allclose(np.cos(samples[:, 0]), np.cos(raw[:, 0]), rtol=0, atol=1e-12), (c.id, sc.s, p)
            else:   # (the oracle stopped at its first throw: the trace is not whole; no case of this kind has a heading near pi)
                samples = centre[None] + np.sqrt(np.array(c.var))[None] * z
                assert abs(centre[0]) < 1.0
            z_theta = z[:, 0]
        else:
            centre, samples, z_theta = after[p], np.zeros((0, 3)), np.zeros(0)
        cxy = g.end_points(sc.scan, centre)
        assert cxy.shape == (Bv, 2), (c.id, sc.s, cxy.shape, Bv)
        sxy = np.stack([g.end_points(sc.scan, sj) for sj in samples]) if len(samples) else np.zeros((0, Bv, 2))
        part["centre_inside"] = bool(pc.inside(c, cxy).all())
        part["samples_inside"] = bool(pc.inside(c, sxy).all())
        part["theta_signs"] = (bool((samples[:, 0] > 0).any()), bool((samples[:, 0] < 0).any())) if len(samples) else (False, False)
        for xy in (cxy, sxy.reshape(-1, 2)):
            ok = pc.inside(c, xy)
            if ok.any():
                row["border"] = min(row["border"], float(pc.cells_of(c, xy[ok])[1].min()))
                # (a point ON the world's own border is in no cell's interior either)
                row["border"] = min(row["border"], float(np.abs(np.abs(xy) - c.half).min()))
        if len(occ[p]) and part["centre_inside"] and part["samples_inside"] and Bv:
            sens_cell = tuple(pc.cells_of(c, pc.sensor_xy(c, centre)[None])[0][0])
            part["staging"] = pc.staging(c.cells, half, sens_cell, row["nt"])
            box = pc.slice_box(c.cells, half, sens_cell) if half else None
            part["box"] = box
            cc = pc.cells_of(c, cxy)[0]
            if sc.icp_ok:
                ut, ur = pc.unstable_sets(c, centre, cxy, samples, sxy, z_theta)
                part.update(u_true=ut, u_rule=ur, seg=pc.segment_counts(ur, row["nt"]))
                why = c.expect.get("discriminates")
                if why:
                    part["u_mutant"] = pc.unstable_sets(c, centre, cxy, samples, sxy, z_theta, sensor_from="robot" if why == "sensor" else "sensor",
                                                        angular=why != "angular")[1]
                    # ... and what a kernel with that bound gets wrong: (sample, beam) pairs of beams it calls stable whose cell carries
                    # another distance code than the centre's (exact field: the code is the squared distance to the nearest occupied cell)
                    mb = np.nonzero(ut & ~part["u_mutant"])[0]
                    part["mutant_wrong_codes"] = 0
                    if kind == "exact" and len(mb):
                        d2c = pc.nearest_d2(c, cc[mb], occ[p])
                        d2s = pc.nearest_d2(c, pc.cells_of(c, sxy[:, mb])[0], occ[p])
                        part["mutant_wrong_codes"] = int((d2s != d2c[None]).sum())
            if lookups and kind == "exact" and box is not None:
                settled = pc.look7_settles(c, cc, occ[p], box)
                part["centre_settled"] = settled
                part["occ"], part["centre_cells"] = occ[p], cc
                codes = [pc.nearest_d2(c, cc, occ[p])]
                if sc.icp_ok and part["u_rule"].any():
                    ub = np.nonzero(part["u_rule"])[0]
                    sc_cells = pc.cells_of(c, sxy[:, ub])[0]                      # [k][nu][2]
                    differs = (sc_cells != cc[ub][None]).any(-1)
                    pair_settled = pc.look7_settles(c, sc_cells, occ[p], box)
                    part["pairs_unsettled"] = int((differs & ~pair_settled).sum())
                    part["pairs_unsettled_centre_settled"] = int((differs & ~pair_settled & settled[ub][None]).sum())
                    part["pairs_settled"] = int((differs & pair_settled).sum())
                    codes.append(pc.nearest_d2(c, sc_cells[differs], occ[p]))
                    # pairs the deferred search decides whose code is NOT the centre's (there `cpz[b]` would be the wrong term)
                    pair_codes = pc.nearest_d2(c, sc_cells, occ[p])
                    part["pairs_unsettled_other_code"] = int((differs & ~pair_settled & (pair_codes != codes[0][ub][None])).sum())
                part["codes"] = np.concatenate([x.reshape(-1) for x in codes])
        row["parts"].append(part)
    return row


def _run(c, kind):
    pf = pc.oracle_filter(c, "inj" if kind == "plain" else "query")
    rows = []
    for sc in pc.scans(c):
        pc.prepare(pf, sc)
        before = pf.particles()[0].copy()
        occ = [pf.grid(p).occ_cells() for p in range(c.N)]
        tr = pf.slam(sc.scan, sc.u, sc.cur, sc.prev, sc.icp_ok, sc.guess, sc.normals)
        rows.append(_analyse(c, kind, pf, sc, before, pf.particles()[0].copy(), occ, tr))
        if tr["rc"]:
            break
    pf.close()
    return rows


@pytest.fixture(scope="module")
def runs():
    """Every case once through each oracle it is compared with (`plain` for an injected field, `exact` for the others), host noise."""
    t0 = time.perf_counter()
    out = {}
    for c in pc.CASES:
        if c.expect.get("unsupported"):
            continue
        for kind in sorted({"plain" if s == "inj" else "exact" for s in c.sources}):
            out[c.id, kind] = _run(c, kind)
    print(f"[propose cases] {len(out)} oracle runs in {time.perf_counter() - t0:.1f} s")
    return out


def _rows(runs, cid):
    return [rows for (i, _), rows in runs.items() if i == cid]


# ---- selectors ------------------------------------------------------------------------------------------------------------------------
def test_the_restated_literals_are_the_host_code_s_and_the_kernel_s():
    host = open(os.path.join(CSRC, "rbpf.hip")).read()
    dev = open(os.path.join(CSRC, "rbpf_device.hpp")).read()
    ker = open(os.path.join(CSRC, "rbpf_propose.hip")).read() + open(os.path.join(CSRC, "rbpf_lookup.hpp")).read()   # (its lookups)
    api = open(os.path.join(CSRC, "rbpf_api.hip")).read()
    plan = open(os.path.join(CSRC, "rbpf_plan.hpp")).read()       # (plan_propose: tests/test_rbpf_plan.py runs it against these restatements)
    for src, pieces in ((plan, ("const size_t bvn = in.Bv > 0 ? in.Bv : 1;",
                                "p.lds = sizeof(double) * ((12 + kUnCap) * (size_t)in.k + 3 * bvn) + sizeof(unsigned int) * 4 * bvn + p.slice_bytes;",
                                "if (in.df_mode == 2) {\n    // LDS copy of the occupancy bitmap",
                                "if (bytes <= 48 * 1024) { p.occ_half = half; p.slice_bytes = bytes; break; }",
                                "p.fits = p.lds <= (size_t)kMaxLds - 3072;",
                                "p.threads = (p.lds + 3072 > (size_t)kMaxLds / 4) ? 2 * kProposeThreads : kProposeThreads;",
                                "constexpr int kUnCap = 16;", "constexpr int kMaxLds = 160 * 1024;", "#define TBNAV_PROPOSE_THREADS 256",
                                "constexpr int kWave = 64;", "constexpr int kMixLut = 1024;")),
                        (host, ("if (!pp.fits) return TBNAV_ERR_UNSUPPORTED;", "if (pp.threads == NT_ && pp.dn == DN_) {", "pp.dn = noise.in_kernel;",
                                "return TBNAV_ERR_UNSUPPORTED;  // (a form the plan names and the list does not have)",
                                "h->TW = (xsize + kTS - 1) / kTS;")),
                        (dev, ("constexpr int kTS = 32, kTSh = 5,", "constexpr int kMixLds = 128;")),
                        (ker, ("tt_all <= NT && tt_all <= 256;", "constexpr int kStC = 12, kStIds = 256;",
                               "ntc = min(2 * nW, ds.occ.TW - tc0), n_ids = ((R1 >> kTSh) - tr0 + 1) * ntc;",
                               "if (ntc <= kStC && (whole_table || n_ids <= kStIds)) {",
                               "if (bw <= 9 && bw <= clear * clear) return bw;",
                               "const bool parked = dn || j < NT;",
                               "sdxy + (double)(sqrtf((float)(pt.x * pt.x + pt.y * pt.y)) * 1.000001f) * sdth + 1e-9;",
                               "const bool stable = ctag[b] < 0x10000u && (double)marg[b] > delta;",
                               "mg = __double2float_rd(fmin(fmin(ex - x_lo, x_hi - ex), fmin(ey - y_lo, y_hi - ey)));",
                               "const int seg = (c.Bv + kPW - 1) / kPW;", "constexpr int kPW = NT / kWave;",
                               "if (L.lds && cd < kMixLds) return L.lds[cd];", "if (L.glob && cd < kMixLut) return L.glob[cd];")),
                        (api, ('"rbpf_propose<%d, %s>", pp.threads, pp.dn ? "true" : "false"', "const ProposePlan& pp = h->last_propose;"))):
        for piece in pieces:
            assert piece in src, (f"the source no longer writes `{piece}`: if the rule changed, change its restatement in tests/propose_cases.py "
                                  "(and the cases' claims) with it; if only its spelling changed, update this list")
    # the four names are exactly the four explicit instantiations: the kernel file makes them from the one list of forms
    # (rbpf_device.hpp: TBNAV_PROPOSE_FORMS), which the launch dispatch and create's LDS attributes are made from too
    assert "#define TBNAV_X(NT_, DN_) template __global__ void rbpf_propose<NT_, DN_>(" in ker and ker.count("TBNAV_PROPOSE_FORMS(TBNAV_X)") == 1
    assert host.count("TBNAV_PROPOSE_FORMS(TBNAV_X)") == 2 and "template __global__ void rbpf_propose<k" not in ker
    forms = re.search(r"^#define TBNAV_PROPOSE_FORMS\(X\) (.*)$", dev, flags=re.M).group(1)
    inst = re.findall(r"X\(([^,]+), (true|false)\)", forms)
    assert " ".join(f"X({nt}, {dn})" for nt, dn in inst) == forms.strip()
    spelled = {"kProposeThreads": pc.K_PROPOSE_THREADS, "2 * kProposeThreads": 2 * pc.K_PROPOSE_THREADS}
    got = sorted(pc.name(spelled[nt], dn == "true") for nt, dn in inst)
    assert len(inst) == 4 and got == sorted(pc.name(nt, dn) for nt in (256, 512) for dn in (False, True))


def test_the_workgroup_size_and_the_lds_ceiling_fall_where_the_formula_puts_them():
    small = pc.CASE["k-97"]
    sb = pc.slice_bytes(small, "query")
    assert small.cells == 80 and sb == 1600 == pc.slice_bytes(small, "inj") and pc.slice_bytes(small, "window") == 0
    assert pc.propose_lds(97, 360, sb) == 37728 and 37728 + 3072 <= 40960 < pc.propose_lds(98, 360, sb) + 3072
    assert [pc.threads(k, 360, sb) for k in (1, 97, 98, 646)] == [256, 256, 512, 512]
    assert [pc.fits(k, 360, sb) for k in (646, 647)] == [True, False]
    assert pc.threads(10, 1080, sb) == 512 and pc.threads(10, 360, sb) == 256        # 512 threads forced by the scan, not by k
    for c in pc.CASES:
        for src in c.sources:
            for sc in pc.scans(c):
                Bv = pc.n_valid(c, sc.scan)
                if c.expect.get("unsupported"):
                    assert not pc.fits(c.k, Bv, pc.slice_bytes(c, src)) and c.threads is None, c.id
                else:
                    assert pc.fits(c.k, Bv, pc.slice_bytes(c, src)), c.id
                    assert pc.threads(c.k, Bv, pc.slice_bytes(c, src)) == c.threads, (c.id, src, sc.s, Bv)
        if "more_samples_than_threads" in c.expect and c.threads:
            assert c.expect["more_samples_than_threads"] == (c.k > c.threads), c.id
    assert {c.k for c in pc.CASES if c.expect.get("more_samples_than_threads")} == {513, 577, 646}


def test_every_instantiation_has_a_case_of_each_group_that_can_reach_it():
    assert {c.group for c in pc.CASES} == set(pc.GROUPS) and len({c.id for c in pc.CASES}) == len(pc.CASES)
    have = {(c.group, c.threads, n == "dn") for c in pc.CASES if c.threads for n in c.noises}
    for group in pc.GROUPS:
        for nt in (256, 512):
            for dn in (False, True):
                assert (group, nt, dn) in have, (group, nt, dn)
    for c in pc.CASES:
        assert 1 <= c.N <= 16 and c.cells <= 700 and c.n_scans <= 5 and c.k not in (2, 3), c.id
        assert set(c.sources) <= {"inj", "query", "window", "full"} and set(c.noises) <= {"host", "dn"}, c.id
        assert c.window is None or "inj" not in c.sources, c.id


# ---- reach ----------------------------------------------------------------------------------------------------------------------------
def test_every_case_returns_the_status_it_claims_and_keeps_its_beams(runs):
    for (cid, kind), rows in runs.items():
        c = pc.CASE[cid]
        status_at = c.expect.get("status_at", {})
        assert len(rows) == (min(status_at) + 1 if status_at else c.n_scans), (cid, kind, len(rows))
        for r in rows:
            assert r["rc"] == status_at.get(r["s"], 0), (cid, kind, r["s"], r["rc"])
            want = c.expect.get("valid_at", {}).get(r["s"])
            if want is not None:
                assert r["Bv"] == want, (cid, r["s"], r["Bv"])
            elif isinstance(c.valid.get(r["s"]), dict):
                assert r["Bv"] == len(c.valid[r["s"]]), (cid, r["s"], r["Bv"])
            elif not isinstance(c.valid.get(r["s"]), int):
                assert r["Bv"] == c.beams, (cid, r["s"], r["Bv"])
            assert (r["nocc"] == [0] * c.N) if r["s"] == 0 else (min(r["nocc"]) > 0), (cid, r["s"])
        for s in c.expect.get("resampled_at", ()):
            assert rows[s]["resampled"] == 1, (cid, kind)
    # the out-of-world statuses come from where the cases say: the moved pose of the ICP-failed branch; a SAMPLE alone
    for rows in _rows(runs, "sample-out-of-world"):
        parts = rows[2]["parts"]
        assert all(p["centre_inside"] for p in parts) and not all(p["samples_inside"] for p in parts)
    for rows in _rows(runs, "fail-out-of-world"):
        assert not rows[2]["icp_ok"] and not all(p["centre_inside"] for p in rows[2]["parts"])
    for cid in ("fail-straight", "fail-nearly-straight", "fail-1080", "fail-arc"):
        ws = {pc.CASE[cid].u_at[s][0] for s in range(3)}
        assert (max(abs(w) for w in ws) < 1e-12) == bool(pc.CASE[cid].expect.get("straight")), cid
    assert {pc.CASE[i].u_at[0][0] for i in ("fail-arc", "fail-straight", "fail-nearly-straight")} == {0.04, 0.0, 1e-13}


def test_the_unstable_counts_and_segments_are_what_the_cases_claim(runs):
    seen_chunks = set()
    for (cid, kind), rows in runs.items():
        c = pc.CASE[cid]
        e = c.expect
        for r in rows:
            for p, part in enumerate(r["parts"]):
                if "u_rule" not in part:
                    continue
                n = int(part["u_rule"].sum())
                seen_chunks.add((n + pc.K_UNCAP - 1) // pc.K_UNCAP if n <= 2 * pc.K_UNCAP + 1 else 99)
                if "unstable" in e:
                    assert e["unstable"][0] <= n <= e["unstable"][1], (cid, kind, r["s"], p, n)
                if r["s"] in e.get("unstable_at", {}):
                    assert n == e["unstable_at"][r["s"]] == r["Bv"], (cid, kind, r["s"], p, n)
                if r["s"] in e.get("segments_at", {}):
                    assert tuple(x > 0 for x in part["seg"]) == e["segments_at"][r["s"]], (cid, kind, r["s"], p, part["seg"])
                    assert int(part["u_true"].sum()) > 0, (cid, kind, p)      # (and some sample really leaves the centre's cell)
        for s in list(e.get("unstable_at", {})) + list(e.get("segments_at", {})):
            assert all("u_rule" in part for part in rows[s]["parts"]), (cid, kind, s)
    assert {0, 1, 2, 3, 99} <= seen_chunks      # no unstable beam, one chunk, two, three (33 beams), many
    # one chunk exactly / one beam into the second: 16 and 17, 32 and 33 are the claimed values themselves
    assert [pc.CASE[f"split-{n}"].expect["unstable_at"][2] for n in (16, 17, 32, 33)] == [16, 17, 32, 33]
    # a wave's range can be empty of BEAMS too: fewer valid beams than waves
    for cid, kpw in (("valid-1", 4), ("valid-3", 4), ("valid-1-k170", 8), ("valid-7-k170", 8)):
        assert pc.CASE[cid].expect["valid_at"][2] < kpw == pc.CASE[cid].threads // 64


def test_the_rule_s_premise_holds_a_beam_called_stable_stays_in_the_centre_s_cell_for_every_sample(runs):
    checked = 0
    for (cid, kind), rows in runs.items():
        for r in rows:
            for p, part in enumerate(r["parts"]):
                if "u_rule" in part:
                    missed = part["u_true"] & ~part["u_rule"]
                    assert not missed.any(), (cid, kind, r["s"], p, np.nonzero(missed)[0])
                    checked += 1
    assert checked > 400


@pytest.mark.parametrize("cid", ["rot-spread", "trs-rot-spread"])
def test_the_rotation_cases_tell_the_bound_from_its_mutants(runs, cid):
    """Without its angular term (rot-spread), or with the sensor's travel taken from the robot's pose (trs-rot-spread), the bound calls
    beams stable that some sample moves to another cell: a kernel with that mutation computes other likelihoods in these cases."""
    missed = wrong = 0
    for rows in _rows(runs, cid):
        for r in rows:
            for part in r["parts"]:
                if "u_mutant" in part:
                    missed += int((part["u_true"] & ~part["u_mutant"]).sum())
                    wrong += part["mutant_wrong_codes"]
    assert missed > 0 and wrong > 0, (cid, missed, wrong)


def test_the_lookup_cases_reach_the_paths_they_name(runs):
    for (cid, kind), rows in runs.items():
        c = pc.CASE[cid]
        e = c.expect
        if c.group not in ("lookups", "res") or kind != "exact":
            continue
        for r in rows[1:]:
            for p, part in enumerate(r["parts"]):
                if "staging" in e:
                    assert part["staging"] == e["staging"], (cid, r["s"], p, part["staging"])
                if e.get("slice_at_map_border"):
                    assert part["box"][0] == 0 and part["box"][2] == 0 and part["box"][1] == c.cells - 1, (cid, part["box"])
                if r["s"] in e.get("unsettled_centre_at", ()):
                    assert (~part["centre_settled"]).sum() > 0, (cid, r["s"], p)
                if r["s"] in e.get("settled_centre_at", ()):
                    assert part["centre_settled"].all(), (cid, r["s"], p, int((~part["centre_settled"]).sum()))
                if r["s"] in e.get("unsettled_pair_at", ()):
                    assert part["pairs_unsettled_centre_settled"] > 0 and part["pairs_settled"] > 0, (cid, r["s"], p)
                    assert part["pairs_unsettled_other_code"] > 0, (cid, r["s"], p)
                if r["s"] == e.get("tiers_at"):
                    cd = part["codes"]
                    assert (cd < pc.K_MIX_LDS).any() and ((cd >= pc.K_MIX_LDS) & (cd < pc.K_MIX_LUT)).any() and (cd >= pc.K_MIX_LUT).any(), (cid, p)
                    assert cd.max() <= 200 * 200        # (within cell_radius: a code, not the stored "never reached")
    # the limit of the 7 x 7 look: the two hand-made cells, the lookup between them, and the oracle's term is code 16's
    c = pc.CASE["look7-limit"]
    e = c.expect["look7"]
    (ai, aj), (bi, bj), (li, lj) = e["A"], e["B"], e["L"]
    r = runs[c.id, "exact"][e["at"]]
    assert r["Bv"] == 1 and ((ai - li) ** 2 + (aj - lj) ** 2, (bi - li) ** 2 + (bj - lj) ** 2) == (16, 18) and (abs(bi - li), abs(bj - lj)) == (3, 3)
    term = lambda d2: 0.95 * np.exp(-0.5 * d2 * pc.RES ** 2 / 0.25) / np.sqrt(2 * np.pi * 0.25) + 0.01 / 0.04   # noqa: E731
    for p, part in enumerate(r["parts"]):
        assert sorted(part["occ"].tolist()) == sorted([ai * c.cells + aj, bi * c.cells + bj]), (p, part["occ"])
        assert part["centre_cells"].tolist() == [[li, lj]] and not part["centre_settled"].any() and part["codes"].tolist() == [16], p
        assert pc.look7_fits(c, part["centre_cells"], part["box"]).all(), (p, part["box"])    # the look RUNS at L and answers 18: `bw <= 9` refuses it
        assert not part["u_rule"].any(), p                                   # (every sample sees the centre's cell: one lookup decides them all)
    assert np.allclose(r["p_scan"], term(16), rtol=1e-12) and abs(term(18) / term(16) - 1) > 1e-3
    stagings = {pc.CASE[i].expect["staging"] for i in ("cells-512", "cells-544", "cells-700-ids", "cells-700-words", "cells-700-none")}
    assert stagings == {"whole_table", "ids", "words", "none"}
    assert (pc.CASE["cells-512"].cells, pc.CASE["cells-544"].cells) == (512, 544)          # 16 x 16 tiles and the first size beyond
    assert [smc.slice_regime(pc._Slice(pc.CASE[i].cells, pc.CASE[i].range_max, pc.RES))[0] for i in ("cells-700-ids", "cells-700-words", "cells-700-none")] == [48, 16, None]


def test_the_clamp_and_geometry_cases_reach_what_they_name(runs):
    for rows in _rows(runs, "heading-pi"):
        for p in range(pc.CASE["heading-pi"].N):
            assert any(all(r["parts"][p]["theta_signs"]) for r in rows), p      # samples on both sides of +-pi
    for rows in _rows(runs, "scan-max-binds"):
        ps = np.concatenate([r["p_scan"].reshape(-1) for r in rows[1:]])
        assert (ps > 1e-30).all()                                                         # the upper clamp binds for every sample, the lower never
    for rows in _rows(runs, "scan-max-some"):
        ps = np.concatenate([r["p_scan"].reshape(-1) for r in rows[1:]])
        assert (ps > 1.5 * 1.01).sum() >= 10 and (ps < 1.5 / 1.01).sum() >= 10 and (ps > 1e-300).all()   # ... for some samples, not for others
    for rows in _rows(runs, "scan-min-binds"):
        ps = np.concatenate([r["p_scan"].reshape(-1) for r in rows])
        assert (ps < 1e30).all()
    for rows in _rows(runs, "open") + _rows(runs, "open-k98"):
        ps = np.concatenate([r["p_scan"].reshape(-1) for r in rows])
        assert (ps > 1e-300).all() and (ps < 1e300).all() and ps[ps != 1.0].max() / ps.min() > 1e3      # the likelihoods decide mu
    # decision margins of the two eta cases: a factor 2 at least from 1e-12, on the side claimed
    for rows in _rows(runs, "eta-small"):
        for r in rows:
            assert (r["eta"] >= 2e-12).all() and (r["eta"] <= 1e-11).all(), (r["s"], r["eta"])
    c = pc.CASE["eta-zero"]
    assert c.k * c.clamps[1] * c.clamps[3] <= 0.5e-12 and c.expect["status_at"] == {0: STATUS_ETA_ZERO}
    assert pc.CASE["sample-out-of-world"].expect["status_at"] == {2: STATUS_OUT_OF_WORLD}


# ---- other cell sizes ---------------------------------------------------------------------------------------------------------------------
def test_the_cases_at_0p05_are_byte_for_byte_what_they_were():
    """The table took a cell size (Case.res, default 0.05): the fields, runs, slices and every scan's inputs of these cases hash to what
    tests/golden/make_case_digests.py recorded before it did."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("make_case_digests", os.path.join(ROOT, "tests", "golden", "make_case_digests.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "case_digests.json")))["propose"]
    assert set(want) == set(mk.PROPOSE_IDS) and len(want) >= 8
    for cid in mk.PROPOSE_IDS:
        assert pc.CASE[cid].res == pc.RES == 0.05 and mk.propose_digest(cid) == want[cid], cid
    assert all((c.res == pc.RES) == (c.group != "res") for c in pc.CASES)


def test_the_cell_size_cases_reach_what_they_name(runs):
    """Per case of group `res`, from the oracle's numbers (host noise): the least and most unstable beams of a particle by the kernel's
    rule, the tiers of mix_term its lookups take, whether the 7 x 7 look settles the centre lookups, and the slice margin."""
    sigma = np.sqrt(pc._ALL[1])
    assert sigma / 0.0394 > 1.5 and sigma / 0.5 < 0.13          # the wide spread: a cell and a half, an eighth of a cell
    for res in pc.RES_SIZES:
        tag = pc.res_tag(res)
        for cid, var in ((f"res-{tag}", pc.DEFAULT_VAR), (f"res-{tag}-wide", pc._ALL)):
            c = pc.CASE[cid]
            assert (c.res, c.N, c.k, c.beams, c.var, c.half, c.cells) == (res, 4, 10, 360, var, 2.0, int(np.ceil(4.0 / res))) and c.cells % 2 == 0, cid
            assert len(pc.runs_of(c)) == 8 and c.threads == 256, cid
    for c in pc.CASES:
        if c.group != "res":
            continue
        e = c.expect
        margin, half = smc.slice_regime(pc._Slice(c.cells, c.range_max, c.res))
        assert margin == e["margin"] == 48 and half >= c.cells and pc.occ_half(c, "query") == half, c.id      # every map here is inside its slice
        if "unstable" not in e:
            continue
        for kind in ("plain", "exact"):
            rows = runs[c.id, kind]
            un = [int(part["u_rule"].sum()) for r in rows[1:] for part in r["parts"]]
            assert len(un) == 2 * c.N and (min(un), max(un)) == e["unstable"], (c.id, kind, min(un), max(un))
        rows = runs[c.id, "exact"]
        parts = [part for r in rows[1:] for part in r["parts"]]
        assert all(part["staging"] == "whole_table" for part in parts), c.id
        cd = np.concatenate([part["codes"] for part in parts])
        tiers = tuple(t for t, hit in (("lds", (cd < pc.K_MIX_LDS).any()), ("lut", ((cd >= pc.K_MIX_LDS) & (cd < pc.K_MIX_LUT)).any()),
                                       ("beyond", (cd >= pc.K_MIX_LUT).any())) if hit)
        assert tiers == e["tiers"], (c.id, tiers, int(cd.max()))
        frac = [part["centre_settled"].mean() for part in parts]
        kind = "every" if min(frac) == 1.0 else "none" if max(frac) == 0.0 else "some"
        assert kind == e["centre_settled"] and (kind != "some" or (0.05 < min(frac) and max(frac) < 0.95)), (c.id, min(frac), max(frac))
    # either side of the kUnCap = 16 unstable beams of the per-pair path: the shipped spread stays in one chunk at every size, the wide
    # one takes more than two
    for res in pc.RES_SIZES:
        tag = pc.res_tag(res)
        assert pc.CASE[f"res-{tag}"].expect["unstable"][1] <= pc.K_UNCAP and pc.CASE[f"res-{tag}-wide"].expect["unstable"][0] > 2 * pc.K_UNCAP, res
    # what a size cannot reach: a code is at most 2 (cells - 1)^2 — below kMixLds on the 8-cell map, below kMixLut on the 14-cell one
    assert 2 * 7 * 7 < pc.K_MIX_LDS and 2 * 13 * 13 < pc.K_MIX_LUT < 2 * 57 * 57
    assert pc.CASE["res-0p0394-tiers"].expect["tiers_at"] == 3 and pc.CASE["res-0p0394-tiers"].res == 0.0394


# ---- margins --------------------------------------------------------------------------------------------------------------------------
def test_no_end_point_lies_within_1e_12_m_of_a_cell_border(runs):
    """Centre and every sample, every beam, every case: about fifty times the rounding of a four-operation coordinate of at most
    17.5 m.  Inside it the device's sincos could put a point in the neighbouring cell."""
    worst = min(r["border"] for rows in runs.values() for r in rows)
    print(f"[propose cases] nearest end point to a cell border: {worst:.3g} m")
    for (cid, kind), rows in runs.items():
        for r in rows:
            assert r["border"] >= pc.BORDER_MIN, (cid, kind, r["s"], r["border"])
