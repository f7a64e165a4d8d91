"""rbpf_propose<NT, DN> (csrc/rbpf_propose.hip) against the oracle, path by path: one run per case, field source and noise form of
tests/propose_cases.py.  After every scan the launched instantiation is the one the restated host expressions name, and every stage
of the update agrees with the oracle at the project's own tolerances — with the oracle's field injected, tests/test_rbpf_gpu.py's
_compare_scan; un-injected (query / window / full against the `exact_field` oracle), tests/test_rbpf_field_gpu.py's
_assert_every_stage and the maps with `==`.  tests/test_propose_cases.py shows on the CPU which path of the kernel each case takes and
that no end point of any case is near enough to a cell border to land elsewhere on the device."""
import time

import numpy as np
import pytest

import oracle_api as orc  # noqa: F401  (builds the oracle before the first case)
import propose_cases as pc
from test_rbpf_field_gpu import _assert_every_stage, _stage_row
from test_rbpf_gpu import _compare_scan, _inject

pytestmark = pytest.mark.gpu

RUNS = [(c, src, noise) for c in pc.CASES if not c.expect.get("unsupported") for src, noise in pc.runs_of(c)]
SEED = 4242


def _dev(gpu_pkg, case, src, noise):
    from rtn_amd import capi
    from rtn_amd.rbpf import ParticleFilter, default_params
    pf = ParticleFilter(default_params(**pc.device_params_kw(case)), df_mode=None if src == "inj" else src)
    if noise == "dn":
        pf.setOption(capi.RBPF_OPT_NOISE_IN_KERNEL, 1)
        pf.setSeed(SEED)
        if case.shard:
            pf.setRngShard(case.shard[0], case.N + case.shard[1])
    return pf


def _device_scan(pf_d, sc, noise):
    """One scan on the device; returns its stats and the normal stream it used (dn: what the kernel drew, as the handle reports it)."""
    pc.prepare(pf_d, sc, setter="setParticles")
    if noise == "dn":
        st = pf_d.SLAM(sc.scan, sc.u, sc.cur, sc.prev, sc.icp_ok, sc.guess, None, check=False)
        return st, pf_d.lastNormals(pf_d.numNormals(sc.icp_ok))
    return pf_d.SLAM(sc.scan, sc.u, sc.cur, sc.prev, sc.icp_ok, sc.guess, sc.normals, check=False), sc.normals


def _run(gpu_pkg, case, src, noise, keep=None):
    t0 = time.perf_counter()
    pf_o, pf_d = pc.oracle_filter(case, src), _dev(gpu_pkg, case, src, noise)
    assert (pf_d.xsize, pf_d.ysize) == (case.cells, case.cells)
    status_at = case.expect.get("status_at", {})
    rows = []
    for sc in pc.scans(case):
        if src == "inj":
            _inject(pf_o, pf_d)
        st, normals = _device_scan(pf_d, sc, noise)
        pc.prepare(pf_o, sc)
        tr_o = pf_o.slam(sc.scan, sc.u, sc.cur, sc.prev, sc.icp_ok, sc.guess, normals)
        Bv = pc.n_valid(case, sc.scan)
        assert st.n_valid_beams == Bv, (case.id, sc.s, st.n_valid_beams, Bv)
        want = pc.name(pc.threads(case.k, Bv, pc.slice_bytes(case, src)), noise == "dn")
        assert pf_d.lastKernelNames()[0] == want == pc.name(case.threads, noise == "dn"), (case.id, src, noise, sc.s, pf_d.lastKernelNames()[0], want)
        if sc.s in status_at:       # what the reference throws, the kernel reports: statuses only
            assert st.status == tr_o["rc"] == status_at[sc.s], (case.id, src, noise, sc.s, st.status, tr_o["rc"])
            break
        assert st.status == 0 and tr_o["rc"] == 0, (case.id, src, noise, sc.s, st.status, tr_o["rc"])
        if src == "inj":
            _compare_scan(pf_o, pf_d, tr_o, st, sc.icp_ok)
        else:
            if sc.icp_ok:
                rows.append(_stage_row(pf_o, pf_d, tr_o, st))
                _assert_every_stage(rows[-1:])
            else:
                _compare_scan(pf_o, pf_d, tr_o, st, False)
            nocc = pf_d.occupiedCount()
            for p in range(case.N):
                g = pf_o.grid(p)
                assert np.array_equal(pf_d.logOdds(p), g.dump()["log_odds"]), f"{case.id}, scan {sc.s}: log-odds differ for particle {p}"
                assert nocc[p] == len(g.occ_cells()), (case.id, sc.s, p)
        if sc.s in case.expect.get("resampled_at", ()):
            assert st.resampled == 1 == tr_o["resampled"], (case.id, sc.s)
        if keep is not None:
            keep.append((pf_d.trace(), pf_d.particles()))
    pf_d.close(); pf_o.close()
    print(f"[{case.id} {src} {noise}] {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("case,src,noise", RUNS, ids=lambda v: v.id if isinstance(v, pc.Case) else v)
def test_the_proposal_equals_the_oracle_on_the_path_the_case_names(gpu_pkg, case, src, noise):
    _run(gpu_pkg, case, src, noise)


def test_query_window_and_full_give_each_other_bit_identical_traces(gpu_pkg):
    """The three modes hold the same field: where a case names more than one of them, every number the proposal leaves is the same
    bit for bit, scan by scan (device against device; the oracle comparison is the test above)."""
    checked = 0
    for case in pc.CASES:
        modes = [s for s in case.sources if s != "inj"]
        if len(modes) < 2:
            continue
        got = {}
        for m in modes:
            got[m] = []
            _run(gpu_pkg, case, m, "host", keep=got[m])
        for m in modes[1:]:
            assert len(got[m]) == len(got[modes[0]]) == case.n_scans
            for s, ((tr_a, pa), (tr_b, pb)) in enumerate(zip(got[modes[0]], got[m])):
                for key in ("sampled", "p_scan", "p_pose", "eta", "mu", "sigma", "new_pose", "weight_raw"):
                    assert np.array_equal(tr_a[key], tr_b[key]), (case.id, m, s, key)
                assert all(np.array_equal(x, y) for x, y in zip(pa, pb)), (case.id, m, s)
            checked += 1
    assert checked >= 2


def test_a_scan_too_large_for_one_workgroup_is_refused_and_leaves_the_state_alone(gpu_pkg):
    """k = 647 at 360 beams on an 80-cell map: one sample more than the LDS ceiling holds.  TBNAV_ERR_UNSUPPORTED, and poses,
    weights and log-odds as before the call (a map is built first through the map update alone: the proposal never ran)."""
    from rtn_amd import capi
    case = pc.CASE["k-647"]
    for src in case.sources:
        pf_d = _dev(gpu_pkg, case, src, "host")
        sc = next(iter(pc.scans(case)))
        assert not pc.fits(case.k, pc.n_valid(case, sc.scan), pc.slice_bytes(case, src))
        pf_d.integrateScanMany(sc.scan, pf_d.particles()[0])
        assert pf_d.occupiedCount().min() > 0
        before = [a.copy() for a in pf_d.particles()] + [pf_d.logOdds(p).copy() for p in range(case.N)]
        with pytest.raises(capi.TbnavError) as ei:
            pf_d.SLAM(sc.scan, sc.u, sc.cur, sc.prev, True, sc.guess, sc.normals)
        assert ei.value.status == capi.ERR_UNSUPPORTED, ei.value.status
        after = [a.copy() for a in pf_d.particles()] + [pf_d.logOdds(p).copy() for p in range(case.N)]
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        pf_d.close()
