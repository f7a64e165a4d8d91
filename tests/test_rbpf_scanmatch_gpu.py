"""rbpf_scanmatch (csrc/rbpf_propose.hip) against the oracle's matcher on the lookup paths it ships with: a free run per case of
tests/scanmatch_cases.py, NOTHING injected — the device in the case's distance-field mode (query: the LDS slice of the bitmap, the
7 x 7 look, the bit-scan look, `clear`, the global bitmap; window / full: the stored field inside the refreshed window), the oracle
with its `exact_field` switch on, which is the field all three modes hold.  After every scan the matched centres and scores, every
stage of the update and the maps must agree at the tolerances of tests/test_rbpf_gpu.py; tests/test_scanmatch_cases.py shows on the
CPU that each case reaches what it is there for and that no matcher decision is close enough to differ between the two sides."""
import time

import numpy as np
import pytest

import oracle_api as orc  # noqa: F401  (builds the oracle before the first case)
import scanmatch_cases as smc
from test_rbpf_field_gpu import _assert_every_stage, _stage_row
from test_rbpf_gpu import LIK_RTOL, POSE_RTOL, _close

pytestmark = pytest.mark.gpu


def _dev(gpu_pkg, case, mode=None):
    from rtn_amd.rbpf import ParticleFilter, default_params
    return ParticleFilter(default_params(**smc.params(case)), df_mode=mode or case.mode)


def _device_step(pf_d, case, sc, check=True):
    pf_d.setScanMatching(sc.matching, *case.steps)
    if sc.weights is not None:
        pf_d.setParticles(w=sc.weights)
    return pf_d.SLAM(sc.scan, sc.u, sc.cur, sc.prev, True, sc.guess, sc.normals, check=check)


@pytest.mark.parametrize("case", smc.CASES, ids=lambda c: c.id)
def test_free_run_with_the_matcher_on_equals_the_exact_field_oracle(gpu_pkg, case):
    from rtn_amd import capi
    t0 = time.perf_counter()
    pf_o, pf_d = smc.oracle_filter(case), _dev(gpu_pkg, case)
    assert (pf_d.xsize, pf_d.ysize) == (case.cells, case.cells)
    rows, moved = [], 0
    for sc in smc.scans(case):
        tr_o = smc.oracle_step(pf_o, case, sc)
        if sc.s == case.expect.get("out_of_world_at"):
            # a trial pose's end points leave the map: the reference's world2rowmajor throws, the kernel reports — statuses only
            st = _device_step(pf_d, case, sc, check=False)
            assert tr_o["rc"] == capi.ERR_OUT_OF_WORLD == st.status, (tr_o["rc"], st.status)
            break
        st = _device_step(pf_d, case, sc)
        assert st.status == 0 and tr_o["rc"] == 0, (case.id, sc.s, st.status, tr_o["rc"])
        if sc.matching:
            c_o, sc_o = pf_o.scan_match_result()
            c_d, sc_d = pf_d.scanMatch()
            dc = float(np.max(np.abs(c_d - c_o))); ds = float(np.max(np.abs(sc_d - sc_o) / np.abs(sc_o)))
            print(f"[{case.id}] scan {sc.s}: centres differ by {dc:.3g}, scores by {ds:.3g} rel; oracle moves {pf_o.scan_match_stats()['moves'].tolist()}")
            assert _close(c_d, c_o, POSE_RTOL, 1e-14), (case.id, sc.s, dc)
            assert _close(sc_d, sc_o, LIK_RTOL), (case.id, sc.s, ds)
            moved += int(pf_o.scan_match_stats()["moves"].sum())
        rows.append(_stage_row(pf_o, pf_d, tr_o, st))
        _assert_every_stage(rows[-1:])
        nocc = pf_d.occupiedCount()
        for p in range(case.N):
            g = pf_o.grid(p)
            assert np.array_equal(pf_d.logOdds(p), g.dump()["log_odds"]), f"{case.id}, scan {sc.s}: log-odds differ for particle {p}"
            assert nocc[p] == len(g.occ_cells()), (case.id, sc.s, p)
    if "moves_at" in case.expect:   # (a matcher that never moved would agree trivially; the CPU test pins which cases name no such scan)
        assert moved > 0, case.id
    for s in case.expect.get("resampled_at", ()):
        assert rows[s]["resampled"] == (1, 1)
    pf_d.close(); pf_o.close()
    print(f"[{case.id}] {time.perf_counter() - t0:.2f} s")


def test_query_window_and_full_give_each_other_bit_identical_centres(gpu_pkg):
    """The three modes hold the same field, so on the modes case they make the same lookups' values and the same moves: matched
    centres and scores bit for bit, scan by scan (device against device; the oracle comparison is the test above)."""
    got = {}
    for cid in smc.MODE_CASES:
        case = smc.CASE[cid]
        pf_d = _dev(gpu_pkg, case)
        got[case.mode] = []
        for sc in smc.scans(case):
            _device_step(pf_d, case, sc)
            got[case.mode].append(pf_d.scanMatch())
        pf_d.close()
    assert set(got) == {"query", "window", "full"}
    for mode in ("window", "full"):
        for s, ((c_q, s_q), (c_m, s_m)) in enumerate(zip(got["query"], got[mode])):
            assert np.array_equal(c_q, c_m) and np.array_equal(s_q, s_m), (mode, s)
