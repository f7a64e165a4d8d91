"""One bounded randomized sweep of the device ICP inside the suite: tools/fuzz_icp.py, 200 cases from a FIXED seed — random beam
counts (half of them beside a multiple of 256), both metrics, lasers, valid fractions, rooms / wrapped rays with exact distance
ties / one target point, Trs, max_corr_dist, epsilons, max_iter, guess errors — each through tbnav_icp_match twice and every
fourth through a six-scan tbnav_icp_step_batch, against the numpy restatements bit for bit.  The sweep must also have gone
through every instantiation of both kernels and every stop rule.  The committed record of a run (profiles/r07_fuzz_icp.txt) is
refreshed by hand, never by the suite."""
import ast
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CASES, SEED = 200, 2027


def test_bounded_fuzz_sweep_of_the_icp_against_the_restatements(gpu_pkg):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_icp.py"), str(N_CASES), str(SEED)], capture_output=True,
                       text=True, timeout=900, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("icp:", "[FAIL]"))]
    print("\n" + "\n".join(lines[-4:]))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    summary = [l for l in lines if l.startswith(f"icp: {N_CASES} cases done")]
    assert len(summary) == 1 and summary[0].startswith(f"icp: {N_CASES} cases done, failures so far 0; "), lines
    tot = ast.literal_eval(summary[0].split("; ", 1)[1])
    assert tot["matches"] == N_CASES and tot["batches"] == N_CASES // 4, tot
    assert set(tot["point_P"]) == {1, 2, 3, 4, 6, 8, 12, 16}, tot      # every instantiation of icp_align<PointMetric>
    assert set(tot["line_P"]) == {1, 2, 3, 4, 6, 8}, tot               # and of icp_align<LineMetric>
    assert set(tot["criterion"]) == {0, 1, 2, 3, 4, 5, 6}, tot         # every way to stop (0: a batch's first scan)
    assert tot["with_ties"] >= 10, tot
