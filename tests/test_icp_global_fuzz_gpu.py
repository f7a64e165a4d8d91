"""30 drawn cases of the global search (include/tbnav_icp.h GLOBAL SEARCH, csrc/icp_global.hip) against the exhaustive restatement with
==: sparse maps scanned by 1-3 points, where equal scores in many blocks are the rule and L4's index rule and L6's "a bound that equals
the score is refined" decide the answer, and dense maps with up to 120 points; every pooling, regions, stamps of other widths."""
import numpy as np
import pytest

import icp_global_cases as gc
import icp_global_restatement as G
import icp_restatement as R
import icp_search_restatement as S
from test_icp_global_gpu import _aligner, _check, _filter, _occ_of, _set_occ

pytestmark = pytest.mark.gpu


def draw(seed):
    rng = np.random.default_rng(1000 + seed)
    size_id = ("s44", "s64", "s72", "s96")[int(rng.integers(4))]
    geom = gc.geom(size_id)
    n = geom.side
    sparse = seed % 2 == 0
    occ = np.zeros((n, n), dtype=np.uint8)
    if sparse:
        for _ in range(int(rng.integers(1, 7))):
            occ[int(rng.integers(n)), int(rng.integers(n))] = 1
        if seed % 6 == 0:                                   # a pattern and its copy a multiple of every s apart
            i, j = int(rng.integers(n - 33)), int(rng.integers(n - 33))
            occ[i, j] = occ[i + 32, j] = occ[i, j + 32] = 1
    else:
        occ = (rng.random((n, n)) < rng.uniform(0.01, 0.08)).astype(np.uint8)
    scan = np.full(360, 0.05, dtype=np.float32)
    beams = rng.choice(360, size=int(rng.integers(1, 4)) if sparse else int(rng.integers(20, 121)), replace=False)
    scan[beams] = rng.uniform(0.13, 0.6 * n * 0.05, size=beams.size).astype(np.float32)
    if seed % 5 == 0:
        scan[beams[0]] = np.float32(0.125 * (1 + int(rng.integers(4)) * 2))      # 2.5, 7.5, ... cells along its beam
    k = int((1, 2, 3, 5)[int(rng.integers(4))])
    sp = S.Params(sigma=float((0.05, 0.1)[int(rng.integers(2))]), stamp_cells=k)
    region = (-1, -1, -1, -1)
    if rng.random() < 0.4:
        x0, y0 = int(rng.integers(n - 1)), int(rng.integers(n - 1))
        region = (x0, y0, int(rng.integers(x0, n)), int(rng.integers(y0, n)))
    gp = G.Params(ang_count=int(rng.integers(1, 13)), ang_step=float(rng.uniform(0.05, 1.5)), pool_log2=int(rng.integers(1, 6)), region=region,
                  min_quality=float(rng.uniform(0.1, 0.9)))
    assert S.valid(sp) and G.valid(gp, n)
    return geom, occ, scan, sp, gp


@pytest.mark.parametrize("seed", range(30))
def test_a_drawn_case_equals_the_restatement(gpu_pkg, seed):
    geom, occ, scan, sp, gp = draw(seed)
    pf = _filter(gpu_pkg, geom, N=1)
    _set_occ(pf, 0, occ)
    assert np.array_equal(_occ_of(pf, 0), occ)
    a = _aligner(gpu_pkg, sp)
    want = G.localize(occ, geom, R.cloud(scan, gc.LASER)[0], sp, gp)
    _check(a, pf, 0, scan, gp, want, (seed, geom.side, sp.stamp_cells, gp))
    a.close(); pf.close()
