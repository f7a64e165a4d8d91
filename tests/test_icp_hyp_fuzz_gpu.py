"""30 drawn cases of the hypotheses of the global search (include/tbnav_icp.h HYPOTHESES, csrc/icp_hyp.hip) against the brute-force
restatement with ==: the global search's drawn maps (sparse maps scanned by 1-3 points, where equal scores and plateaus are the rule,
and dense maps with up to 120 points; every pooling, regions, stamps of other widths; 44 to 96 cells) and maps of 24 cells of 0.5 m, with
a drawn floor, separations, wrap and K."""
import numpy as np
import pytest

import icp_global_cases as gc
import icp_global_restatement as G
import icp_hyp_restatement as H
import icp_restatement as R
from test_icp_global_fuzz_gpu import draw as draw_global
from test_icp_hyp_gpu import _aligner, _check, _filter, _occ_of, _set_occ

pytestmark = pytest.mark.gpu


def draw(seed):
    geom, occ, scan, sp, gp = draw_global(seed)
    rng = np.random.default_rng(7000 + seed)
    if seed % 6 == 1:                                       # 24 cells of 0.5 m
        geom, sp = gc.geom("r24"), gc.SP50
        occ = (rng.random((24, 24)) < 0.08).astype(np.uint8)
        scan = np.full(360, 0.05, dtype=np.float32)
        beams = rng.choice(360, size=int(rng.integers(1, 30)), replace=False)
        scan[beams] = rng.uniform(0.6, 3.4, size=beams.size).astype(np.float32)
        gp = G.Params(ang_count=int(rng.integers(1, 13)), ang_step=float(rng.uniform(0.05, 1.5)), pool_log2=int(rng.integers(1, 4)),
                      min_quality=float(rng.uniform(0.1, 0.9)))
    f = int((1, 512, 768, 1000, 1024)[int(rng.integers(5))]) if seed % 3 else int(rng.integers(1, 1025))
    hp = H.HypParams(max_hyp=int((1, 3, 8, 64)[int(rng.integers(4))]), floor_q10=f, sep_cells=int(rng.integers(0, 13)),
                     sep_steps=int(rng.integers(0, 8)), wrap=int(rng.integers(0, 2)))
    assert H.valid(hp) and G.valid(gp, geom.side)
    return geom, occ, scan, sp, gp, hp


@pytest.mark.parametrize("seed", range(30))
def test_a_drawn_case_equals_the_restatement(gpu_pkg, seed):
    geom, occ, scan, sp, gp, hp = draw(seed)
    pf = _filter(gpu_pkg, geom, N=1)
    _set_occ(pf, 0, occ)
    assert np.array_equal(_occ_of(pf, 0), occ)
    a = _aligner(gpu_pkg, sp)
    want = H.localize_hyp(occ, geom, R.cloud(scan, gc.LASER)[0], sp, gp, hp)
    assert want.status == "ok"
    info = _check(a, pf, 0, scan, gp, hp, want, (seed, geom.side, sp.stamp_cells, gp, hp))
    print(seed, geom.side, info["n_peaks"], info["candidates"], info["floor_blocks"])
    a.close(); pf.close()
