"""Seeded fuzz of the map search (include/tbnav_icp.h MAP SEARCH, csrc/icp_search_map.hip) against its restatement with ==: 30 drawn
maps, origins, parameters, guesses and scans; the table, tgt_points, the score volume and the record."""
import numpy as np
import pytest

import icp_restatement as R
import icp_search_map_cases as mc
import icp_search_map_restatement as M
import icp_search_restatement as S
from test_icp_search_map_gpu import _aligner, _check, _filter, _occ_of, _set_occ

pytestmark = pytest.mark.gpu

HALF_EXTENTS = (0.39, 0.79, 0.84, 1.19, 1.63, 2.4)      # n = 16, 32, 34, 48, 66, 96


@pytest.mark.parametrize("size_id,seed0", [("s64", 100), ("s80", 200), ("s96", 300)])
def test_drawn_maps_origins_parameters_and_guesses(gpu_pkg, size_id, seed0):
    geom = mc.geom(size_id)
    pf = _filter(gpu_pkg, geom, N=2)
    for seed in range(seed0, seed0 + 10):
        rng = np.random.default_rng(seed)
        k = int(rng.integers(1, 9))
        p = S.Params(half_extent=float(rng.choice(HALF_EXTENTS)), sigma=float(rng.choice((0.03, 0.05, 0.1, 0.3))), stamp_cells=k,
                     lin_cells=int(rng.integers(0, 17)), ang_steps=int(rng.integers(0, 4)), slack_q10=int(rng.choice((0, 0, 100, 1023))),
                     min_quality=float(rng.choice((0.05, 0.5))))
        assert S.valid(p) and M.stamp_is_a_non_increasing_function_of_d2(p)
        occ = (rng.random((geom.side, geom.side)) < float(rng.choice((0.002, 0.02, 0.3)))).astype(np.uint8)
        slot = int(rng.integers(0, 2))
        _set_occ(pf, slot, occ)
        assert np.array_equal(_occ_of(pf, slot), occ)
        T = mc.guess(size_id, int(rng.integers(0, geom.side)), int(rng.integers(0, geom.side)), th=float(rng.uniform(-3.2, 3.2)),
                     fx=float(rng.random()), fy=float(rng.random()))
        scan = rng.uniform(0.1, 3.6, int(rng.choice((3, 90, 360)))).astype(np.float32)
        a, laser = _aligner(gpu_pkg, p)
        want = M.search(occ, geom, R.cloud(scan, laser)[0], T, p)
        _check(a, pf, slot, scan, T, want, f"seed {seed}", False)
        a.close()
    pf.close()
