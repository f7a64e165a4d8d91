"""30 drawn cases of the map alignment (include/tbnav_icp.h MAP ALIGNMENT; csrc/icp_align_map.hip) against the restatement with ==:
maps of at most 96 cells, at most 360 beams, every parameter drawn inside its limits, the pose anywhere in the map, a room of drawn
size with drawn clutter.  The seed is fixed: the cases are the same on every run."""
import numpy as np
import pytest

import icp_align_map_cases as ac
import icp_align_map_restatement as A
import icp_restatement as R
import nav_from_map_cases as fc
from test_icp_align_map_gpu import _aligner, _check, _filter, _occ_of, _set_occ

pytestmark = pytest.mark.gpu
SEED, DRAWS = 20260, 30


def draw(rng, i):
    size_id = ("s64", "s80", "s96", "r20")[i % 4]
    s = fc.SIZE[size_id]
    side = s.xsize
    p = A.Params(half_cells=int(rng.integers(8, 65)), gate_cells=int(rng.integers(1, 17)), feature_cells=int(rng.integers(1, 5)),
                 max_flatness=float(rng.choice([0.0, 0.1, 0.25, 0.5, 0.9])))
    cx, cy = (int(v) for v in rng.integers(0, side, 2))
    h = int(rng.integers(2, 4)) if size_id == "r20" else int(rng.integers(3, 12))
    occ = ac.box_occ(size_id, cx, cy, h)()
    occ |= (rng.random((side, side)) < rng.choice([0.0, 0.01, 0.05])).astype(np.uint8)
    truth = ac.centre(size_id, cx, cy, th=float(rng.uniform(-3.2, 3.2)))
    n_beams = int(rng.integers(1, 361))
    scan = ac.cast(truth, ac.box_walls(size_id, cx, cy, h), n_beams)
    scan = (scan + rng.normal(0.0, 0.2 * s.res, n_beams)).astype(np.float32)
    scan[rng.random(n_beams) < 0.05] = np.nan
    T = (truth[0] + rng.uniform(-0.05, 0.05), truth[1] + rng.uniform(-0.5, 0.5) * s.res, truth[2] + rng.uniform(-0.5, 0.5) * s.res)
    if ac.geom(size_id) and A.cell_of(ac.geom(size_id), T[1], T[2]) is None:
        T = truth
    icp = dict(ac.ICP, max_iter=int(rng.choice([1, 2, 5, 30])))
    return size_id, occ, p, T, scan, icp


def test_thirty_drawn_cases_equal_the_restatement(gpu_pkg):
    rng = np.random.default_rng(SEED)
    draws = [draw(rng, i) for i in range(DRAWS)]
    crits = set()
    for size_id in ("s64", "s80", "s96", "r20"):
        geom = ac.geom(size_id)
        pf = _filter(gpu_pkg, geom, N=2)
        for i, (sid, occ, p, T, scan, icp) in enumerate(draws):
            if sid != size_id:
                continue
            _set_occ(pf, 1, occ)
            assert np.array_equal(_occ_of(pf, 1), occ)
            a, laser = _aligner(gpu_pkg, icp)
            cloud, beam = R.cloud(scan, laser)
            want = A.align(occ, geom, cloud, beam, scan.size, T, p, **icp)
            crits.add(want.criterion)
            _check(a, pf, 1, scan, T, p, want, f"draw {i}: {size_id} {p} T = {T} beams = {scan.size} {icp}")
            a.close()
        pf.close()
    assert len(crits) >= 3, crits
