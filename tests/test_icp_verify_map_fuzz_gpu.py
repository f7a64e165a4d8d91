"""30 drawn cases of the map check (include/tbnav_icp.h MAP CHECK; csrc/icp_verify_map.hip) against the restatement with == on every
field of the record and of the per-beam hook: maps of 64 to 130 cells with drawn walls (axis-parallel and diagonal, the latter only
8-connected), free discs, cells known and neither, and whole tiles nobody has written; the pose anywhere in the map, a sensor offset
in half of them, drawn ranges with holes, and H, k and the three thresholds drawn inside their limits.  The seed is fixed: the cases are
the same on every run."""
import numpy as np
import pytest

import icp_restatement as R
import icp_search_map_restatement as M
import icp_verify_map_restatement as V
from nav_frontier_cases import F, K, O, U
from test_icp_verify_map_gpu import _aligner, _check, _classes_of, _filter, _set_lo

pytestmark = pytest.mark.gpu
SEED, DRAWS = 20261, 30
SIDES = (64, 80, 98, 110, 130)      # (sides whose ceil((xmax - xmin) / resolution) is the side itself in fp64)
RES = 0.05


def draw_map(rng, side):
    lo = rng.choice(np.array([F, K]), size=(side, side), p=[0.7, 0.3])
    for _ in range(int(rng.integers(1, 5))):          # free discs
        ci, cj, r = rng.integers(0, side), rng.integers(0, side), rng.integers(5, 21)
        ii, jj = np.ogrid[:side, :side]
        lo[(ii - ci) ** 2 + (jj - cj) ** 2 <= r * r] = F
    for _ in range(int(rng.integers(2, 9))):          # walls
        i, j, n = int(rng.integers(0, side)), int(rng.integers(0, side)), int(rng.integers(3, 40))
        di, dj = ((1, 0), (0, 1), (1, 1), (1, -1))[int(rng.integers(0, 4))]
        for q in range(n):
            if 0 <= i + q * di < side and 0 <= j + q * dj < side:
                lo[i + q * di, j + q * dj] = O
    tiles = -(-side // 32)
    for ti in range(tiles):                            # tiles nobody has written
        for tj in range(tiles):
            if rng.random() < 0.25:
                lo[32 * ti:32 * ti + 32, 32 * tj:32 * tj + 32] = U
    return lo


def draw(rng, i):
    side = SIDES[i % len(SIDES)]
    geom = M.Geom(-0.5 * side * RES, -0.5 * side * RES, RES, side)
    q10 = lambda open_: int(rng.integers(0, 1025)) if rng.random() < 0.5 else open_      # half of the draws leave a threshold open
    p = V.Params(half_cells=int(rng.integers(8, 129)), slack_cells=int(rng.integers(0, 9)), max_through_q10=q10(1024), max_missing_q10=q10(1024),
                 min_hit_q10=q10(0))
    lo = draw_map(rng, side)
    Trs = (float(rng.uniform(-3.0, 3.0)), float(rng.uniform(-0.2, 0.2)), float(rng.uniform(-0.2, 0.2))) if i % 2 else (0.0, 0.0, 0.0)
    T = (float(rng.uniform(-3.2, 3.2)), float(rng.uniform(geom.xmin + 0.3, -geom.xmin - 0.3)), float(rng.uniform(geom.ymin + 0.3, -geom.ymin - 0.3)))
    n_beams = int(rng.choice([1, 17, 256, 360, 500, 1080]))
    scan = rng.uniform(0.1, min(1.2 * p.half_cells * RES, 3.6), n_beams).astype(np.float32)
    scan[rng.random(n_beams) < 0.05] = np.nan
    return side, geom, lo, p, T, scan, Trs


def test_thirty_drawn_cases_equal_the_restatement(gpu_pkg):
    rng = np.random.default_rng(SEED)
    draws = [draw(rng, i) for i in range(DRAWS)]
    classes, accepted = set(), set()
    for side in SIDES:
        mine = [d for d in draws if d[0] == side]
        pf = _filter(gpu_pkg, mine[0][1], N=len(mine) + 1)
        for slot, (_, geom, lo, p, T, scan, Trs) in enumerate(mine, start=1):      # a slot of its own: an all-zero tile stays id 0
            _set_lo(pf, slot, lo)
            a, laser = _aligner(gpu_pkg, dict(Trs=Trs))
            cloud, beam = R.cloud(scan, laser, Trs)
            want = V.verify(_classes_of(pf, slot), geom, cloud, beam, scan.size, T, p, V.origin_of(Trs))
            assert want is not None
            classes |= set(want.beams["cls"].tolist())
            accepted.add(want.info["accepted"])
            _check(a, pf, slot, scan, T, p, want, f"side {side} slot {slot}: {p} T = {T} Trs = {Trs} beams = {scan.size}")
            a.close()
        pf.close()
    assert classes == set(range(7)) and accepted == {0, 1}, (classes, accepted)
