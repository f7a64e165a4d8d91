"""Drawn maps for the exploration frontiers (include/tbnav_nav.h G10-G16): 30 maps of blobs of each class, even sides 34 .. 130 (the filter refuses an odd side), random holes
in the cost grid, random visited discs, min_cells 1 .. 20, fixed seeds — the same == as tests/test_nav_frontier_gpu.py."""
import numpy as np
import pytest

import nav_frontier_cases as cs
import nav_frontier_check as ck

pytestmark = pytest.mark.gpu

N_MAPS, GROUP = 30, 6


def draw(seed):
    rng = np.random.default_rng(9000 + seed)
    xs = 2 * int(rng.integers(17, 66))       # 34 .. 130: the filter takes even sides only
    lo = np.zeros((xs, xs))
    for _ in range(int(rng.integers(6, 30))):       # blobs: discs and boxes of one class each, later ones over earlier ones
        v = cs.VALUES[int(rng.choice(5, p=(0.25, 0.3, 0.15, 0.15, 0.15)))]
        cx, cy, r = int(rng.integers(xs)), int(rng.integers(xs)), int(rng.integers(1, max(3, xs // 3)))
        if rng.random() < 0.5:
            X, Y = np.meshgrid(np.arange(xs), np.arange(xs), indexing="ij")
            lo[(X - cx) ** 2 + (Y - cy) ** 2 <= r * r] = v
        else:
            lo[max(0, cx - r):cx + r, max(0, cy - r // 2):cy + r // 2 + 1] = v
    cost = rng.integers(1, 10, (xs, xs)).astype(np.uint8)
    cost[rng.random((xs, xs)) < rng.choice((0.0, 0.02, 0.15))] = 0
    discs = tuple((int(rng.integers(xs)), int(rng.integers(xs)), int(rng.integers(0, 12))) for _ in range(int(rng.integers(0, 4))))
    return xs, lo, cost, discs, int(rng.integers(1, 21))


@pytest.mark.parametrize("group", range(N_MAPS // GROUP))
def test_drawn_maps_equal_the_restatement(gpu_pkg, group):
    from rtn_amd.nav import GoalField
    from rtn_amd.rbpf import ParticleFilter, default_params
    seen = 0
    for seed in range(group * GROUP, (group + 1) * GROUP):
        xs, lo, cost, discs, min_cells = draw(seed)
        half = (xs - 0.5) * 0.05 / 2       # the filter's side is ceil(extent / resolution): half a cell short of xs cells rounds up to xs
        pf = ParticleFilter(default_params(N=1, k=2, map_min=-half, map_max=half, resolution=0.05))
        assert (pf.xsize, pf.ysize) == (xs, xs), seed
        nav = GoalField(xs, xs, -half, -half, 0.05)
        pf.setLogOdds(0, lo.reshape(-1))
        mask = ck.install(nav, cost, discs)
        info, front, lab, seed_cells = ck.check_find(nav, pf, 0, cost, mask, min_cells, ("fuzz", seed))
        ck.check_solves(nav, cost, seed_cells, 0.05, ("fuzz", seed))
        seen += info["cells"]
        nav.close(); pf.close()
    assert seen > 0
