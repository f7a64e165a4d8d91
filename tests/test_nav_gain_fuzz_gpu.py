"""Drawn maps for the frontiers ranked by information gain (include/tbnav_nav.h G17-G20): 30 maps of blobs of each of
nav_frontier_cases.VALUES' five classes (tests/test_nav_frontier_fuzz_gpu.py's draw: even sides 34 .. 130, holes in the cost grid, visited
discs, min_cells 1 .. 20), each with a drawn range 1 .. 128 — a third of them either side of the kernels' threshold — and a drawn weight
0 .. 4096, fixed seeds — the same == as tests/test_nav_gain_gpu.py."""
import numpy as np
import pytest

import nav_frontier_check as ck
import nav_gain_check as gk
import nav_gain_restatement as gr
from test_nav_frontier_fuzz_gpu import draw

pytestmark = pytest.mark.gpu

N_MAPS, GROUP = 30, 6


def draw_gain(seed):
    rng = np.random.default_rng(17000 + seed)
    R = int(rng.choice((rng.integers(1, 129), rng.integers(28, 37), rng.integers(1, 12))))
    weight = int(rng.choice((rng.integers(0, 4097), rng.integers(0, 4), 4096)))
    return R, weight


@pytest.mark.parametrize("group", range(N_MAPS // GROUP))
def test_drawn_maps_equal_the_restatement(gpu_pkg, group):
    from rtn_amd.nav import GoalField
    from rtn_amd.rbpf import ParticleFilter, default_params
    views, large, small = 0, 0, 0
    for seed in range(group * GROUP, (group + 1) * GROUP):
        xs, lo, cost, discs, min_cells = draw(seed)
        R, weight = draw_gain(seed)
        half = (xs - 0.5) * 0.05 / 2       # the filter's side is ceil(extent / resolution): half a cell short of xs cells rounds up to xs
        pf = ParticleFilter(default_params(N=1, k=2, map_min=-half, map_max=half, resolution=0.05))
        assert (pf.xsize, pf.ysize) == (xs, xs), seed
        nav = GoalField(xs, xs, -half, -half, 0.05)
        pf.setLogOdds(0, lo.reshape(-1))
        mask = ck.install(nav, cost, discs)
        want = gr.find_gain(pf.particleMap(0), xs, cost, mask, min_cells, R)
        info, gi = gk.check_find_gain(nav, pf, 0, min_cells, R, want, ("fuzz", seed, R))
        if want[2].any():
            gk.check_ranked(nav, cost, want[2], want[3], 0.05, weight, ("fuzz", seed, R, weight))
        else:
            assert nav.solveFrontiersRanked(weight) is False
        views += gi["viewpoints"]
        large += R > 32
        small += R <= 32
        nav.close(); pf.close()
    assert views > 0 and small > 0
