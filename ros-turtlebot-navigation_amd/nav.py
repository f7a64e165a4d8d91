"""Python mirror of planner::GoalField over the C-ABI of include/tbnav_nav.h (tests / tools plumbing): the exact cost-to-go to a
goal cell over a cost grid, solved on the device, and its hand-over to an MPPI handle as a cost field.  The header is the
specification (G1-G21); the shipped host surface for ROS nodes is the C++ class in host/include/planner/goal_field.hpp.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi


def nav_cost_from_distance(dist, r_robot: float, r_inflate: float, k: float) -> np.ndarray:
    """A cost grid (uint8, the shape of `dist`, tbnav_nav.h G2) from distances to the nearest obstacle, e.g. what
    rbpf.get_occ_dist returns for one particle: 0 (blocked) where d <= r_robot; elsewhere 1 + rint(k * t * t) with
    t = (r_inflate - d) / (r_inflate - r_robot) clamped to 0 .. 1 — 1 in the open, 1 + k at the robot's radius; fp64.
    0 <= r_robot < r_inflate and 0 <= k <= 63.  (planner::navCostFromDistance is the same arithmetic, bit for bit.)"""
    if not (0.0 <= r_robot < r_inflate) or not (0.0 <= k <= 63.0):
        raise ValueError("nav_cost_from_distance: 0 <= r_robot < r_inflate and 0 <= k <= 63 are required")
    d = np.asarray(dist, dtype=np.float64)
    t = (r_inflate - d) / (r_inflate - r_robot)
    t = np.where(t > 0.0, t, 0.0)
    t = np.where(t < 1.0, t, 1.0)
    return np.where(d <= r_robot, 0.0, 1.0 + np.rint(k * t * t)).astype(np.uint8)


def inflation_tables(resolution: float, r_robot: float, r_inflate: float, k: float):
    """tbnav_nav_inflation_tables (tbnav_nav.h G7; no GPU needed): (cost, field, reach) — cost uint8 and field float32 by squared
    cell distance c = 0 .. reach**2, each FOLLOWED BY its open value (so reach**2 + 2 values)."""
    L = capi.lib()
    n, reach = C.c_int32(), C.c_int32()
    capi.check(L.tbnav_nav_inflation_tables(resolution, r_robot, r_inflate, k, None, None, 0, C.byref(n), C.byref(reach)),
               "tbnav_nav_inflation_tables")
    cost, field = np.empty(n.value + 1, dtype=np.uint8), np.empty(n.value + 1, dtype=np.float32)
    capi.check(L.tbnav_nav_inflation_tables(resolution, r_robot, r_inflate, k, cost.ctypes.data, field.ctypes.data, n.value + 1,
                                            C.byref(n), C.byref(reach)), "tbnav_nav_inflation_tables")
    assert n.value + 1 == cost.size
    return cost, field, reach.value


def gain_rays(range_cells: int) -> np.ndarray:
    """tbnav_nav_gain_rays (tbnav_nav.h G17; no GPU needed): int32 [n][2], the end points (ex, ey) of the rays in ascending order."""
    L = capi.lib()
    n = C.c_int32()
    capi.check(L.tbnav_nav_gain_rays(int(range_cells), None, 0, C.byref(n)), "tbnav_nav_gain_rays")
    ends = np.empty((n.value, 2), dtype=np.int32)
    capi.check(L.tbnav_nav_gain_rays(int(range_cells), ends.ctypes.data, n.value, C.byref(n)), "tbnav_nav_gain_rays")
    return ends


class GoalField:
    """tbnav_nav on one MI355X.  Cells are (ix, iy), arrays [nx][ny]."""

    def __init__(self, nx: int, ny: int, xmin: float, ymin: float, resolution: float, device: int = -1):
        p = capi.NavParams(nx, ny, xmin, ymin, resolution, device, 0)
        self.nx, self.ny, self.xmin, self.ymin, self.resolution = nx, ny, xmin, ymin, resolution
        self._L = capi.lib()
        self._h = C.c_void_p()
        capi.check(self._L.tbnav_nav_create(C.byref(p), C.byref(self._h)), "tbnav_nav_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tbnav_nav_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setCost(self, cost):
        """G2: uint8 [nx][ny]; what the next solve uses."""
        c = np.asarray(cost)
        if c.shape != (self.nx, self.ny) or c.dtype.kind not in "ui" or (c.size and (c.min() < 0 or c.max() > 255)):
            raise ValueError("setCost: cost must be an integer array of shape [nx][ny] with values 0 .. 255")
        c = np.ascontiguousarray(c, dtype=np.uint8)
        capi.check(self._L.tbnav_nav_set_cost(self._h, c.ctypes.data), "tbnav_nav_set_cost")

    def setCostFrom(self, pf, r_robot: float, r_inflate: float, k: float, particle=None):
        """G7-G9: the cost grid from the occupancy bits of a particle of an rtn_amd.rbpf.ParticleFilter (None: the best one, found
        on the device), formed on the device: nav_cost_from_distance(pf.occDist(p), ...) without the distance field or the host."""
        p = capi.NAV_BEST_PARTICLE if particle is None else int(particle)
        capi.check(self._L.tbnav_nav_set_cost_from_rbpf(self._h, pf._h, p, r_robot, r_inflate, k), "tbnav_nav_set_cost_from_rbpf")

    def profileCostFrom(self, pf, r_robot: float, r_inflate: float, k: float, launches: int, particle=None) -> float:
        """setCostFrom with the kernel launched `launches` times between two events: microseconds per launch (a measurement hook)."""
        p = capi.NAV_BEST_PARTICLE if particle is None else int(particle)
        ms = C.c_float()
        capi.check(self._L.tbnav_nav_profile_cost_from_rbpf(self._h, pf._h, p, r_robot, r_inflate, k, launches, C.byref(ms)),
                   "tbnav_nav_profile_cost_from_rbpf")
        return ms.value * 1e3

    def cost(self) -> np.ndarray:
        """The grid the next solve uses, however it was set."""
        c = np.empty((self.nx, self.ny), dtype=np.uint8)
        capi.check(self._L.tbnav_nav_get_cost(self._h, c.ctypes.data), "tbnav_nav_get_cost")
        return c

    def lastCostKernel(self) -> str:
        """The kernel setCostFrom launched, as a profiler prints it; "" until that route has run."""
        name = C.create_string_buffer(64)
        capi.check(self._L.tbnav_nav_last_cost_kernel(self._h, name, 64), "tbnav_nav_last_cost_kernel")
        return name.value.decode()

    def solve(self, ix: int, iy: int):
        capi.check(self._L.tbnav_nav_solve(self._h, ix, iy), "tbnav_nav_solve")

    def solveAt(self, x: float, y: float):
        """solve with the goal given in world coordinates."""
        self.solve(*self.cellOf(x, y))

    # ---- exploration frontiers as goals (tbnav_nav.h G10-G16) ----
    @staticmethod
    def _frontier_info(info) -> dict:
        return dict(found=bool(info.found), min_cells=info.min_cells, cells=info.cells, clusters=info.clusters,
                    seed_clusters=info.seed_clusters, seed_cells=info.seed_cells, rounds=info.rounds, launches=info.launches,
                    tile_visits=int(info.tile_visits))

    def findFrontiers(self, pf, min_cells: int = 8, particle=None) -> dict:
        """G10-G13 for a particle of an rtn_amd.rbpf.ParticleFilter (None: the best one, found on the device): the counts of frontier
        cells, clusters, seed clusters and seed cells, and the labelling's rounds, launches and tile visits."""
        p = capi.NAV_BEST_PARTICLE if particle is None else int(particle)
        info = capi.NavFrontierInfo()
        capi.check(self._L.tbnav_nav_find_frontiers(self._h, pf._h, p, int(min_cells), C.byref(info)), "tbnav_nav_find_frontiers")
        return self._frontier_info(info)

    def profileFindFrontiers(self, pf, min_cells: int = 8, particle=None):
        """findFrontiers with events between its stages: (info, microseconds of mark / label rounds / sizes / seeds) (a measurement hook)."""
        p = capi.NAV_BEST_PARTICLE if particle is None else int(particle)
        info, ms = capi.NavFrontierInfo(), (C.c_float * 4)()
        capi.check(self._L.tbnav_nav_profile_find_frontiers(self._h, pf._h, p, int(min_cells), C.byref(info), ms), "tbnav_nav_profile_find_frontiers")
        return self._frontier_info(info), dict(zip(("mark", "label", "sizes", "seeds"), (v * 1e3 for v in ms)))

    def lastFrontiers(self) -> dict:
        info = capi.NavFrontierInfo()
        capi.check(self._L.tbnav_nav_last_frontiers(self._h, C.byref(info)), "tbnav_nav_last_frontiers")
        return self._frontier_info(info)

    def frontierLabels(self) -> np.ndarray:
        """G12: uint32 [nx][ny], the least index ix*ny + iy of the cell's cluster; NAV_UNREACHED where the cell is no frontier cell."""
        lab = np.empty((self.nx, self.ny), dtype=np.uint32)
        capi.check(self._L.tbnav_nav_get_frontier_labels(self._h, lab.ctypes.data), "tbnav_nav_get_frontier_labels")
        return lab

    def frontiers(self) -> list:
        """G16: one dict per cluster in ascending label order: root, size, seeds, box (ix_min, iy_min, ix_max, iy_max), sum_ix, sum_iy."""
        n = C.c_int32(0)
        rc = self._L.tbnav_nav_frontier_list(self._h, None, 0, C.byref(n))
        if n.value <= 0:
            capi.check(rc, "tbnav_nav_frontier_list")
            return []
        recs = (capi.NavFrontier * n.value)()
        capi.check(self._L.tbnav_nav_frontier_list(self._h, recs, n.value, C.byref(n)), "tbnav_nav_frontier_list")
        return [dict(root=(r.root[0], r.root[1]), size=r.size, seeds=bool(r.seeds), box=tuple(r.box), sum_ix=int(r.sum_ix), sum_iy=int(r.sum_iy))
                for r in recs[:n.value]]

    def markVisited(self, ix: int, iy: int, radius_cells: int):
        """G14: the disc of radius_cells round (ix, iy) joins the visited mask."""
        capi.check(self._L.tbnav_nav_mark_visited(self._h, int(ix), int(iy), int(radius_cells)), "tbnav_nav_mark_visited")

    def clearVisited(self):
        capi.check(self._L.tbnav_nav_clear_visited(self._h), "tbnav_nav_clear_visited")

    def visited(self) -> np.ndarray:
        v = np.empty((self.nx, self.ny), dtype=np.uint8)
        capi.check(self._L.tbnav_nav_get_visited(self._h, v.ctypes.data), "tbnav_nav_get_visited")
        return v

    def solveGoals(self, cells):
        """G15: the cost-to-go to the nearest of the listed cells, [(ix, iy), ...]."""
        c = np.ascontiguousarray(np.asarray(cells, dtype=np.int32).reshape(-1, 2))
        capi.check(self._L.tbnav_nav_solve_goals(self._h, c.ctypes.data, c.shape[0]), "tbnav_nav_solve_goals")

    def solveFrontiers(self) -> bool:
        """G15 with the last find's seeds as goals, taken from the device.  False where that find left no seed: nothing left to
        explore, and the last solution stays."""
        rc = self._L.tbnav_nav_solve_frontiers(self._h)
        if rc == capi.ERR_UNSUPPORTED:
            return False
        capi.check(rc, "tbnav_nav_solve_frontiers")
        return True

    def lastFrontierKernels(self) -> list:
        """The kernels a find launches, as a profiler prints them; [] before the first find."""
        name = C.create_string_buffer(160)
        capi.check(self._L.tbnav_nav_last_frontier_kernels(self._h, name, 160), "tbnav_nav_last_frontier_kernels")
        return [k for k in name.value.decode().split(";") if k]

    # ---- frontiers ranked by what a scan from them would reveal (tbnav_nav.h G17-G20) ----
    @staticmethod
    def _gain_info(gi) -> dict:
        return dict(computed=bool(gi.computed), range_cells=gi.range_cells, rays=gi.rays, viewpoints=gi.viewpoints, gain_min=gi.gain_min,
                    gain_max=gi.gain_max, best=(gi.best[0], gi.best[1]))

    def findFrontiersGain(self, pf, range_cells: int, min_cells: int = 8, particle=None):
        """G19: findFrontiers, and in the same call the gain of every seed cell at a range of range_cells: (info, gain info)."""
        p = capi.NAV_BEST_PARTICLE if particle is None else int(particle)
        info, gi = capi.NavFrontierInfo(), capi.NavGainInfo()
        capi.check(self._L.tbnav_nav_find_frontiers_gain(self._h, pf._h, p, int(min_cells), int(range_cells), C.byref(info), C.byref(gi)),
                   "tbnav_nav_find_frontiers_gain")
        return self._frontier_info(info), self._gain_info(gi)

    def profileFindFrontiersGain(self, pf, range_cells: int, min_cells: int = 8, particle=None):
        """findFrontiersGain with events between its stages: (info, gain info, microseconds of mark / label / sizes / seeds / gain)."""
        p = capi.NAV_BEST_PARTICLE if particle is None else int(particle)
        info, gi, ms = capi.NavFrontierInfo(), capi.NavGainInfo(), (C.c_float * 5)()
        capi.check(self._L.tbnav_nav_profile_find_frontiers_gain(self._h, pf._h, p, int(min_cells), int(range_cells), C.byref(info), C.byref(gi), ms),
                   "tbnav_nav_profile_find_frontiers_gain")
        return self._frontier_info(info), self._gain_info(gi), dict(zip(("mark", "label", "sizes", "seeds", "gain"), (v * 1e3 for v in ms)))

    def lastGain(self) -> dict:
        gi = capi.NavGainInfo()
        capi.check(self._L.tbnav_nav_last_gain(self._h, C.byref(gi)), "tbnav_nav_last_gain")
        return self._gain_info(gi)

    def frontierGain(self) -> np.ndarray:
        """G18: uint32 [nx][ny], the distinct unknown cells the rays from a seed cell see; 0 where the cell is no seed."""
        gain = np.empty((self.nx, self.ny), dtype=np.uint32)
        capi.check(self._L.tbnav_nav_get_frontier_gain(self._h, gain.ctypes.data), "tbnav_nav_get_frontier_gain")
        return gain

    def frontierGainList(self) -> list:
        """G19: one dict per cluster in ascending label order: root, gain_max, best; 0 and (-1, -1) where the cluster is no seed."""
        n = C.c_int32(0)
        rc = self._L.tbnav_nav_frontier_gain_list(self._h, None, 0, C.byref(n))
        if n.value <= 0:
            capi.check(rc, "tbnav_nav_frontier_gain_list")
            return []
        recs = (capi.NavFrontierGain * n.value)()
        capi.check(self._L.tbnav_nav_frontier_gain_list(self._h, recs, n.value, C.byref(n)), "tbnav_nav_frontier_gain_list")
        return [dict(root=(r.root[0], r.root[1]), gain_max=r.gain_max, best=(r.best[0], r.best[1])) for r in recs[:n.value]]

    def solveFrontiersRanked(self, gain_weight: int) -> bool:
        """G20: every seed starts at gain_weight * (gain_max - its gain).  False where the find left no seed; the last solution stays."""
        rc = self._L.tbnav_nav_solve_frontiers_ranked(self._h, int(gain_weight))
        if rc == capi.ERR_UNSUPPORTED:
            return False
        capi.check(rc, "tbnav_nav_solve_frontiers_ranked")
        return True

    def lastGainKernels(self) -> list:
        """The gain's kernels of the last find with gain, as a profiler prints them; [] where none ran."""
        name = C.create_string_buffer(160)
        capi.check(self._L.tbnav_nav_last_gain_kernels(self._h, name, 160), "tbnav_nav_last_gain_kernels")
        return [k for k in name.value.decode().split(";") if k]

    def cellOf(self, x: float, y: float) -> tuple:
        ix, iy = C.c_int32(), C.c_int32()
        capi.check(self._L.tbnav_nav_cell_of(self._h, x, y, C.byref(ix), C.byref(iy)), "tbnav_nav_cell_of")
        return ix.value, iy.value

    def costToGo(self) -> np.ndarray:
        d = np.empty((self.nx, self.ny), dtype=np.uint32)
        capi.check(self._L.tbnav_nav_get_cost_to_go(self._h, d.ctypes.data), "tbnav_nav_get_cost_to_go")
        return d

    def field(self, cap: float) -> np.ndarray:
        v = np.empty((self.nx, self.ny), dtype=np.float32)
        capi.check(self._L.tbnav_nav_get_field(self._h, cap, v.ctypes.data), "tbnav_nav_get_field")
        return v

    def path(self, ix: int, iy: int) -> np.ndarray:
        """G6: int32 [n][2], start and goal included."""
        n = C.c_int32(0)
        rc = self._L.tbnav_nav_path(self._h, ix, iy, None, 0, C.byref(n))
        if n.value <= 0:   # (a path has a cell at least: the length query answered something else than "buffer too small")
            capi.check(rc, "tbnav_nav_path")
        cells = np.empty((n.value, 2), dtype=np.int32)
        capi.check(self._L.tbnav_nav_path(self._h, ix, iy, cells.ctypes.data, n.value, C.byref(n)), "tbnav_nav_path")
        return cells

    def lastSolve(self) -> dict:
        info, name = capi.NavSolveInfo(), C.create_string_buffer(64)
        capi.check(self._L.tbnav_nav_last_solve(self._h, C.byref(info), name, 64), "tbnav_nav_last_solve")
        return dict(solved=bool(info.solved), goal=(info.goal[0], info.goal[1]), rounds=info.rounds, launches=info.launches,
                    tiles=(info.tiles[0], info.tiles[1]), tile_visits=int(info.tile_visits), kernel=name.value.decode())

    def applyTo(self, mppi, cap: float, weight: float):
        """tbnav_nav_apply_to_mppi(_group): the field of `cap` becomes the cost field of an rtn_amd.mppi.MPPI or MPPIGroup."""
        from .mppi import MPPIGroup
        if isinstance(mppi, MPPIGroup):
            capi.check(self._L.tbnav_nav_apply_to_mppi_group(self._h, mppi._h, cap, weight), "tbnav_nav_apply_to_mppi_group")
        else:
            capi.check(self._L.tbnav_nav_apply_to_mppi(self._h, mppi._h, cap, weight), "tbnav_nav_apply_to_mppi")
