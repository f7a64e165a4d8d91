"""TEST INFRASTRUCTURE — restatement of the exploration frontiers of include/tbnav_nav.h (G10-G16), written from the header alone.

Classes come from an int8 EXPORTED map (GridMapper::gridMap / tbnav_rbpf_particle_map: the nav grid transposed), clusters from a flood
fill, sizes and seeds from counting, the cost-to-go to the nearest of several goals from Dijkstra in Python integers (with one goal it
must equal nav_restatement.cost_to_go).  The wrong variants the case table must tell apart are switches of the same functions.  Nothing
in the product imports this file.
"""
from __future__ import annotations

import heapq
import math

import numpy as np

import nav_restatement as nr

UNREACHED = nr.UNREACHED
MAX_VISIT_RADIUS = 64
N4 = ((-1, 0), (1, 0), (0, -1), (0, 1))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


# ---- G10 --------------------------------------------------------------------------------------------------------------------
def export_value(l):
    """GridMapper::gridMap's value of one log-odds (grid_mapper.hpp:27-30 for the probability): what the CPU tests export a case's
    log-odds with; on the device the filter's own export is the definition."""
    prob = 1 - (1 / (1 + math.exp(l)))
    if prob == 0.5:
        return -1
    if prob >= 0.90:
        return 100
    if prob <= 0.35:
        return 0
    return int(prob * 100)


def export_map(log_odds):
    """int8 [G]: the exported map of a log-odds grid [xs][xs] (x slow) — TRANSPOSED, as the filter hands it out."""
    lo = np.asarray(log_odds, dtype=np.float64)
    vals = {float(v): export_value(float(v)) for v in np.unique(lo)}
    out = np.vectorize(lambda v: vals[float(v)], otypes=[np.int8])(lo)
    return np.ascontiguousarray(out.T).reshape(-1)


def classes(exported, xs):
    """(unknown, free) bool [xs][xs] in the nav grid's orientation from an exported map."""
    m = np.asarray(exported, dtype=np.int8).reshape(xs, xs).T
    return m == -1, m == 0


# ---- G11 --------------------------------------------------------------------------------------------------------------------
def frontier_cells(unknown, free, cost, visited=None, look8=False, outside_unknown=False, keep_blocked=False):
    """bool [nx][ny].  The switches are the planted errors: the 8-neighbour look, outside-the-grid counted as unknown, a blocked cell
    kept."""
    unknown, free, cost = np.asarray(unknown, dtype=bool), np.asarray(free, dtype=bool), np.asarray(cost)
    nx, ny = unknown.shape
    pad = np.full((nx + 2, ny + 2), bool(outside_unknown))
    pad[1:-1, 1:-1] = unknown
    near = np.zeros((nx, ny), dtype=bool)
    for dx, dy in (N8 if look8 else N4):
        near |= pad[1 + dx:1 + dx + nx, 1 + dy:1 + dy + ny]
    f = free & near
    if not keep_blocked:
        f &= cost != 0
    if visited is not None:
        f &= ~np.asarray(visited, dtype=bool)
    return f


# ---- G12 --------------------------------------------------------------------------------------------------------------------
def labels(front, conn4=False):
    """uint32 [nx][ny]: the least index ix*ny + iy of the cell's component, UNREACHED off the frontier.  A flood fill from every
    unlabelled frontier cell in ascending index order: the cell a fill starts from is its component's least."""
    front = np.asarray(front, dtype=bool)
    nx, ny = front.shape
    lab = [[UNREACHED] * ny for _ in range(nx)]
    nb = N4 if conn4 else N8
    for ix in range(nx):
        for iy in range(ny):
            if not front[ix, iy] or lab[ix][iy] != UNREACHED:
                continue
            root = ix * ny + iy
            lab[ix][iy] = root
            stack = [(ix, iy)]
            while stack:
                ax, ay = stack.pop()
                for dx, dy in nb:
                    bx, by = ax + dx, ay + dy
                    if 0 <= bx < nx and 0 <= by < ny and front[bx, by] and lab[bx][by] == UNREACHED:
                        lab[bx][by] = root
                        stack.append((bx, by))
    return np.array(lab, dtype=np.uint32)


# ---- G13, G16 ---------------------------------------------------------------------------------------------------------------
def frontier_list(lab, min_cells, strict=False):
    """One dict per cluster in ascending label order (the fields of tbnav_nav_frontier).  strict: the planted `>` for `>=`."""
    assert min_cells >= 1
    lab = np.asarray(lab)
    nx, ny = lab.shape
    out = []
    for root in np.unique(lab[lab != UNREACHED]):
        ix, iy = np.nonzero(lab == root)
        size = int(ix.size)
        out.append(dict(root=(int(root) // ny, int(root) % ny), size=size, seeds=(size > min_cells) if strict else (size >= min_cells),
                        box=(int(ix.min()), int(iy.min()), int(ix.max()), int(iy.max())), sum_ix=int(ix.sum()), sum_iy=int(iy.sum())))
    return out


def seeds(lab, min_cells, strict=False):
    """bool [nx][ny]: the cells of the clusters that are large enough."""
    lab = np.asarray(lab)
    ny = lab.shape[1]
    keep = [f["root"][0] * ny + f["root"][1] for f in frontier_list(lab, min_cells, strict) if f["seeds"]]
    return np.isin(lab, np.array(keep, dtype=np.uint32)) & (lab != UNREACHED)


def counts(lab, min_cells):
    fl = frontier_list(lab, min_cells)
    return dict(cells=int((np.asarray(lab) != UNREACHED).sum()), clusters=len(fl), seed_clusters=sum(f["seeds"] for f in fl),
                seed_cells=sum(f["size"] for f in fl if f["seeds"]))


def find(exported, xs, cost, visited, min_cells, **wrong):
    """G10-G13 in one go: (frontier bool, labels, seeds bool).  wrong: look8 / outside_unknown / keep_blocked / conn4 / strict."""
    unknown, free = classes(exported, xs)
    front = frontier_cells(unknown, free, cost, visited, look8=wrong.get("look8", False), outside_unknown=wrong.get("outside_unknown", False),
                           keep_blocked=wrong.get("keep_blocked", False))
    lab = labels(front, conn4=wrong.get("conn4", False))
    return front, lab, seeds(lab, min_cells, strict=wrong.get("strict", False))


# ---- G14 --------------------------------------------------------------------------------------------------------------------
def disc(nx, ny, ix, iy, radius):
    """bool [nx][ny]: dix^2 + diy^2 <= radius^2 round (ix, iy), cut at the grid."""
    assert 0 <= ix < nx and 0 <= iy < ny and 0 <= radius <= MAX_VISIT_RADIUS
    X, Y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return (X - ix) ** 2 + (Y - iy) ** 2 <= radius * radius


# ---- G15 --------------------------------------------------------------------------------------------------------------------
def cost_to_go_goals(cost, goals):
    """uint32 [nx][ny]: d = 0 at every goal, G3-G4 otherwise — Dijkstra from all goals at once, Python integers."""
    cost = np.asarray(cost)
    nx, ny = cost.shape
    c = [[int(v) for v in row] for row in cost]
    goals = [(int(gx), int(gy)) for gx, gy in goals]
    assert goals and all(0 <= gx < nx and 0 <= gy < ny and c[gx][gy] != 0 for gx, gy in goals), "G15: every goal is a non-blocked cell of the grid"
    d = [[UNREACHED] * ny for _ in range(nx)]
    heap = []
    for gx, gy in goals:
        if d[gx][gy] != 0:
            d[gx][gy] = 0
            heap.append((0, gx, gy))
    heapq.heapify(heap)
    while heap:
        db, bx, by = heapq.heappop(heap)
        if db != d[bx][by]:
            continue
        cb = c[bx][by]
        for dx, dy, w in nr.MOVES:
            ax, ay = bx - dx, by - dy
            if 0 <= ax < nx and 0 <= ay < ny and nr._allowed(c, nx, ny, ax, ay, dx, dy):
                v = db + w * cb
                if v < d[ax][ay]:
                    d[ax][ay] = v
                    heapq.heappush(heap, (v, ax, ay))
    out = np.array(d, dtype=np.uint64)
    assert int(out[out != UNREACHED].max()) < UNREACHED
    return out.astype(np.uint32)


def goal_cells(mask):
    """[(ix, iy)] of a bool grid, ascending index."""
    return [(int(a), int(b)) for a, b in np.argwhere(np.asarray(mask, dtype=bool))]
