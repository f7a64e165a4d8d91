"""TEST INFRASTRUCTURE — restatement of the frontiers ranked by information gain of include/tbnav_nav.h (G17-G20), written from the
header alone.

The ring and the rays' steps are Python integers (numpy int64 where vectorised over rays and viewpoints: no value here comes near its
range), the classes come from an int8 EXPORTED map like nav_frontier_restatement's, the gain is a count over a boolean grid per viewpoint,
the ranked cost-to-go Dijkstra with a start value per seed, the walk G6 with G20's stop rule.  The wrong variants the case table must
tell apart are switches of the same functions.  Nothing in the product imports this file.
"""
from __future__ import annotations

import heapq

import numpy as np

import nav_frontier_restatement as ff
import nav_restatement as nr

UNREACHED = nr.UNREACHED
MAX_GAIN_RANGE, MAX_GAIN_WEIGHT = 128, 4096
PLANTED = ("leaky", "either", "per_ray", "trunc", "count_occ")


# ---- G17 --------------------------------------------------------------------------------------------------------------------
def ring(R):
    """[(ex, ey)] in ascending order."""
    assert 1 <= R <= MAX_GAIN_RANGE
    return [(ex, ey) for ex in range(-R, R + 1) for ey in range(-R, R + 1) if R * R - R < ex * ex + ey * ey <= R * R + R]


def ray_steps(ex, ey, trunc=False):
    """[(dx, dy)] for s = 1 .. n, Python integers.  trunc: the planted step without its + n."""
    n = max(abs(ex), abs(ey))
    sgn = lambda v: (v > 0) - (v < 0)
    half = 0 if trunc else n
    return [(sgn(ex) * ((2 * s * abs(ex) + half) // (2 * n)), sgn(ey) * ((2 * s * abs(ey) + half) // (2 * n))) for s in range(1, n + 1)]


def ray_table(R, trunc=False):
    """(DX, DY int64 [rays][R], N int64 [rays]): the steps of every ray of E(R), padded with the ray's last step."""
    ends = ring(R)
    DX, DY, N = np.zeros((len(ends), R), dtype=np.int64), np.zeros((len(ends), R), dtype=np.int64), np.zeros(len(ends), dtype=np.int64)
    for k, (ex, ey) in enumerate(ends):
        steps = ray_steps(ex, ey, trunc)
        N[k] = len(steps)
        steps += [steps[-1]] * (R - len(steps))
        DX[k], DY[k] = [s[0] for s in steps], [s[1] for s in steps]
    return DX, DY, N


_TABLES = {}


def _table(R, trunc):
    if (R, trunc) not in _TABLES:
        _TABLES[(R, trunc)] = ray_table(R, trunc)
    return _TABLES[(R, trunc)]


# ---- G18 --------------------------------------------------------------------------------------------------------------------
def classes(exported, xs):
    """(unknown, occupied) bool [xs][xs] in the nav grid's orientation from an exported map (-1 and 100)."""
    m = np.asarray(exported, dtype=np.int8).reshape(xs, xs).T
    return m == -1, m == 100


def seen(unknown, occupied, views, R, leaky=False, either=False, per_ray=False, trunc=False, count_occ=False):
    """(seen bool [views][nx][ny], counts int64 [views]) for the viewpoints [(ix, iy)].  The switches are the planted errors: no diagonal
    rule, one orthogonal cell blocks, no distinct count (counts then is the sum over the rays), the step without + n, the blocking
    occupied cell counted."""
    unknown, occupied = np.asarray(unknown, dtype=bool), np.asarray(occupied, dtype=bool)
    nx, ny = unknown.shape
    DX, DY, N = _table(R, trunc)
    views = np.asarray(views, dtype=np.int64).reshape(-1, 2)
    V, K = views.shape[0], DX.shape[0]
    out = np.zeros((V, nx, ny), dtype=bool)
    total = np.zeros(V, dtype=np.int64)
    vi = np.repeat(np.arange(V), K).reshape(V, K)
    alive = np.ones((V, K), dtype=bool)
    px, py = np.repeat(views[:, 0], K).reshape(V, K), np.repeat(views[:, 1], K).reshape(V, K)
    for s in range(R):
        alive = alive & (s < N)[None, :]
        if not alive.any():
            break
        cx, cy = views[:, 0:1] + DX[None, :, s], views[:, 1:2] + DY[None, :, s]
        inside = (cx >= 0) & (cx < nx) & (cy >= 0) & (cy < ny)
        qx, qy = np.clip(cx, 0, nx - 1), np.clip(cy, 0, ny - 1)
        hit = inside & occupied[qx, qy]
        stop = ~inside | hit
        if not leaky:
            a, b = occupied[px, qy], occupied[qx, py]          # the cells orthogonally between (px, py) and (cx, cy); inside where (cx, cy) is
            stop |= inside & (cx != px) & (cy != py) & ((a | b) if either else (a & b))
        if count_occ:
            m = alive & hit
            out[vi[m], qx[m], qy[m]] = True
            np.add.at(total, vi[m], 1)
        alive = alive & ~stop
        m = alive & unknown[qx, qy]
        out[vi[m], qx[m], qy[m]] = True
        np.add.at(total, vi[m], 1)
        px, py = np.where(alive, qx, px), np.where(alive, qy, py)
    return out, (total if per_ray else out.reshape(V, -1).sum(axis=1))


def gain_map(unknown, occupied, seed, R, chunk=48, **wrong):
    """uint32 [nx][ny]: the gain at every seed cell, 0 elsewhere (G19)."""
    seed = np.asarray(seed, dtype=bool)
    gain = np.zeros(seed.shape, dtype=np.uint32)
    cells = np.argwhere(seed)
    for k in range(0, len(cells), chunk):
        part = cells[k:k + chunk]
        gain[part[:, 0], part[:, 1]] = seen(unknown, occupied, part, R, **wrong)[1]
    return gain


# ---- G19 --------------------------------------------------------------------------------------------------------------------
def gain_info(gain, seed, R):
    """The fields of tbnav_nav_gain_info."""
    seed = np.asarray(seed, dtype=bool)
    ny = seed.shape[1]
    if not seed.any():
        return dict(computed=True, range_cells=R, rays=len(ring(R)), viewpoints=0, gain_min=0, gain_max=0, best=(-1, -1))
    g = np.asarray(gain)[seed]
    top = int(g.max())
    best = int(np.flatnonzero(seed.reshape(-1) & (np.asarray(gain).reshape(-1) == top))[0])
    return dict(computed=True, range_cells=R, rays=len(ring(R)), viewpoints=int(seed.sum()), gain_min=int(g.min()), gain_max=top,
                best=(best // ny, best % ny))


def gain_list(lab, gain, min_cells):
    """One dict per cluster in ascending label order: root, gain_max, best; 0 and (-1, -1) where the cluster is no seed."""
    lab, gain = np.asarray(lab), np.asarray(gain)
    ny = lab.shape[1]
    out = []
    for root in np.unique(lab[lab != UNREACHED]):
        member = (lab == root).reshape(-1)
        rec = dict(root=(int(root) // ny, int(root) % ny), gain_max=0, best=(-1, -1))
        if int(member.sum()) >= min_cells:
            top = int(gain.reshape(-1)[member].max())
            best = int(np.flatnonzero(member & (gain.reshape(-1) == top))[0])
            rec.update(gain_max=top, best=(best // ny, best % ny))
        out.append(rec)
    return out


# ---- G20 --------------------------------------------------------------------------------------------------------------------
def start_values(gain, seed, weight):
    """uint32 [nx][ny]: weight * (gain_max - gain) at the seeds, UNREACHED elsewhere."""
    assert 0 <= weight <= MAX_GAIN_WEIGHT
    seed = np.asarray(seed, dtype=bool)
    g = np.asarray(gain).astype(np.int64)
    top = int(g[seed].max())
    out = np.full(seed.shape, UNREACHED, dtype=np.int64)
    out[seed] = weight * (top - g[seed])
    assert int(out[seed].max()) <= MAX_GAIN_WEIGHT * ((2 * MAX_GAIN_RANGE + 1) ** 2 - 1)
    return out.astype(np.uint32)


def cost_to_go_ranked(cost, start):
    """uint32 [nx][ny]: d[a] = min(start[a], min over allowed moves a -> b of d[b] + w * cost[b]) — Dijkstra from every seed at once with its
    start value as the first key, Python integers."""
    cost = np.asarray(cost)
    nx, ny = cost.shape
    c = [[int(v) for v in row] for row in cost]
    d = [[int(v) for v in row] for row in np.asarray(start)]
    heap = [(d[x][y], x, y) for x in range(nx) for y in range(ny) if d[x][y] != UNREACHED]
    assert heap and all(c[x][y] != 0 for _, x, y in heap), "G20: every seed is a passable cell (G11)"
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
    assert int(out[out != UNREACHED].max()) < UNREACHED     # G20: it cannot overflow
    return out.astype(np.uint32)


def path_ranked(cost, d, start, cell, stop_at_zero=False):
    """G6 with G20's stop rule: int32 [n][2] from `cell` to the first seed whose d equals its own start value.  Raises ValueError where the
    header says TBNAV_ERR_UNSUPPORTED.  stop_at_zero: the planted old rule, d == 0 — where the walk then stands on a cell none of whose
    moves explains its d, it raises RuntimeError."""
    cost = np.asarray(cost)
    nx, ny = cost.shape
    c = [[int(v) for v in row] for row in cost]
    dd = [[int(v) for v in row] for row in np.asarray(d)]
    st = [[int(v) for v in row] for row in np.asarray(start)]
    ax, ay = cell
    if c[ax][ay] == 0 or dd[ax][ay] == UNREACHED:
        raise ValueError("G6: the start is blocked or unreached")
    cells = [(ax, ay)]
    while (dd[ax][ay] != 0) if stop_at_zero else not (st[ax][ay] != UNREACHED and dd[ax][ay] == st[ax][ay]):
        vals = []
        for dx, dy, w in nr.MOVES:
            if nr._allowed(c, nx, ny, ax, ay, dx, dy) and dd[ax + dx][ay + dy] != UNREACHED:
                vals.append((dd[ax + dx][ay + dy] + w * c[ax + dx][ay + dy], dx, dy))
        best = min(v for v, _, _ in vals) if vals else None
        if best != dd[ax][ay]:
            assert stop_at_zero
            raise RuntimeError("the walk passed the seed it had reached")
        dx, dy = [(dx, dy) for v, dx, dy in vals if v == best][0]
        ax, ay = ax + dx, ay + dy
        cells.append((ax, ay))
        assert len(cells) <= nx * ny
    return np.array(cells, dtype=np.int32)


# ---- all of it for one map --------------------------------------------------------------------------------------------------
def find_gain(exported, xs, cost, visited, min_cells, R, **wrong):
    """G10-G13 (nav_frontier_restatement.find) and G17-G19: (frontier, labels, seeds, gain)."""
    front, lab, seed = ff.find(exported, xs, cost, visited, min_cells)
    unknown, occupied = classes(exported, xs)
    return front, lab, seed, gain_map(unknown, occupied, seed, R, **wrong)
