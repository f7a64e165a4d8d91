"""numpy restatement of the device ICP's POINT-TO-LINE METRIC (include/tbnav_icp.h, that section of the contract), beside
icp_restatement.py, which restates the point metric.  This metric has no counterpart in the reference (which only ever runs
PCL's point-to-point ICP): the header is the specification, and this file spells it with every rounding so that the GPU
tests can hold the kernel (csrc/icp.hip, icp_align<LineMetric>) to it bit for bit.

Shared with the point metric and imported from icp_restatement: the cloud, the initial guess, the transformed source
points, the nearest-neighbour search, the distance gate, the summation order, the composition, the stopping rules.
New here: the target normals, the gate "the nearest target has a normal", the ten sums and the 3x3 step.
"""
from __future__ import annotations

import math

import numpy as np

from icp_restatement import (ABS_MSE, DBL_MAX, DEGENERATE, F32, ITERATIONS, NO_CORRESPONDENCES, NOT_RUN, REL_MSE, TRANSFORM,
                             Laser, Result, _tree_sum, cloud)

NORMAL_WINDOW = 1          # TBNAV_ICP_LINE_NORMAL_WINDOW
NORMAL_MAX_GAP = 0.25      # TBNAV_ICP_LINE_NORMAL_MAX_GAP
MIN_COND = 1e-6            # TBNAV_ICP_LINE_MIN_COND
MAX_WINDOW = 16            # TBNAV_ICP_LINE_MAX_WINDOW
MAX_BEAMS = 2048           # TBNAV_ICP_LINE_MAX_BEAMS


def cloud_normals(pts, beam, n_beams, window=NORMAL_WINDOW, max_gap=NORMAL_MAX_GAP):
    """Normals of a cloud taken as a target: pts float32 [m][2] in beam order with the beam index of each point ->
    (normals float32 [m][2], has bool [m]); a point without a normal holds (0, 0)."""
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    beam = np.asarray(beam, dtype=np.int64)
    m = pts.shape[0]
    at = np.full(n_beams, -1, dtype=np.int64)      # beam -> point
    at[beam] = np.arange(m)
    g2 = max_gap * max_gap
    nrm = np.zeros((m, 2), dtype=np.float32)
    has = np.zeros(m, dtype=bool)

    def near(k, j):
        if at[j] < 0:
            return False
        dx = pts[at[j], 0] - pts[k, 0]              # float32 throughout, as in the search
        dy = pts[at[j], 1] - pts[k, 1]
        return float(F32(F32(dx * dx) + F32(dy * dy))) <= g2

    for k in range(m):
        i = int(beam[k])
        lo = hi = i
        for j in range(max(0, i - window), i):                       # the LOWEST index below i
            if near(k, j):
                lo = j
                break
        for j in range(min(n_beams - 1, i + window), i, -1):         # the HIGHEST index above i
            if near(k, j):
                hi = j
                break
        if lo == hi:
            continue
        tx = float(pts[at[hi], 0]) - float(pts[at[lo], 0])
        ty = float(pts[at[hi], 1]) - float(pts[at[lo], 1])
        l = math.sqrt((tx * tx) + (ty * ty))
        if l == 0.0:
            continue
        nrm[k] = (F32(-ty / l), F32(tx / l))
        has[k] = True
    return nrm, has


def normals(scan, laser: Laser, Trs=(0.0, 0.0, 0.0), window=NORMAL_WINDOW, max_gap=NORMAL_MAX_GAP):
    """tbnav_icp_normals: per BEAM of one scan taken as a target -> (nxy float32 [n_beams][2], has int32 [n_beams]); a beam
    without a normal (an invalid beam included) holds (0, 0) and 0."""
    scan = np.asarray(scan, dtype=np.float32)
    pts, beam = cloud(scan, laser, Trs)
    nrm, has = cloud_normals(pts, beam, scan.size, window, max_gap)
    nxy = np.zeros((scan.size, 2), dtype=np.float32)
    flag = np.zeros(scan.size, dtype=np.int32)
    nxy[beam] = nrm
    flag[beam] = has
    return nxy, flag


def match(target_scan, source_scan, laser: Laser, T_init, Trs=(0.0, 0.0, 0.0), max_iter=100, max_corr_dist=0.5,
          transform_eps=1e-8, fitness_eps=1e-6, B=256, window=NORMAL_WINDOW, max_gap=NORMAL_MAX_GAP) -> Result:
    """tbnav_icp_match with TBNAV_ICP_METRIC_LINE on the clouds of two scans from T_init = (theta, x, y)."""
    tgt, tgt_beam = cloud(target_scan, laser, Trs)
    src, src_beam = cloud(source_scan, laser, Trs)
    return match_clouds(tgt, tgt_beam, src, src_beam, np.asarray(source_scan).size, T_init, max_iter, max_corr_dist,
                        transform_eps, fitness_eps, B, window, max_gap)


def match_clouds(tgt, tgt_beam, src, src_beam, n_beams, T_init, max_iter=100, max_corr_dist=0.5, transform_eps=1e-8,
                 fitness_eps=1e-6, B=256, window=NORMAL_WINDOW, max_gap=NORMAL_MAX_GAP) -> Result:
    """The iteration on explicit clouds (float32 [m][2] in beam order, each with its beam indices)."""
    tgt = np.asarray(tgt, dtype=np.float32).reshape(-1, 2)
    src = np.asarray(src, dtype=np.float32).reshape(-1, 2)
    src_beam = np.asarray(src_beam, dtype=np.int64)
    nrm, has = cloud_normals(tgt, tgt_beam, n_beams, window, max_gap)
    c0, s0 = float(F32(math.cos(T_init[0]))), float(F32(math.sin(T_init[0])))
    R = [[c0, -s0], [s0, c0]]
    t = [float(F32(T_init[1])), float(F32(T_init[2]))]
    max2 = max_corr_dist * max_corr_dist
    prev = DBL_MAX
    sx, sy = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64)
    thread = src_beam % B
    rnd = src_beam // B
    rounds = (n_beams + B - 1) // B
    k = 0
    while True:
        k += 1
        ax = (((R[0][0] * sx) + (R[0][1] * sy)) + t[0]).astype(np.float32)
        ay = (((R[1][0] * sx) + (R[1][1] * sy)) + t[1]).astype(np.float32)
        if tgt.shape[0] > 0 and src.shape[0] > 0:
            dx = ax[:, None] - tgt[None, :, 0]
            dy = ay[:, None] - tgt[None, :, 1]
            d = dx * dx + dy * dy                                  # float32 throughout
            j = np.argmin(d, axis=1)                               # first of equal minima = lowest index
            dmin = d[np.arange(d.shape[0]), j]
            keep = (dmin.astype(np.float64) <= max2) & has[j]      # the nearest target, whether or not it has a normal
        else:
            keep = np.zeros(src.shape[0], dtype=bool)
            j = np.zeros(src.shape[0], dtype=np.int64)
        n = int(keep.sum())
        if n < 3:
            return Result(False, (0.0, 0.0, 0.0), k, n, 0.0, NO_CORRESPONDENCES)
        a64x, a64y = ax.astype(np.float64), ay.astype(np.float64)
        b64x, b64y = tgt[j, 0].astype(np.float64), tgt[j, 1].astype(np.float64)
        nx, ny = nrm[j, 0].astype(np.float64), nrm[j, 1].astype(np.float64)
        ex, ey = a64x - b64x, a64y - b64y
        r = (nx * ex) + (ny * ey)
        jj = (a64x * ny) - (a64y * nx)
        vals = [jj * jj, jj * nx, jj * ny, nx * nx, nx * ny, ny * ny, jj * r, nx * r, ny * r, r * r]
        tot = []
        for v in vals:
            partial = np.zeros(B)
            for q in range(rounds):   # each thread adds its q-th beam (if kept) in increasing beam order
                sel = keep & (rnd == q)
                partial[thread[sel]] = partial[thread[sel]] + v[sel]
            tot.append(_tree_sum(partial))
        H00, H01, H02, H11, H12, H22, g0, g1, g2, Sr = tot
        mse = Sr / float(n)
        tr = H11 + H22
        det = (H11 * H22) - (H12 * H12)
        if not det > MIN_COND * (tr * tr):
            return Result(False, (0.0, 0.0, 0.0), k, n, mse, DEGENERATE)
        v1 = ((H22 * H01) - (H12 * H02)) / det
        v2 = ((H11 * H02) - (H12 * H01)) / det
        dth = H00 - ((H01 * v1) + (H02 * v2))
        if not dth > MIN_COND * H00:
            return Result(False, (0.0, 0.0, 0.0), k, n, mse, DEGENERATE)
        th = -(g0 - ((v1 * g1) + (v2 * g2))) / dth
        w1 = g1 + (H01 * th)
        w2 = g2 + (H02 * th)
        tix = -((H22 * w1) - (H12 * w2)) / det
        tiy = -((H11 * w2) - (H12 * w1)) / det
        u = 0.5 * th
        q = 1.0 + (u * u)
        c = (1.0 - (u * u)) / q
        s = th / q
        R = [[(c * R[0][0]) - (s * R[1][0]), (c * R[0][1]) - (s * R[1][1])],
             [(s * R[0][0]) + (c * R[1][0]), (s * R[0][1]) + (c * R[1][1])]]
        t = [((c * t[0]) - (s * t[1])) + tix, ((s * t[0]) + (c * t[1])) + tiy]
        crit = None
        if k >= max_iter:
            crit = ITERATIONS
        elif c >= 1.0 - transform_eps and ((tix * tix) + (tiy * tiy)) <= transform_eps:
            crit = TRANSFORM
        else:
            dm = abs(mse - prev)
            if dm < 1e-12:
                crit = ABS_MSE
            elif dm / prev < fitness_eps:
                crit = REL_MSE
        if crit is not None:
            return Result(True, (math.atan2(R[1][0], R[0][0]), t[0], t[1]), k, n, mse, crit)
        prev = mse


class Wrapper:
    """pclICPWrapper's bookkeeping (icp_restatement.Wrapper) with a metric that tbnav_icp_set_metric may change between
    steps: the stored scan survives the change."""

    def __init__(self, laser: Laser, Trs=(0.0, 0.0, 0.0), metric="line", window=NORMAL_WINDOW, max_gap=NORMAL_MAX_GAP, **kw):
        self.laser, self.Trs, self.kw = laser, Trs, kw
        self.metric, self.window, self.max_gap = metric, window, max_gap
        self.stored = None

    def step(self, scan, T_init) -> Result:
        import icp_restatement as point
        scan = np.asarray(scan, dtype=np.float32)
        if self.stored is None:
            self.stored = scan.copy()
            return Result(True, (0.0, 0.0, 0.0), 0, 0, 0.0, NOT_RUN)
        if self.metric == "line":
            res = match(self.stored, scan, self.laser, T_init, self.Trs, window=self.window, max_gap=self.max_gap, **self.kw)
        else:
            res = point.match(self.stored, scan, self.laser, T_init, self.Trs, **self.kw)
        if res.ok:
            self.stored = scan.copy()
        return res
