"""numpy restatement of the device ICP's contract (include/tbnav_icp.h), written from the reference's
bmapping/src/bmapping/cloud_alignment.cpp (createPointCloud :76-157, pclICP :160-223, pclICPWrapper :37-72) and PCL 1.8's
IterativeClosestPoint / DefaultConvergenceCriteria as the header restates them.  Parity with PCL itself is unpinned.

Every floating-point step is spelled with its rounding: float32 where the contract says float, Python floats (IEEE
doubles, no contraction) where it says fp64, glibc's cosf / sinf through ctypes for the beam angles (numpy's float32 trig is
not glibc's), and the fixed summation order of the header with B threads as a parameter.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

_libm = C.CDLL("libm.so.6")
_libm.cosf.restype = C.c_float
_libm.cosf.argtypes = [C.c_float]
_libm.sinf.restype = C.c_float
_libm.sinf.argtypes = [C.c_float]

F32 = np.float32
DBL_MAX = float(np.finfo(np.float64).max)

# tbnav_icp_criterion
NOT_RUN, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES, DEGENERATE = range(7)


def converged(criterion: int) -> bool:
    return ITERATIONS <= criterion <= REL_MSE


@dataclass
class Laser:
    beam_min: float
    beam_max: float
    beam_delta: float
    range_min: float
    range_max: float


def lds01(beam_delta_deg=1.0) -> Laser:
    """The shipped LDS-01 laser as LaserProperties holds it (floats of the degrees converted in double)."""
    d2r = math.pi / 180.0
    return Laser(float(F32(0.0)), float(F32(360.0 * d2r)), float(F32(beam_delta_deg * d2r)), float(F32(0.12)), float(F32(3.5)))


def beam_table(laser: Laser, n_beams: int):
    """(cosf, sinf) of createPointCloud's float beam angle per beam index, with its wrap (:120-154)."""
    bmin, bmax, bd = F32(laser.beam_min), F32(laser.beam_max), F32(laser.beam_delta)
    ang = bmin
    cs = np.empty((n_beams, 2), dtype=np.float32)
    for i in range(n_beams):
        cs[i, 0] = _libm.cosf(float(ang))
        cs[i, 1] = _libm.sinf(float(ang))
        ang = F32(ang + bd)
        if float(bmax) < 0.0 and ang <= bmax:
            ang = bmin
        elif float(bmax) >= 0.0 and ang >= bmax:
            ang = bmin
    return cs


def cloud(scan, laser: Laser, Trs=(0.0, 0.0, 0.0)):
    """createPointCloud: (points float32 [m][2] in beam order, beam index of each point)."""
    scan = np.asarray(scan, dtype=np.float32)
    cs = beam_table(laser, scan.size)
    tc, ts, tx, ty = math.cos(Trs[0]), math.sin(Trs[0]), float(Trs[1]), float(Trs[2])
    rmin, rmax = F32(laser.range_min), F32(laser.range_max)
    pts, idx = [], []
    for i, r in enumerate(scan):
        if r >= rmin and r < rmax:
            px = float(r) * float(cs[i, 0])
            py = float(r) * float(cs[i, 1])
            pts.append((F32((tc * px - ts * py) + tx), F32((ts * px + tc * py) + ty)))   # Transform2D::operator()
            idx.append(i)
    return np.array(pts, dtype=np.float32).reshape(-1, 2), np.array(idx, dtype=np.int64)


@dataclass
class Result:
    ok: bool
    T: tuple              # (theta, x, y); (0, 0, 0) on a failure
    iterations: int
    correspondences: int
    mse: float
    criterion: int


def _tree_sum(partial: np.ndarray) -> float:
    p = partial.copy()
    s = p.size // 2
    while s >= 1:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return float(p[0])


def match(target_scan, source_scan, laser: Laser, T_init, Trs=(0.0, 0.0, 0.0), max_iter=100, max_corr_dist=0.5,
          transform_eps=1e-8, fitness_eps=1e-6, B=256) -> Result:
    """pclICP on the clouds of two scans from T_init = (theta, x, y)."""
    tgt, _ = cloud(target_scan, laser, Trs)
    src, src_beam = cloud(source_scan, laser, Trs)
    return match_clouds(tgt, src, src_beam, np.asarray(source_scan).size, T_init, max_iter, max_corr_dist, transform_eps,
                        fitness_eps, B)


def match_clouds(tgt, src, src_beam, n_beams, T_init, max_iter=100, max_corr_dist=0.5, transform_eps=1e-8, fitness_eps=1e-6,
                 B=256) -> Result:
    """The iteration on explicit clouds: tgt float32 [m][2] in beam order, src float32 [n][2] with its beam indices."""
    tgt = np.asarray(tgt, dtype=np.float32).reshape(-1, 2)
    src = np.asarray(src, dtype=np.float32).reshape(-1, 2)
    src_beam = np.asarray(src_beam, dtype=np.int64)
    # initial guess (:171-183): float cos / sin / x / y, fp64 from then on
    c0, s0 = float(F32(math.cos(T_init[0]))), float(F32(math.sin(T_init[0])))
    R = [[c0, -s0], [s0, c0]]
    t = [float(F32(T_init[1])), float(F32(T_init[2]))]
    max2 = max_corr_dist * max_corr_dist
    prev = DBL_MAX
    sx, sy = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64)
    thread = src_beam % B          # thread of each source point; its points in increasing beam = increasing point index
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
            keep = dmin.astype(np.float64) <= max2
        else:
            keep = np.zeros(src.shape[0], dtype=bool)
            j = np.zeros(src.shape[0], dtype=np.int64)
            dmin = np.zeros(src.shape[0], dtype=np.float32)
        n = int(keep.sum())
        if n < 3:
            return Result(False, (0.0, 0.0, 0.0), k, n, 0.0, NO_CORRESPONDENCES)
        a64x, a64y = ax.astype(np.float64), ay.astype(np.float64)
        b64x, b64y = tgt[j, 0].astype(np.float64), tgt[j, 1].astype(np.float64)
        vals = [a64x, a64y, b64x, b64y, a64x * b64x, a64y * b64y, a64x * b64y, a64y * b64x, dmin.astype(np.float64)]
        tot = []
        for v in vals:
            partial = np.zeros(B)
            rnd = src_beam // B
            for q in range(rounds):   # each thread adds its q-th beam (if kept) in increasing beam order
                sel = keep & (rnd == q)
                partial[thread[sel]] = partial[thread[sel]] + v[sel]
            tot.append(_tree_sum(partial))
        Sax, Say, Sbx, Sby, Sxx, Syy, Sxy, Syx, Sd = tot
        dn = float(n)
        A = (Sxx + Syy) - ((Sax * Sbx) + (Say * Sby)) / dn
        S = (Sxy - Syx) - ((Sax * Sby) - (Say * Sbx)) / dn
        r = math.sqrt((A * A) + (S * S))
        mse = Sd / dn
        if r == 0.0:
            return Result(False, (0.0, 0.0, 0.0), k, n, mse, DEGENERATE)
        c, s = A / r, S / r
        amx, amy, bmx, bmy = Sax / dn, Say / dn, Sbx / dn, Sby / dn
        tix = bmx - ((c * amx) - (s * amy))
        tiy = bmy - ((s * amx) + (c * amy))
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
    """pclICPWrapper's bookkeeping (:37-72): the first call stores the scan and returns (True, identity); a converged match
    replaces the stored scan, a failed one keeps it."""

    def __init__(self, laser: Laser, Trs=(0.0, 0.0, 0.0), **kw):
        self.laser, self.Trs, self.kw = laser, Trs, kw
        self.stored = None

    def step(self, scan, T_init) -> Result:
        scan = np.asarray(scan, dtype=np.float32)
        if self.stored is None:
            self.stored = scan.copy()
            return Result(True, (0.0, 0.0, 0.0), 0, 0, 0.0, NOT_RUN)
        res = match(self.stored, scan, self.laser, T_init, self.Trs, **self.kw)
        if res.ok:
            self.stored = scan.copy()
        return res


def normalize_angle_PI(rad: float) -> float:
    """rigid2d::normalize_angle_PI (rigid2d.hpp)."""
    PI = 3.14159265358979323846
    turns = math.floor((rad + PI) / (2.0 * PI))
    rad = (rad + PI) - turns * 2.0 * PI
    if rad < 0:
        rad += 2.0 * PI
    return rad - PI


def init_guess(cur, prev):
    """icpInitGuess (particle_filter.cpp:602-612): world-frame dx, dy and the wrapped heading change; poses (theta, x, y)."""
    dth = normalize_angle_PI(normalize_angle_PI(cur[0]) - normalize_angle_PI(prev[0]))
    return (dth, cur[1] - prev[1], cur[2] - prev[2])
