"""Cases of the device ICP (include/tbnav_icp.h, csrc/icp.hip) shared by the CPU tests (test_icp_cases.py: the restatements
alone show that every case does what it is there for) and the GPU tests (test_icp_shapes_gpu.py: the kernel against the
restatements bit for bit), so that what is proven on the CPU is what runs on the GPU.

A case is (name, params kwargs, target scan, source scan, T_init).  The kwargs go to rtn_amd.icp.default_params(**kw) on the
GPU side and through laser(kw) / ref_kw(kw) to icp_restatement.match / icp_line_restatement.match on the CPU side.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import icp_line_restatement as LR
import icp_restatement as R
import oracle_api as orc
import rbpf_cases as rc

Case = namedtuple("Case", "name kw tgt src T")

B = 256                                   # kThreads
POINT_P = (1, 2, 3, 4, 6, 8, 12, 16)      # icp_align<PointMetric, P>: source beams per thread (run_pairs)
LINE_P = (1, 2, 3, 4, 6, 8)               # icp_align<LineMetric, P>
MAX_BEAMS = 4096                          # TBNAV_ICP_MAX_BEAMS
MAX_ITER = 1000                           # TBNAV_ICP_MAX_ITER
F32 = np.float32
NAN = F32(np.nan)
D2R = math.pi / 180.0

BEAM_COUNTS = (1, 2, 3, 4, 5, 255, 256, 257, 361, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1535, 1537, 2047, 2048, 2049,
               3071, 3073, 4095, 4096)


def beams_per_thread(n_beams: int, metric="point") -> int:
    """The instantiation run_pairs launches for n_beams: the smallest P of the metric's list with ceil(n / 256) <= P."""
    per = -(-n_beams // B)
    for P in (LINE_P if metric == "line" else POINT_P):
        if per <= P:
            return P
    raise ValueError((n_beams, metric))


def chains(P: int) -> int:
    """C of icp_align<Metric, P, C>: independent chains of the nearest-neighbour scan (target m is in chain m mod C)."""
    return 4 if P <= 2 else 2 if P <= 4 else 1


_LASER = ("beam_min", "beam_max", "beam_delta", "range_min", "range_max")
_ICP = ("Trs", "max_iter", "max_corr_dist", "transform_eps", "fitness_eps")


def laser(kw) -> R.Laser:
    """The laser rtn_amd.icp.default_params(**kw) describes: the LDS-01 with kw's overrides, every field narrowed to float."""
    v = dict(beam_min=0.0, beam_max=360.0 * D2R, beam_delta=kw.get("beam_delta_deg", 1.0) * D2R, range_min=0.12, range_max=3.5)
    v.update({k: kw[k] for k in _LASER if k in kw})
    return R.Laser(*[float(F32(v[k])) for k in _LASER])


def ref_kw(kw) -> dict:
    return {k: kw[k] for k in _ICP if k in kw}


def ref_guess(T):
    """T_init as the restatements take it.  C's cos / sin of +-inf are NaN (what make_pair computes); Python's math.cos raises
    instead, so an infinite angle is handed over as the NaN it becomes."""
    T = tuple(float(v) for v in T)
    return (math.nan if math.isinf(T[0]) else T[0],) + T[1:]


def restate(case: Case, metric="point", **line_kw) -> R.Result:
    """The restatement's answer for one case (float overflow to inf in a guess is the contract's, not an error)."""
    mod = LR if metric == "line" else R
    with np.errstate(all="ignore"):
        return mod.match(case.tgt, case.src, laser(case.kw), ref_guess(case.T), **ref_kw(case.kw), **line_kw)


def room_pair(n, bd_deg, seed, walls=rc.ROOM_BENCH, pose0=(0.0, 0.0, 0.0), pose1=(0.02, 0.04, 0.01), heading0=0.0):
    """Two noisy scans of one room from two poses (theta, x, y); heading0: the angle of beam 0 in the robot frame."""
    rng = np.random.default_rng(seed)
    a = orc.room_scan((pose0[0] + heading0,) + tuple(pose0[1:]), n_beams=n, beam_delta_deg=bd_deg, walls=walls, rng=rng)
    b = orc.room_scan((pose1[0] + heading0,) + tuple(pose1[1:]), n_beams=n, beam_delta_deg=bd_deg, walls=walls, rng=rng)
    return a, b


def beam_count_cases():
    """A room pair at every beam count that is the lower edge, the upper edge or one past the edge of an instantiation."""
    out = []
    for n in BEAM_COUNTS:
        bd = 360.0 / max(n, 4)
        a, b = room_pair(n, bd, 100 + n)
        out.append(Case(f"n{n}", dict(beam_delta_deg=bd), a, b, (0.015, 0.035, 0.015)))
    return out


def wrap_period(L: R.Laser, n_beams: int) -> int:
    """W: the first beam that has beam 0's angle again (createPointCloud's wrap); 0 when none of n_beams does."""
    cs = R.beam_table(L, n_beams).view(np.uint32)
    for w in range(1, n_beams):
        if np.array_equal(cs[w], cs[0]):
            assert np.array_equal(cs[w:], cs[:n_beams - w])
            return w
    return 0


TIE_SHAPES = (("tie_w135_n405", 405, 8.0 / 3.0, 135), ("tie_w361_n767", 767, 1.0, 361), ("tie_w361_n1023", 1023, 1.0, 361),
              ("tie_w361_n1083", 1083, 1.0, 361))   # the last is the control: P = 6 scans as one chain


def tie_cases(seed=0):
    """Exact float32 ties between distinct target points of different chains.  The beam angle wraps with period W, so beams i and
    i + W lie on one ray; the target holds range ra on the first turn and ra + g on the second, the source ra + g / 2 on the
    first turn: wherever the float32 rounding lets it, the source point is at the same squared distance from both."""
    out = []
    for name, n, bd, W in TIE_SHAPES:
        kw = dict(beam_delta_deg=bd)
        assert wrap_period(laser(kw), n) == W, (name, wrap_period(laser(kw), n))
        tgt, src = tie_scans(n, W, seed)
        out.append(Case(name, kw, tgt, src, (0.0, 0.0, 0.0)))
    return out


def tie_scans(n, W, seed=0):
    """(target, source) of tie_cases for a laser whose angle wraps every W beams; the beams past the turns used are invalid."""
    rng = np.random.default_rng(seed)
    ra = 1.0 + rng.integers(0, 32, W) / 16.0
    g = rng.integers(1, 4, W) / 8.0
    tgt = np.full(n, NAN, dtype=np.float32)
    src = np.full(n, NAN, dtype=np.float32)
    tgt[:W] = ra
    tgt[W:2 * W] = ra + g
    src[:W] = ra + g / 2.0
    return tgt, src


def count_ties(case, C):
    """In the first iteration's float32 distance matrix (identity guess): (source points whose minimum is attained by two
    targets of different coordinates in different chains, those of them whose lowest index is not in the lowest chain)."""
    L = laser(case.kw)
    Trs = tuple(case.kw.get("Trs", (0.0, 0.0, 0.0)))
    tgt, tgt_beam = R.cloud(case.tgt, L, Trs)
    src, _ = R.cloud(case.src, L, Trs)
    assert tuple(case.T) == (0.0, 0.0, 0.0)          # a = src exactly
    dx = src[:, None, 0] - tgt[None, :, 0]
    dy = src[:, None, 1] - tgt[None, :, 1]
    d = dx * dx + dy * dy
    assert d.dtype == np.float32
    tied = wrong_chain = 0
    for i in range(d.shape[0]):
        at = np.flatnonzero(d[i] == d[i].min())
        if at.size < 2:
            continue
        first = at[0]
        others = [m for m in at[1:] if tuple(tgt[m]) != tuple(tgt[first]) and (C == 1 or tgt_beam[m] % C != tgt_beam[first] % C)]
        if not others:
            continue
        tied += 1
        if any(tgt_beam[m] % C < tgt_beam[first] % C for m in others):
            wrong_chain += 1
    return tied, wrong_chain


def bench_run(n=6, seed=11):
    """The bench room's trajectory as test_icp_gpu.py runs it: (poses, scans)."""
    steps, poses = rc.trajectory(n, inc=rc.TRAJ_BENCH)
    rng = np.random.default_rng(seed)
    return poses, np.stack([orc.room_scan(p, walls=rc.ROOM_BENCH, rng=rng) for p in poses])


CORRIDOR = (-50, 50, -1, 1)


def criterion_cases():
    """Parameter sets that take every exit of the iteration on the bench-room trajectory, and the two DEGENERATE exits."""
    poses, scans = bench_run()
    out = []
    for s in range(1, 6):
        g = R.init_guess(poses[s], poses[s - 1])
        out.append(Case(f"rel_mse_s{s}", dict(transform_eps=0.0), scans[s - 1], scans[s], g))
        out.append(Case(f"abs_mse_or_cycle_s{s}", dict(transform_eps=0.0, fitness_eps=0.0), scans[s - 1], scans[s], g))
        out.append(Case(f"max_iter_{MAX_ITER}_s{s}", dict(transform_eps=0.0, fitness_eps=0.0, max_iter=MAX_ITER), scans[s - 1], scans[s], g))
    out.append(Case("default_s1", dict(), scans[0], scans[1], R.init_guess(poses[1], poses[0])))
    out.append(Case("identical", dict(), scans[2], scans[2].copy(), (0.0, 0.0, 0.0)))
    out.append(Case("max_iter_2", dict(max_iter=2), scans[0], scans[1], (0.0, 0.0, 0.0)))
    empty = np.full(360, NAN, dtype=np.float32)
    out.append(Case("empty_source", dict(), scans[0], empty, (0.0, 0.0, 0.0)))
    # the point metric's r == 0: every source point pairs with the one target point, so both cross-covariance terms vanish
    tgt, src = empty.copy(), empty.copy()
    tgt[0] = 1.0
    src[[0, 1, 358, 359]] = [1.1, 0.9, 1.2, 1.05]
    out.append(Case("degenerate_one_target_point", dict(), tgt, src, (0.0, 0.0, 0.0)))
    # the line metric's: a noise-free corridor leaves only the normals' float rounding across it
    c0 = orc.room_scan((0.0, 0.0, 0.0), walls=CORRIDOR)
    c1 = orc.room_scan((0.0, 0.05, 0.0), walls=CORRIDOR)
    out.append(Case("corridor_without_noise", dict(), c0, c1, (0.0, 0.05, 0.0)))
    return out


def _mask(n, frac, bunched, rng):
    if bunched:   # the strides t, t + 256, ... of a few neighbouring threads
        return ((np.arange(n) - 5) % B) < max(1, round(frac * B))
    m = np.zeros(n, dtype=bool)
    m[rng.choice(n, max(1, round(frac * n)), replace=False)] = True
    return m


T_SPECIALS = (("nan", math.nan), ("pinf", math.inf), ("ninf", -math.inf), ("1e30", 1e30), ("1e39", 1e39))


def edge_cases():
    out = []
    # sparse scans: most beams invalid, in both scans
    for n in (360, MAX_BEAMS):
        bd = 360.0 / n
        a, b = room_pair(n, bd, 200 + n)
        for frac in (0.01, 0.05, 0.5):
            for bunched in (False, True):
                m = _mask(n, frac, bunched, np.random.default_rng(int(frac * 100) + n))
                out.append(Case(f"sparse_n{n}_{int(frac * 100)}pct_{'bunched' if bunched else 'spread'}", dict(beam_delta_deg=bd),
                                np.where(m, a, NAN), np.where(m, b, NAN), (0.015, 0.035, 0.015)))
    a, b = room_pair(360, 1.0, 7)
    # exactly 2 and exactly 3 correspondences (n < 3)
    for beams in ((10, 130), (10, 130, 250)):
        src = np.full(360, NAN, dtype=np.float32)
        src[list(beams)] = b[list(beams)]
        out.append(Case(f"corr_{len(beams)}", dict(), a, src, (0.015, 0.035, 0.015)))
    # a pair at exactly max_corr_dist: kept ('<='); one ulp further: dropped.  Two exact pairs beside it.
    tgt = np.full(360, NAN, dtype=np.float32)
    tgt[[0, 90, 180]] = 1.0
    for name, r0 in (("at", F32(1.5)), ("above", np.nextafter(F32(1.5), F32(2.0)))):
        src = tgt.copy()
        src[0] = r0
        out.append(Case(f"max_corr_dist_{name}_one_iteration", dict(max_iter=1), tgt, src, (0.0, 0.0, 0.0)))
        out.append(Case(f"max_corr_dist_{name}", dict(), tgt, src, (0.0, 0.0, 0.0)))
    # initial guesses that are not numbers, or not small ones
    for slot in range(3):
        for name, v in T_SPECIALS:
            T = [0.015, 0.035, 0.015]
            T[slot] = v
            out.append(Case(f"guess_{'txy'[slot]}_{name}", dict(), a, b, tuple(T)))
    # range_min is in ('>='), range_max is out ('<')
    lo, hi = F32(0.12), F32(3.5)
    edge = [lo, np.nextafter(lo, F32(0.0)), hi, np.nextafter(hi, F32(0.0))]
    ta, tb = a.copy(), b.copy()
    ta[[3, 50, 120, 200]] = edge
    tb[[3, 60, 121, 201]] = edge
    out.append(Case("range_bounds", dict(), ta, tb, (0.015, 0.035, 0.015)))
    # a laser that turns the other way (beam_delta < 0, beam_max < 0: the other wrap branch), past its wrap
    kw = dict(beam_min=0.0, beam_max=-360.0 * D2R, beam_delta=-1.0 * D2R)
    na, nb = room_pair(400, -1.0, 8)
    out.append(Case("negative_delta_and_beam_max", kw, na, nb, (0.015, 0.035, 0.015)))
    # a laser that starts behind the robot, mounted off-centre
    kw = dict(beam_min=-180.0 * D2R, beam_max=180.0 * D2R, Trs=(0.3, -0.04, 0.02))
    ma, mb = room_pair(360, 1.0, 9, heading0=-math.pi)
    out.append(Case("beam_min_minus_pi_and_Trs", kw, ma, mb, (0.015, 0.035, 0.015)))
    return out


UNIT_ROOM = (-1.0, 1.0, -1.0, 1.0)


def batch_run(n, n_scans, seed=0):
    """A logged run for tbnav_icp_step_batch with the shipped 1 degree laser at n beams (its angle wraps every 361 beams, so a
    longer scan sees the room several times): ordinary scans of a small room with, between them, the tie pair, all-invalid scans
    (one alone, two in a row), a sparse scan, and the point metric's DEGENERATE (three exact points stored by an identical
    repeat, then four source points that all pair with one of them).  -> (params kwargs, scans [n_scans][n], T_init [n_scans][3])"""
    assert n >= 2 * 361 and n_scans >= 24
    W = 361
    tie_t, tie_s = tie_scans(n, W, seed)
    rng = np.random.default_rng(1000 + n + seed)
    three = np.full(n, NAN, dtype=np.float32)
    three[[0, 90, 180]] = 1.0
    four = np.full(n, NAN, dtype=np.float32)
    four[[0, 1, 358, 359]] = [1.1, 0.9, 1.2, 1.05]
    special = {0: tie_t, 1: tie_s, 5: np.full(n, NAN, dtype=np.float32), 12: three, 13: three.copy(), 14: four,
               20: np.full(n, F32(np.inf), dtype=np.float32), 21: np.full(n, F32(-1.0), dtype=np.float32)}
    inc = np.array([0.004, 0.006, 0.003])
    pose = np.zeros(3)
    scans, T = [], []
    for s in range(n_scans):
        if s in special:
            scans.append(special[s])
            T.append((0.0, 0.0, 0.0))
            continue
        pose = pose + inc
        sc = orc.room_scan(tuple(pose), n_beams=n, walls=UNIT_ROOM, rng=rng)
        if s == 9:     # sparse: one beam in twenty
            sc = np.where(np.arange(n) % 20 == 3, sc, NAN)
        scans.append(sc)
        T.append(tuple(inc))
    return dict(), np.stack(scans).astype(np.float32), np.array(T, dtype=np.float64)


def all_cases():
    return beam_count_cases() + tie_cases() + criterion_cases() + edge_cases()
