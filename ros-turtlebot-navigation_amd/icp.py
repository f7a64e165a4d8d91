"""Python mirror of bmapping::ScanAlignment with the device ICP (include/tbnav_icp.h, csrc/icp.hip).

Same method names and meaning as the reference's class (bmapping/include/bmapping/cloud_alignment.hpp:28-80):
pclICPWrapper(T_init, scan) keeps the previous scan in the handle (cloud_alignment.cpp:37-72), pclICP aligns two scans
statelessly (:160-223).  wrapperBatch replays a logged run: its (ok, T) arrays are tbnav_rbpf_slam_batch's icp_ok / T_icp.
init_guess is ParticleFilter::icpInitGuess (particle_filter.cpp:602-612).  The algorithm is a restatement of PCL's
IterativeClosestPoint; parity with PCL itself is unpinned (see the header).

search=True | dict(...) (an addition with no counterpart in the reference) puts the correlative search of the header's
CORRELATIVE SEARCH section in front of every alignment: it scores every pose of a window round the guess against a table of
the target scan and starts the ICP from the best one, when that one is good enough.  The default is off.

shape=True | dict(...) beside search (an addition too) measures the shape of the search's score volume (the header's items
F1-F6) and keeps the guess along a direction in which the scores are flat, a corridor's axis: the search alone pulls two scans of
a corridor on top of each other.  The default is off.

wide=True | dict(...) beside search (an addition too) adds the wide second stage of the header's items W1-W8: a window of up to
+-64 cells and +-180 steps, scored only when the first stage is rejected (when="reject", the default), or also when its choice
sits on the border of its window ("reject_or_edge"), or always and in its place ("always").  The default is off.

searchMap(filter, T_init, scan) (an addition too) searches against the MAP of a particle of an rbpf.ParticleFilter instead of the
previous scan (the header's MAP SEARCH, M1-M9): for a pose that has drifted over many scans, or a filter restarted in a known map.

localizeMap(filter, scan) (an addition too) takes NO guess: it scores every heading at every cell of the particle's map and prunes
with the exact bound of a max-pooled copy of the likelihood map (the header's GLOBAL SEARCH, L1-L10): where the robot is in a map
the filter already holds.

alignMap(filter, T_init, scan) (an addition too) aligns one scan to the particle's map BELOW one cell (the header's MAP ALIGNMENT,
A1-A11): a point-to-line step against lines fitted to the occupied cells; relocalizeMap(filter, scan) is localizeMap followed by it.

verifyMap(filter, T, scan) (an addition too) asks whether the particle's map CONTRADICTS a pose (the header's MAP CHECK, V1-V10):
every beam is walked through the map, and the beams that pass through a wall the map holds or end in space it knows to be free are
counted against thresholds; relocalizeMapChecked(filter, scan) is localizeMap, alignMap and this check in a row.

metric="line" (an addition with no counterpart in the reference, which only runs PCL's point-to-point ICP) aligns with the
point-to-line metric of the header's POINT-TO-LINE METRIC section; the default stays "point".
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import capi


def default_params(beam_delta_deg=1.0, Trs=(0.0, 0.0, 0.0), device=-1, **kw) -> "capi.IcpParams":
    """The shipped LDS-01 laser (config/LDS_01_lidar.yaml, narrowed to float like LaserProperties) and the reference's ICP
    settings (cloud_alignment.cpp:21-34)."""
    L = capi.lib()
    p = capi.IcpParams()
    L.tbnav_icp_default_params(C.byref(p))
    d2r = math.pi / 180.0
    p.beam_min, p.beam_max, p.beam_delta = 0.0, float(np.float32(360.0 * d2r)), float(np.float32(beam_delta_deg * d2r))
    p.range_min, p.range_max = 0.12, 3.5
    p.Trs[:] = [float(v) for v in Trs]
    p.device = device
    for key, v in kw.items():
        setattr(p, key, v)
    return p


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def _info(i: "capi.IcpInfo") -> dict:
    return dict(iterations=i.iterations, correspondences=i.correspondences, mse=i.mse, criterion=i.criterion)


def converged(criterion: int) -> bool:
    return capi.ICP_ITERATIONS <= criterion <= capi.ICP_REL_MSE


def normalize_angle_PI(rad: float) -> float:
    """rigid2d::normalize_angle_PI (host/include/rigid2d/rigid2d.hpp)."""
    PI = 3.14159265358979323846
    turns = math.floor((rad + PI) / (2.0 * PI))
    rad = (rad + PI) - turns * 2.0 * PI
    if rad < 0:
        rad += 2.0 * PI
    return rad - PI


def init_guess(cur, prev):
    """icpInitGuess: (dtheta, dx, dy) of two odometry poses (theta, x, y) — world-frame dx, dy, as the reference writes it."""
    dth = normalize_angle_PI(normalize_angle_PI(float(cur[0])) - normalize_angle_PI(float(prev[0])))
    return (dth, float(cur[1]) - float(prev[1]), float(cur[2]) - float(prev[2]))


_METRICS = {"point": capi.ICP_METRIC_POINT, "line": capi.ICP_METRIC_LINE}
_SEARCH_FIELDS = tuple(f for f, _ in capi.IcpSearchParams._fields_)


_SHAPE_FIELDS = ("drop_q10", "flat_cells2")
_WIDE_FIELDS = ("lin_cells", "ang_steps", "when")
_WIDE_WHEN = {"reject": capi.ICP_WIDE_ON_REJECT, "reject_or_edge": capi.ICP_WIDE_ON_REJECT_OR_EDGE, "always": capi.ICP_WIDE_ALWAYS}


def _search_shape(r: "capi.IcpSearchShape") -> dict:
    return dict(S0=r.S0, Sx=r.Sx, Sy=r.Sy, Sxx=r.Sxx, Sxy=r.Sxy, Syy=r.Syy, l1=r.l1, l2=r.l2, ex=r.ex, ey=r.ey, T_raw=tuple(r.T_raw),
                cells=r.cells, kind=r.kind, computed=r.computed)


_GLOBAL_FIELDS = ("ang_count", "ang_step", "pool_log2", "region", "min_quality")


def _global_params(kw) -> "capi.IcpGlobalParams":
    p = capi.IcpGlobalParams()
    capi.lib().tbnav_icp_default_global_params(C.byref(p))
    for key, v in kw.items():
        if key not in _GLOBAL_FIELDS:
            raise TypeError(f"localizeMap: no parameter {key!r} (one of {_GLOBAL_FIELDS})")
        if key == "region":
            p.region[:] = [int(x) for x in v]
        else:
            setattr(p, key, v)
    return p


_HYP_FIELDS = ("max_hyp", "floor_q10", "sep_cells", "sep_steps", "wrap", "reserved")


def _hyp_params(kw) -> "capi.IcpHypParams":
    p = capi.IcpHypParams()
    capi.lib().tbnav_icp_default_hyp_params(C.byref(p))
    for key, v in (kw or {}).items():
        if key not in _HYP_FIELDS:
            raise TypeError(f"localizeMapHypotheses: no parameter {key!r} (one of {_HYP_FIELDS})")
        setattr(p, key, int(v))
    return p


def _hyp_info(i: "capi.IcpHypInfo") -> dict:
    return dict(searched=i.searched, n=i.n, n_peaks=i.n_peaks, best_score=i.best_score, floor_score=i.floor_score, points=i.points,
                occupied=i.occupied, blocks=i.blocks, floor_blocks=i.floor_blocks, refined_blocks=i.refined_blocks, candidates=i.candidates,
                rounds=i.rounds)


def _hypothesis(y: "capi.IcpHypothesis") -> dict:
    return dict(T=tuple(y.T), quality=y.quality, score=y.score, ia=y.ia, tx=y.tx, ty=y.ty, accepted=y.accepted)


_ALIGN_MAP_FIELDS = ("half_cells", "gate_cells", "feature_cells", "max_flatness", "reserved")
_ALIGN_MAP_PAIR = np.dtype([(f, np.dtype(t)) for f, t in capi.IcpAlignMapPair._fields_])


def _align_map_params(kw) -> "capi.IcpAlignMapParams":
    p = capi.IcpAlignMapParams()
    capi.lib().tbnav_icp_default_align_map_params(C.byref(p))
    for key, v in kw.items():
        if key not in _ALIGN_MAP_FIELDS:
            raise TypeError(f"alignMap: no parameter {key!r} (one of {_ALIGN_MAP_FIELDS})")
        setattr(p, key, v)
    return p


_VERIFY_MAP_FIELDS = ("half_cells", "slack_cells", "max_through_q10", "max_missing_q10", "min_hit_q10", "reserved")
_VERIFY_MAP_BEAM = np.dtype([("cls", np.int32), ("ei", np.int32), ("ej", np.int32), ("n", np.int32), ("b", np.int32), ("D", np.int32),
                             ("free_cells", np.int32), ("unknown_cells", np.int32)])
assert _VERIFY_MAP_BEAM.itemsize == C.sizeof(capi.IcpVerifyMapBeam)


def _verify_map_params(kw) -> "capi.IcpVerifyMapParams":
    p = capi.IcpVerifyMapParams()
    capi.lib().tbnav_icp_default_verify_map_params(C.byref(p))
    for key, v in kw.items():
        if key not in _VERIFY_MAP_FIELDS:
            raise TypeError(f"verifyMap: no parameter {key!r} (one of {_VERIFY_MAP_FIELDS})")
        setattr(p, key, v)
    return p


def _verify_map_info(i: "capi.IcpVerifyMapInfo") -> dict:
    return dict(points=i.points, outside=i.outside, walked=i.walked, hit=i.hit, through=i.through, missing=i.missing, unseen=i.unseen,
                undecided=i.undecided, free_cells=i.free_cells, unknown_cells=i.unknown_cells, sensor_cell=tuple(i.sensor_cell),
                sensor_class=i.sensor_class, accepted=i.accepted)


def _global_info(i: "capi.IcpGlobalInfo") -> dict:
    return dict(T=tuple(i.T), quality=i.quality, blocks=i.blocks, refined_blocks=i.refined_blocks, score=i.score, points=i.points,
                occupied=i.occupied, ia=i.ia, tx=i.tx, ty=i.ty, rounds=i.rounds, accepted=i.accepted, searched=i.searched)


def _search_info(i: "capi.IcpSearchInfo") -> dict:
    return dict(T=tuple(i.T), quality=i.quality, score=i.score, points=i.points, candidates=i.candidates, ia=i.ia, iy=i.iy,
                ix=i.ix, at_edge=i.at_edge, accepted=i.accepted, searched=i.searched)


class ScanAlignment:
    """bmapping::ScanAlignment on one MI355X."""

    def __init__(self, params: "capi.IcpParams | None" = None, metric="point", normal_window=0, normal_max_gap=0.0, search=None, shape=None,
                 wide=None):
        self._L = capi.lib()
        self.params = params if params is not None else default_params()
        if metric not in _METRICS:
            raise ValueError(f"metric must be one of {sorted(_METRICS)}, not {metric!r}")
        self._h = C.c_void_p()
        capi.check(self._L.tbnav_icp_create(C.byref(self.params), C.byref(self._h)), "tbnav_icp_create")
        if metric != "point" or normal_window or normal_max_gap:
            try:
                self.setMetric(metric, normal_window, normal_max_gap)
            except Exception:
                self.close()
                raise
        if search is not None and search is not False:
            try:
                self.setSearch(**({} if search is True else dict(search)))
            except Exception:
                self.close()
                raise
        if shape is not None and shape is not False:
            try:
                self.setSearchShape(**({} if shape is True else dict(shape)))
            except Exception:
                self.close()
                raise

        if wide is not None and wide is not False:
            try:
                self.setSearchWide(**({} if wide is True else dict(wide)))
            except Exception:
                self.close()
                raise

    def setSearchWide(self, *off, **kw):
        """tbnav_icp_set_search_wide: setSearchWide(lin_cells=..., ang_steps=..., when=...) turns the wide second stage on
        wherever a search runs, with the defaults (tbnav_icp_default_search_wide_params) for what is not named; when is
        "reject" | "reject_or_edge" | "always" or the C constant; setSearchWide(None) turns it off.  It is idle while the
        search itself is off.  Its window must contain the search's, so call setSearch first."""
        if off:
            if off != (None,) or kw:
                raise TypeError("setSearchWide(None) turns the wide stage off; parameters go by keyword")
            capi.check(self._L.tbnav_icp_set_search_wide(self._h, None), "tbnav_icp_set_search_wide")
            return
        p = capi.IcpSearchWideParams()
        self._L.tbnav_icp_default_search_wide_params(C.byref(p))
        for key, v in kw.items():
            if key not in _WIDE_FIELDS:
                raise TypeError(f"setSearchWide: no parameter {key!r} (one of {_WIDE_FIELDS})")
            if key == "when" and isinstance(v, str):
                if v not in _WIDE_WHEN:
                    raise ValueError(f"when must be one of {sorted(_WIDE_WHEN)}, not {v!r}")
                v = _WIDE_WHEN[v]
            setattr(p, key, v)
        capi.check(self._L.tbnav_icp_set_search_wide(self._h, C.byref(p)), "tbnav_icp_set_search_wide")

    def searchWideParams(self):
        """-> (on, dict of tbnav_icp_search_wide_params) as the handle holds them (the defaults while the wide stage is off)"""
        on, p = C.c_int32(), capi.IcpSearchWideParams()
        capi.check(self._L.tbnav_icp_get_search_wide(self._h, C.byref(on), C.byref(p)), "tbnav_icp_get_search_wide")
        return bool(on.value), {f: getattr(p, f) for f in _WIDE_FIELDS}

    def lastSearchWide(self) -> dict:
        """beside lastSearch()'s outcome: the first stage's record and whether the wide stage ran -> dict(first=..., ran=...)"""
        r = capi.IcpSearchWideInfo()
        capi.check(self._L.tbnav_icp_last_search_wide(self._h, C.byref(r)), "tbnav_icp_last_search_wide")
        return dict(first=_search_info(r.first), ran=r.ran)

    def searchWideScores(self, T_init, target_scan, source_scan, scores=True):
        """test hook, stateless: the wide stage alone, whatever `when` says -> (accepted, T, info dict,
        uint32 [2A+1][2W+1][2W+1], or None with scores=False)"""
        tgt = np.ascontiguousarray(target_scan, dtype=np.float32)
        src = np.ascontiguousarray(source_scan, dtype=np.float32)
        if tgt.size != src.size:
            raise ValueError("target and source scans must have the same number of beams")
        p = self.searchWideParams()[1]
        na, nl = 2 * p["ang_steps"] + 1, 2 * p["lin_cells"] + 1
        vol = np.zeros((na, nl, nl), dtype=np.uint32) if scores else None
        out = (C.c_double * 3)()
        info = capi.IcpSearchInfo()
        capi.check(self._L.tbnav_icp_search_wide_scores(self._h, tgt.ctypes.data, src.ctypes.data, src.size, _d3(T_init), out,
                                                        C.byref(info), vol.ctypes.data if scores else None),
                   "tbnav_icp_search_wide_scores")
        return bool(info.accepted), tuple(out), _search_info(info), vol

    def setSearchShape(self, *off, **kw):
        """tbnav_icp_set_search_shape: setSearchShape(drop_q10=..., flat_cells2=...) turns the shape of the score volume on
        wherever a search runs, with the defaults (tbnav_icp_default_search_shape_params) for what is not named;
        setSearchShape(None) turns it off.  It is idle while the search itself is off."""
        if off:
            if off != (None,) or kw:
                raise TypeError("setSearchShape(None) turns the shape off; parameters go by keyword")
            capi.check(self._L.tbnav_icp_set_search_shape(self._h, None), "tbnav_icp_set_search_shape")
            return
        p = capi.IcpSearchShapeParams()
        self._L.tbnav_icp_default_search_shape_params(C.byref(p))
        for key, v in kw.items():
            if key not in _SHAPE_FIELDS:
                raise TypeError(f"setSearchShape: no parameter {key!r} (one of {_SHAPE_FIELDS})")
            setattr(p, key, v)
        capi.check(self._L.tbnav_icp_set_search_shape(self._h, C.byref(p)), "tbnav_icp_set_search_shape")

    def searchShapeParams(self):
        """-> (on, dict of tbnav_icp_search_shape_params) as the handle holds them (the defaults while the shape is off)"""
        on, p = C.c_int32(), capi.IcpSearchShapeParams()
        capi.check(self._L.tbnav_icp_get_search_shape(self._h, C.byref(on), C.byref(p)), "tbnav_icp_get_search_shape")
        return bool(on.value), {f: getattr(p, f) for f in _SHAPE_FIELDS}

    def lastSearchShape(self) -> dict:
        """the shape record beside lastSearch()'s (computed = 0: none was formed)"""
        r = capi.IcpSearchShape()
        capi.check(self._L.tbnav_icp_last_search_shape(self._h, C.byref(r)), "tbnav_icp_last_search_shape")
        return _search_shape(r)

    def searchWithShape(self, T_init, target_scan, source_scan):
        """test hook, stateless: search() with the shape applied whether or not the handle has it on
        -> (accepted, T, info dict, shape dict)"""
        tgt = np.ascontiguousarray(target_scan, dtype=np.float32)
        src = np.ascontiguousarray(source_scan, dtype=np.float32)
        if tgt.size != src.size:
            raise ValueError("target and source scans must have the same number of beams")
        out = (C.c_double * 3)()
        info, rec = capi.IcpSearchInfo(), capi.IcpSearchShape()
        capi.check(self._L.tbnav_icp_search_with_shape(self._h, tgt.ctypes.data, src.ctypes.data, src.size, _d3(T_init), out,
                                                       C.byref(info), C.byref(rec)), "tbnav_icp_search_with_shape")
        return bool(info.accepted), tuple(out), _search_info(info), _search_shape(rec)

    def setSearch(self, *off, **kw):
        """tbnav_icp_set_search: setSearch(resolution=..., lin_cells=..., ...) turns the correlative search on for every later
        call, with the defaults (tbnav_icp_default_search_params) for what is not named; setSearch(None) turns it off."""
        if off:
            if off != (None,) or kw:
                raise TypeError("setSearch(None) turns the search off; parameters go by keyword")
            capi.check(self._L.tbnav_icp_set_search(self._h, None), "tbnav_icp_set_search")
            return
        p = capi.IcpSearchParams()
        self._L.tbnav_icp_default_search_params(C.byref(p))
        for key, v in kw.items():
            if key not in _SEARCH_FIELDS:
                raise TypeError(f"setSearch: no parameter {key!r} (one of {_SEARCH_FIELDS})")
            setattr(p, key, v)
        capi.check(self._L.tbnav_icp_set_search(self._h, C.byref(p)), "tbnav_icp_set_search")

    def searchParams(self):
        """-> (on, dict of tbnav_icp_search_params) as the handle holds them (the defaults while the search is off)"""
        on, p = C.c_int32(), capi.IcpSearchParams()
        capi.check(self._L.tbnav_icp_get_search(self._h, C.byref(on), C.byref(p)), "tbnav_icp_get_search")
        return bool(on.value), {f: getattr(p, f) for f in _SEARCH_FIELDS}

    def _search(self, T_init, target_scan, source_scan, scores):
        tgt = np.ascontiguousarray(target_scan, dtype=np.float32)
        src = np.ascontiguousarray(source_scan, dtype=np.float32)
        if tgt.size != src.size:
            raise ValueError("target and source scans must have the same number of beams")
        out = (C.c_double * 3)()
        info = capi.IcpSearchInfo()
        if scores is None:
            capi.check(self._L.tbnav_icp_search(self._h, tgt.ctypes.data, src.ctypes.data, src.size, _d3(T_init), out, C.byref(info)),
                       "tbnav_icp_search")
        else:
            capi.check(self._L.tbnav_icp_search_scores(self._h, tgt.ctypes.data, src.ctypes.data, src.size, _d3(T_init), out,
                                                       C.byref(info), scores.ctypes.data), "tbnav_icp_search_scores")
        return bool(info.accepted), tuple(out), _search_info(info)

    def search(self, T_init, target_scan, source_scan):
        """tbnav_icp_search, stateless: the search alone with the handle's parameters (the defaults while it is off)
        -> (accepted, T, info dict)"""
        return self._search(T_init, target_scan, source_scan, None)

    def searchScores(self, T_init, target_scan, source_scan):
        """test hook: the same and the whole score volume -> (accepted, T, info dict, uint32 [na][nl][nl])"""
        p = self.searchParams()[1]
        na, nl = 2 * p["ang_steps"] + 1, 2 * p["lin_cells"] + 1
        scores = np.zeros((na, nl, nl), dtype=np.uint32)
        return self._search(T_init, target_scan, source_scan, scores) + (scores,)

    def searchTable(self, scan):
        """test hook: the likelihood table of one scan taken as a target: uint8 [n][n], indexed [iy][ix]"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        p = self.searchParams()[1]
        n = 2 * math.ceil(p["half_extent"] / p["resolution"])
        tab = np.zeros((n, n), dtype=np.uint8)
        capi.check(self._L.tbnav_icp_search_table(self._h, scan.ctypes.data, scan.size, tab.ctypes.data), "tbnav_icp_search_table")
        return tab

    def searchMap(self, filter, T_init, scan, particle=capi.ICP_MAP_BEST_PARTICLE):
        """tbnav_icp_search_map (the header's MAP SEARCH, M1-M9): the search of one scan against the map of a particle of `filter`
        (rbpf.ParticleFilter; particle=-1: its best one, found on the device) from the WORLD guess T_init = (theta, x, y), with the
        handle's search parameters -> (accepted, T in the world, info dict).  The map never leaves the device."""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        info = capi.IcpSearchInfo()
        capi.check(self._L.tbnav_icp_search_map(self._h, filter._h, int(particle), scan.ctypes.data, scan.size, _d3(T_init), C.byref(info)),
                   "tbnav_icp_search_map")
        return bool(info.accepted), tuple(info.T), _search_info(info)

    def searchMapBatch(self, filter, T_init, scan, particles):
        """tbnav_icp_search_map_batch (M7): one scan, n pairs (particles[i], T_init[i]), each equal to the single call
        -> list of (accepted, T, info dict)"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        particles = np.ascontiguousarray(particles, dtype=np.int32).reshape(-1)
        n = particles.size
        T_init = np.ascontiguousarray(T_init, dtype=np.float64).reshape(n, 3)
        infos = (capi.IcpSearchInfo * max(n, 1))()
        capi.check(self._L.tbnav_icp_search_map_batch(self._h, filter._h, scan.ctypes.data, scan.size, n, particles.ctypes.data,
                                                      T_init.ctypes.data, C.cast(infos, C.c_void_p)), "tbnav_icp_search_map_batch")
        return [(bool(i.accepted), tuple(i.T), _search_info(i)) for i in infos[:n]]

    def searchMapTable(self, filter, T_init, particle=capi.ICP_MAP_BEST_PARTICLE):
        """test hook: the table (M4) of one pair and tgt_points -> (uint8 [n][n] indexed [iy][ix], int)"""
        p = self.searchParams()[1]
        n = 2 * math.ceil(p["half_extent"] / p["resolution"])
        tab = np.zeros((n, n), dtype=np.uint8)
        cnt = C.c_uint32()
        capi.check(self._L.tbnav_icp_search_map_table(self._h, filter._h, int(particle), _d3(T_init), tab.ctypes.data, C.byref(cnt)),
                   "tbnav_icp_search_map_table")
        return tab, int(cnt.value)

    def searchMapScores(self, filter, T_init, scan, particle=capi.ICP_MAP_BEST_PARTICLE, wide=False):
        """test hook: searchMap and the whole score volume -> (accepted, T, info dict, uint32 [na][nl][nl]); wide=True: the wide
        stage alone (as searchWideScores), its volume [2A+1][2W+1][2W+1]"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        p = self.searchWideParams()[1] if wide else self.searchParams()[1]
        na, nl = 2 * p["ang_steps"] + 1, 2 * p["lin_cells"] + 1
        vol = np.zeros((na, nl, nl), dtype=np.uint32)
        info = capi.IcpSearchInfo()
        fn = self._L.tbnav_icp_search_map_wide_scores if wide else self._L.tbnav_icp_search_map_scores
        capi.check(fn(self._h, filter._h, int(particle), scan.ctypes.data, scan.size, _d3(T_init), C.byref(info), vol.ctypes.data),
                   "tbnav_icp_search_map_wide_scores" if wide else "tbnav_icp_search_map_scores")
        return bool(info.accepted), tuple(info.T), _search_info(info), vol

    def lastMapKernel(self) -> str:
        """the map search's table kernel as a profiler prints it; "" until searchMap has run on this handle"""
        buf = C.create_string_buffer(64)
        capi.check(self._L.tbnav_icp_last_map_kernel(self._h, buf, 64), "tbnav_icp_last_map_kernel")
        return buf.value.decode()

    def localizeMap(self, filter, scan, particle=capi.ICP_MAP_BEST_PARTICLE, **params):
        """tbnav_icp_localize_map (the header's GLOBAL SEARCH, L1-L10): the pose of one scan in the map of a particle of `filter`
        (particle=-1: its best one), with no guess; params: ang_count, ang_step, pool_log2, region=(tx0, ty0, tx1, ty1), min_quality
        (tbnav_icp_default_global_params for what is not named) -> (accepted, T in the world, info dict)"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        info = capi.IcpGlobalInfo()
        capi.check(self._L.tbnav_icp_localize_map(self._h, filter._h, int(particle), scan.ctypes.data, scan.size,
                                                  C.byref(_global_params(params)), C.byref(info)), "tbnav_icp_localize_map")
        return bool(info.accepted), tuple(info.T), _global_info(info)

    GLOBAL_STAGES = ("field", "pool", "offsets", "bound", "hist", "list_1", "refine_1", "list_2", "refine_2")

    def localizeMapTimed(self, filter, scan, particle=capi.ICP_MAP_BEST_PARTICLE, **params):
        """tbnav_icp_localize_map_timed: localizeMap with its stages timed by events -> (accepted, T, info dict, {stage: ms})"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        info = capi.IcpGlobalInfo()
        ms = np.zeros(capi.ICP_GLOBAL_STAGES, dtype=np.float32)
        capi.check(self._L.tbnav_icp_localize_map_timed(self._h, filter._h, int(particle), scan.ctypes.data, scan.size,
                                                        C.byref(_global_params(params)), C.byref(info), ms.ctypes.data),
                   "tbnav_icp_localize_map_timed")
        return bool(info.accepted), tuple(info.T), _global_info(info), dict(zip(self.GLOBAL_STAGES, (float(v) for v in ms)))

    def lastGlobal(self) -> dict:
        """the record of the last localizeMap of this handle (searched = 0: none ran)"""
        info = capi.IcpGlobalInfo()
        capi.check(self._L.tbnav_icp_last_global(self._h, C.byref(info)), "tbnav_icp_last_global")
        return _global_info(info)

    def lastGlobalKernels(self) -> list:
        """the last localizeMap's kernels as a profiler prints them; [] before the first call"""
        buf = C.create_string_buffer(256)
        capi.check(self._L.tbnav_icp_last_global_kernels(self._h, buf, 256), "tbnav_icp_last_global_kernels")
        return [k for k in buf.value.decode().split(";") if k]

    @staticmethod
    def _global_shape(filter, p):
        side, s = filter.xsize, 1 << p.pool_log2
        whole = all(v == -1 for v in p.region)
        w = side if whole else p.region[2] - p.region[0] + 1
        h = side if whole else p.region[3] - p.region[1] + 1
        return side, s, w, h

    def localizeMapField(self, filter, particle=capi.ICP_MAP_BEST_PARTICLE, **params):
        """test hook (L9) -> (lik uint8 [side][side] indexed [ci][cj], pool uint8 [side + s - 1][side + s - 1] indexed
        [i + s - 1][j + s - 1], occupied)"""
        p = _global_params(params)
        side, s, _, _ = self._global_shape(filter, p)
        lik = np.zeros((side, side), dtype=np.uint8)
        pool = np.zeros((side + s - 1, side + s - 1), dtype=np.uint8)
        occ = C.c_int32()
        capi.check(self._L.tbnav_icp_localize_map_field(self._h, filter._h, int(particle), C.byref(p), lik.ctypes.data, pool.ctypes.data,
                                                        C.byref(occ)), "tbnav_icp_localize_map_field")
        return lik, pool, int(occ.value)

    def localizeMapBounds(self, filter, scan, particle=capi.ICP_MAP_BEST_PARTICLE, **params):
        """test hook (L9) -> the bound volume, uint32 [NA][nbx][nby]"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        p = _global_params(params)
        _, s, w, h = self._global_shape(filter, p)
        vol = np.zeros((max(p.ang_count, 1), max(-(-w // s), 1), max(-(-h // s), 1)), dtype=np.uint32)
        capi.check(self._L.tbnav_icp_localize_map_bounds(self._h, filter._h, int(particle), scan.ctypes.data, scan.size, C.byref(p),
                                                         vol.ctypes.data), "tbnav_icp_localize_map_bounds")
        return vol

    def localizeMapScores(self, filter, scan, particle=capi.ICP_MAP_BEST_PARTICLE, **params):
        """test hook (L9) -> every candidate's score, uint32 [NA][w][h], by the refinement kernel run over all blocks"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        p = _global_params(params)
        _, _, w, h = self._global_shape(filter, p)
        vol = np.zeros((max(p.ang_count, 1), max(w, 1), max(h, 1)), dtype=np.uint32)
        capi.check(self._L.tbnav_icp_localize_map_scores(self._h, filter._h, int(particle), scan.ctypes.data, scan.size, C.byref(p),
                                                         vol.ctypes.data), "tbnav_icp_localize_map_scores")
        return vol

    def localizeMapHypotheses(self, filter, scan, particle=capi.ICP_MAP_BEST_PARTICLE, hyp=None, cap=None, **params):
        """tbnav_icp_localize_map_hyp (the header's HYPOTHESES, H1-H10): the global search's separated peaks, best first.  hyp: dict of
        max_hyp, floor_q10, sep_cells, sep_steps, wrap (tbnav_icp_default_hyp_params for what is not named); cap: how many records to
        take (default: max_hyp); params: localizeMap's -> (list of dicts T, quality, score, ia, tx, ty, accepted; info dict)"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        hp = _hyp_params(hyp)
        cap = int(hp.max_hyp if cap is None else cap)
        hyps = (capi.IcpHypothesis * max(cap, 1))()
        info = capi.IcpHypInfo()
        capi.check(self._L.tbnav_icp_localize_map_hyp(self._h, filter._h, int(particle), scan.ctypes.data, scan.size,
                                                      C.byref(_global_params(params)), C.byref(hp), C.cast(hyps, C.c_void_p), cap,
                                                      C.byref(info)), "tbnav_icp_localize_map_hyp")
        return [_hypothesis(hyps[i]) for i in range(min(cap, info.n))], _hyp_info(info)

    def lastHyp(self) -> dict:
        """the record of the last localizeMapHypotheses of this handle (searched = 0: none ran)"""
        info = capi.IcpHypInfo()
        capi.check(self._L.tbnav_icp_last_hyp(self._h, C.byref(info)), "tbnav_icp_last_hyp")
        return _hyp_info(info)

    def lastHypKernels(self) -> list:
        """the last localizeMapHypotheses' kernels as a profiler prints them; [] before the first call"""
        buf = C.create_string_buffer(512)
        capi.check(self._L.tbnav_icp_last_hyp_kernels(self._h, buf, 512), "tbnav_icp_last_hyp_kernels")
        return [k for k in buf.value.decode().split(";") if k]

    def localizeMapHypCandidates(self, filter, scan, particle=capi.ICP_MAP_BEST_PARTICLE, hyp=None, **params):
        """test hook (H9): every candidate with score >= the floor, in ascending index order
        -> (index uint32 [m], score uint32 [m], peak uint8 [m])"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        gp, hp = _global_params(params), _hyp_params(hyp)
        count = C.c_int64()
        args = (self._h, filter._h, int(particle), scan.ctypes.data, scan.size, C.byref(gp), C.byref(hp))
        capi.check(self._L.tbnav_icp_localize_map_hyp_candidates(*args, None, None, None, 0, C.byref(count)), "tbnav_icp_localize_map_hyp_candidates")
        m = int(count.value)
        index, score, peak = np.zeros(max(m, 1), np.uint32), np.zeros(max(m, 1), np.uint32), np.zeros(max(m, 1), np.uint8)
        capi.check(self._L.tbnav_icp_localize_map_hyp_candidates(*args, index.ctypes.data, score.ctypes.data, peak.ctypes.data, m, C.byref(count)),
                   "tbnav_icp_localize_map_hyp_candidates")
        assert int(count.value) == m
        return index[:m], score[:m], peak[:m]

    def relocalizeMapHypotheses(self, filter, scan, particle=capi.ICP_MAP_BEST_PARTICLE, localize=None, hyp=None, align=None, verify=None,
                                even_if_rejected=False):
        """localizeMapHypotheses, then ONE alignMapBatch from the hypotheses with accepted = 1 (all of them when even_if_rejected) and ONE
        verifyMapBatch of each of those at its aligned pose, or at its found pose where the alignment did not converge: three synchronous
        calls whatever the number of hypotheses.  localize, hyp, align, verify: dicts of those calls' parameters.
        -> dict(hypotheses=[dict(found=the hypothesis, fine=alignMap's (ok, T, info) or None, check=verifyMap's record or None, T, verified)],
        info=the search's record, verified_count, best (the lowest index verified, -1: none), ambiguous (verified_count > 1),
        T (best's, or hypothesis 0's when none is verified, or None when there is no hypothesis))"""
        hyps, info = self.localizeMapHypotheses(filter, scan, particle, hyp=hyp, **(localize or {}))
        out = [dict(found=y, fine=None, check=None, T=y["T"], verified=False) for y in hyps]
        take = [i for i, y in enumerate(hyps) if y["accepted"] or even_if_rejected]
        if take:
            parts = [int(particle)] * len(take)
            fine = self.alignMapBatch(filter, [hyps[i]["T"] for i in take], scan, parts, **(align or {}))
            for i, f in zip(take, fine):
                out[i]["fine"] = f
                out[i]["T"] = f[1] if f[0] else hyps[i]["T"]
            recs = self.verifyMapBatch(filter, [out[i]["T"] for i in take], scan, parts, **(verify or {}))
            for i, rec in zip(take, recs):
                out[i]["check"] = rec
                out[i]["verified"] = bool(rec["accepted"])
        ver = [i for i, o in enumerate(out) if o["verified"]]
        best = ver[0] if ver else -1
        T = out[best]["T"] if ver else (out[0]["T"] if out else None)
        return dict(hypotheses=out, info=info, verified_count=len(ver), best=best, ambiguous=len(ver) > 1, T=T)

    def alignMap(self, filter, T_init, scan, particle=capi.ICP_MAP_BEST_PARTICLE, **params):
        """tbnav_icp_align_map (the header's MAP ALIGNMENT, A1-A11): the alignment of one scan to the map of a particle of
        `filter` (particle=-1: its best one) from the WORLD guess T_init, below one cell; params: half_cells, gate_cells,
        feature_cells, max_flatness (tbnav_icp_default_align_map_params for what is not named)
        -> (ok, T in the world, info dict); on a failure T is T_init unchanged."""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        out, ok, info = (C.c_double * 3)(), C.c_int32(), capi.IcpInfo()
        capi.check(self._L.tbnav_icp_align_map(self._h, filter._h, int(particle), scan.ctypes.data, scan.size, _d3(T_init),
                                               C.byref(_align_map_params(params)), out, C.byref(ok), C.byref(info)), "tbnav_icp_align_map")
        return bool(ok.value), tuple(out), _info(info)

    def alignMapBatch(self, filter, T_init, scan, particles, **params):
        """tbnav_icp_align_map_batch (A8): one scan, n pairs (particles[i], T_init[i]), each equal to the single call
        -> list of (ok, T, info dict)"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        particles = np.ascontiguousarray(particles, dtype=np.int32).reshape(-1)
        n = particles.size
        T_init = np.ascontiguousarray(T_init, dtype=np.float64).reshape(n, 3)
        T = np.zeros((max(n, 1), 3), dtype=np.float64)
        ok = np.zeros(max(n, 1), dtype=np.int32)
        infos = (capi.IcpInfo * max(n, 1))()
        capi.check(self._L.tbnav_icp_align_map_batch(self._h, filter._h, scan.ctypes.data, scan.size, n, particles.ctypes.data,
                                                     T_init.ctypes.data, C.byref(_align_map_params(params)), T.ctypes.data, ok.ctypes.data,
                                                     C.cast(infos, C.c_void_p)), "tbnav_icp_align_map_batch")
        return [(bool(ok[i]), tuple(float(v) for v in T[i]), _info(infos[i])) for i in range(n)]

    def alignMapPairs(self, filter, T_init, scan, particle=capi.ICP_MAP_BEST_PARTICLE, **params):
        """test hook (A10): iteration 1's pairing, per beam -> dict of arrays [n_beams]: has_home, hi, hj, mi, mj, D, has_normal,
        kept (int32), bx, by (float64), nx, ny (float32)"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        recs = (capi.IcpAlignMapPair * scan.size)()
        capi.check(self._L.tbnav_icp_align_map_pairs(self._h, filter._h, int(particle), scan.ctypes.data, scan.size, _d3(T_init),
                                                     C.byref(_align_map_params(params)), C.cast(recs, C.c_void_p)), "tbnav_icp_align_map_pairs")
        a = np.frombuffer(recs, dtype=_ALIGN_MAP_PAIR).copy()
        return {f: np.ascontiguousarray(a[f]) for f in _ALIGN_MAP_PAIR.names}

    def lastAlignMapKernel(self) -> str:
        """the map alignment's kernel as a profiler prints it; "" until alignMap has run on this handle"""
        buf = C.create_string_buffer(64)
        capi.check(self._L.tbnav_icp_last_align_map_kernel(self._h, buf, 64), "tbnav_icp_last_align_map_kernel")
        return buf.value.decode()

    def relocalizeMap(self, filter, scan, particle=capi.ICP_MAP_BEST_PARTICLE, localize=None, **params):
        """localizeMap, then alignMap from its T when it is accepted: where the robot is in the particle's map, with no guess and
        below one cell.  localize: dict of localizeMap's parameters; params: alignMap's
        -> (ok, T in the world, dict(localize=localizeMap's record, align=alignMap's info or None when the search was rejected))"""
        acc, T, ginfo = self.localizeMap(filter, scan, particle, **(localize or {}))
        if not acc:
            return False, T, dict(localize=ginfo, align=None)
        ok, Ta, info = self.alignMap(filter, T, scan, particle, **params)
        return ok, Ta, dict(localize=ginfo, align=info)

    def verifyMap(self, filter, T, scan, particle=capi.ICP_MAP_BEST_PARTICLE, **params):
        """tbnav_icp_verify_map (the header's MAP CHECK, V1-V10): the WORLD pose T checked against the walls and the free space of
        the map of a particle of `filter` (particle=-1: its best one) with one scan; params: half_cells, slack_cells,
        max_through_q10, max_missing_q10, min_hit_q10 (tbnav_icp_default_verify_map_params for what is not named)
        -> dict of V7's record: points, outside, walked, hit, through, missing, unseen, undecided, free_cells, unknown_cells,
        sensor_cell, sensor_class, accepted"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        info = capi.IcpVerifyMapInfo()
        capi.check(self._L.tbnav_icp_verify_map(self._h, filter._h, int(particle), scan.ctypes.data, scan.size, _d3(T),
                                                C.byref(_verify_map_params(params)), C.byref(info)), "tbnav_icp_verify_map")
        return _verify_map_info(info)

    def verifyMapBatch(self, filter, T, scan, particles, **params):
        """tbnav_icp_verify_map_batch (V8): one scan, n pairs (particles[i], T[i]), each equal to the single call -> list of dicts"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        particles = np.ascontiguousarray(particles, dtype=np.int32).reshape(-1)
        n = particles.size
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(n, 3)
        infos = (capi.IcpVerifyMapInfo * max(n, 1))()
        capi.check(self._L.tbnav_icp_verify_map_batch(self._h, filter._h, scan.ctypes.data, scan.size, n, particles.ctypes.data, T.ctypes.data,
                                                      C.byref(_verify_map_params(params)), C.cast(infos, C.c_void_p)), "tbnav_icp_verify_map_batch")
        return [_verify_map_info(infos[i]) for i in range(n)]

    def verifyMapBeams(self, filter, T, scan, particle=capi.ICP_MAP_BEST_PARTICLE, **params):
        """test hook (V9): the record of every beam -> (verifyMap's dict, dict of int32 arrays [n_beams]: cls, ei, ej, n, b, D,
        free_cells, unknown_cells)"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        info = capi.IcpVerifyMapInfo()
        recs = (capi.IcpVerifyMapBeam * scan.size)()
        capi.check(self._L.tbnav_icp_verify_map_beams(self._h, filter._h, int(particle), scan.ctypes.data, scan.size, _d3(T),
                                                      C.byref(_verify_map_params(params)), C.byref(info), C.cast(recs, C.c_void_p)),
                   "tbnav_icp_verify_map_beams")
        a = np.frombuffer(recs, dtype=_VERIFY_MAP_BEAM).copy()
        return _verify_map_info(info), {f: np.ascontiguousarray(a[f]) for f in _VERIFY_MAP_BEAM.names}

    def lastVerifyMapKernel(self) -> str:
        """the map check's kernel as a profiler prints it; "" until verifyMap has run on this handle"""
        buf = C.create_string_buffer(64)
        capi.check(self._L.tbnav_icp_last_verify_map_kernel(self._h, buf, 64), "tbnav_icp_last_verify_map_kernel")
        return buf.value.decode()

    def relocalizeMapChecked(self, filter, scan, particle=capi.ICP_MAP_BEST_PARTICLE, localize=None, align=None, even_if_rejected=False, **params):
        """localizeMap; when it is accepted (or even_if_rejected) alignMap from the pose it found; then verifyMap at the aligned
        pose, or at the found pose when the alignment did not converge.  localize, align: dicts of those calls' parameters; params:
        verifyMap's.  relocalizeMap itself is untouched.
        -> (verified, T in the world, dict(localize=localizeMap's record, align=alignMap's info or None, aligned=bool,
        verify=verifyMap's record or None)); verified: the search was accepted (or even_if_rejected) and the check accepts the pose"""
        acc, T, ginfo = self.localizeMap(filter, scan, particle, **(localize or {}))
        if not acc and not even_if_rejected:
            return False, T, dict(localize=ginfo, align=None, aligned=False, verify=None)
        ok, Ta, info = self.alignMap(filter, T, scan, particle, **(align or {}))
        Tv = Ta if ok else T
        rec = self.verifyMap(filter, Tv, scan, particle, **params)
        return bool(rec["accepted"]), Tv, dict(localize=ginfo, align=info, aligned=ok, verify=rec)

    def lastSearch(self) -> dict:
        """the search record of the last pclICP / pclICPWrapper, for a wrapperBatch the last scan's (searched = 0: none ran)"""
        info = capi.IcpSearchInfo()
        capi.check(self._L.tbnav_icp_last_search(self._h, C.byref(info)), "tbnav_icp_last_search")
        return _search_info(info)

    def setMetric(self, metric="point", normal_window=0, normal_max_gap=0.0):
        """tbnav_icp_set_metric: "point" | "line" for every later call; normal_window (beams, 0: the default 1) and
        normal_max_gap (metres, 0: the default 0.25) are the line metric's.  The stored scan is kept."""
        if metric not in _METRICS:
            raise ValueError(f"metric must be one of {sorted(_METRICS)}, not {metric!r}")
        capi.check(self._L.tbnav_icp_set_metric(self._h, _METRICS[metric], int(normal_window), float(normal_max_gap)),
                   "tbnav_icp_set_metric")

    def metric(self):
        """-> (metric name, normal_window, normal_max_gap) as the handle holds them"""
        m, w, g = C.c_int32(), C.c_int32(), C.c_double()
        capi.check(self._L.tbnav_icp_get_metric(self._h, C.byref(m), C.byref(w), C.byref(g)), "tbnav_icp_get_metric")
        return {v: k for k, v in _METRICS.items()}[m.value], w.value, g.value

    def normals(self, scan):
        """the normals the line metric gives one scan taken as a target, per beam: (float32 [n_beams][2], int32 [n_beams]
        flags); a beam without a normal holds (0, 0) and 0"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        nxy = np.zeros((scan.size, 2), dtype=np.float32)
        has = np.zeros(scan.size, dtype=np.int32)
        capi.check(self._L.tbnav_icp_normals(self._h, scan.ctypes.data, scan.size, nxy.ctypes.data, has.ctypes.data),
                   "tbnav_icp_normals")
        return nxy, has

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.tbnav_icp_destroy(self._h)
        self._h = C.c_void_p()

    __del__ = close

    def reset(self):
        capi.check(self._L.tbnav_icp_reset(self._h), "tbnav_icp_reset")

    def pclICPWrapper(self, T_init, scan):
        """-> (ok, T = (theta, x, y), info dict)"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        out = (C.c_double * 3)()
        ok = C.c_int32()
        info = capi.IcpInfo()
        capi.check(self._L.tbnav_icp_step(self._h, scan.ctypes.data, scan.size, _d3(T_init), out, C.byref(ok), C.byref(info)),
                   "tbnav_icp_step")
        return bool(ok.value), tuple(out), _info(info)

    def pclICP(self, T_init, target_scan, source_scan):
        """-> (ok, T, info dict); stateless"""
        tgt = np.ascontiguousarray(target_scan, dtype=np.float32)
        src = np.ascontiguousarray(source_scan, dtype=np.float32)
        if tgt.size != src.size:
            raise ValueError("target and source scans must have the same number of beams")
        out = (C.c_double * 3)()
        info = capi.IcpInfo()
        capi.check(self._L.tbnav_icp_match(self._h, tgt.ctypes.data, src.ctypes.data, src.size, _d3(T_init), out, C.byref(info)),
                   "tbnav_icp_match")
        return converged(info.criterion), tuple(out), _info(info)

    def wrapperBatch(self, T_init, scans):
        """n successive pclICPWrapper calls in one call: T_init [n][3], scans [n][n_beams] -> (ok int32 [n], T [n][3],
        info list)"""
        scans = np.ascontiguousarray(scans, dtype=np.float32)
        n, nb = scans.shape
        T_init = np.ascontiguousarray(T_init, dtype=np.float64).reshape(n, 3)
        ok = np.zeros(n, dtype=np.int32)
        T = np.zeros((n, 3), dtype=np.float64)
        info = (capi.IcpInfo * n)()
        capi.check(self._L.tbnav_icp_step_batch(self._h, scans.ctypes.data, nb, n, T_init.ctypes.data, ok.ctypes.data,
                                                T.ctypes.data, C.cast(info, C.c_void_p)), "tbnav_icp_step_batch")
        return ok, T, [_info(i) for i in info]

    def lastBatchLaunches(self) -> int:
        return int(self._L.tbnav_icp_last_batch_launches(self._h))

    def cloud(self, scan):
        """the cloud the kernel builds from one scan: float32 [m][2] in beam order"""
        scan = np.ascontiguousarray(scan, dtype=np.float32)
        xy = np.empty((scan.size, 2), dtype=np.float32)
        m = C.c_int32()
        capi.check(self._L.tbnav_icp_cloud(self._h, scan.ctypes.data, scan.size, xy.ctypes.data, C.byref(m)), "tbnav_icp_cloud")
        return xy[:m.value].copy()
