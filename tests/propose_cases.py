"""The case table of the RBPF proposal kernel (csrc/rbpf_propose.hip: rbpf_propose<NT, DN>, four instantiations, six phases).  Plain
data, the host expressions of csrc/rbpf_plan.hpp::plan_propose that choose the instantiation and the staging form, restated, and the
kernel's own rules restated in float64 over the oracle's numbers: which beams a particle's samples can move out of the centre's cell
(U_true), which the kernel's bound calls unstable (U_rule), the per-wave segment counts of its list, and which query-mode lookups
the 7 x 7 look settles.  tests/test_propose_cases.py proves the table on the CPU with the oracle alone;
tests/test_rbpf_propose_gpu.py runs it on the device.  The kernel reports nothing about its phases: which path a case takes is
established by these restatements.

A run: as in tests/scanmatch_cases.py the filters start at `start - inc`, so the particles' frame is the world's.  A case names the
field sources it runs in — `inj`: the oracle's brushfire field injected before every scan, against the plain oracle; `query`,
`window`, `full`: nothing injected, against the `exact_field` oracle — and its noise: `host` (a stored stream handed to both sides)
or `dn` (drawn inside the kernel; the oracle is fed the stream the device reports afterwards).

k = 2 and 3 are left out on purpose: with fewer than four samples `sigma` is singular, and the sign of a pivot that is zero to
rounding decides whether the reference's LLT stops — a property of the reference, not of the kernel.
"""
import math
from collections import namedtuple

import numpy as np

import oracle_api as orc
import rbpf_cases as rc
import scanmatch_cases as smc

ZERO = (0.0, 0.0, 0.0)
START = (0.01, 0.012, 0.007)       # (from (0, 0, 0) beam 0 of the first scan ends ON the border y = 0 of its cell)
RES = 0.05                        # the shipped cell size, and the default of a case's `res`
K_UNCAP = 16                      # rbpf_plan.hpp: kUnCap
K_MAX_LDS = 160 * 1024            # kMaxLds
K_PROPOSE_THREADS = 256           # kProposeThreads (TBNAV_PROPOSE_THREADS)
K_WAVE = 64
K_TS_SHIFT = 5                    # kTSh: 32 x 32-cell tiles
K_MIX_LDS, K_MIX_LUT = 128, 1024  # kMixLds, kMixLut: the tiers of mix_term
DEFAULT_VAR = (1e-10, 1e-8, 1e-8)           # slam.launch's sample_range
DEFAULT_CLAMPS = (1.0, 20.0, 1.0, 10.0)     # scan_min, scan_max, pose_min, pose_max
BORDER_MIN = 1e-12                # no end point the oracle computes may be nearer than this to a cell border
ROOM_EDGE = smc.ROOM_EDGE
ROOM_TINY = (-1.0, 1.0, -0.8, 0.9)          # the room mapped first in the lookups cases
ROOM_FAR = (-2.4, 2.5, -2.2, 2.3)           # walls 20 to 40 cells beyond it
ROOM_TIERS = (-2.9, 1.8, -1.5, 1.3)         # walls 38, 16, 14 and 8 cells beyond it: codes >= 1024, in 128..1023, below 128

# id; group; map half-extent -> cells; room; range_max; Trs; start pose; true increment per scan; N, k, beams; sources; noises; number
# of scans; seed of the range noise; valid = {scan: number of beams left valid, {beam: range}, or the name of a hand-made scan};
# var = sample_range; clamps; icp = per-scan icp_ok; u_at = {scan: (w, vx)} handed over instead of the true twist's; resample_at;
# shard = (first, extra) for setRngShard(first, N + extra); window of the oracle's maps; walls_at = {first scan: room};
# reset_at = scans before which every particle is put on the true pose; threads = the workgroup size the case must launch;
# expect = what else the case claims (see the CPU test); res = the cell size.
Case = namedtuple("Case", "id group half cells room range_max trs start inc N k beams sources noises n_scans seed valid var clamps icp "
                          "u_at resample_at shard window walls_at reset_at threads expect res", defaults=(RES,))


def _case(id, group, half=2.0, room=rc.ROOM_SMALL, range_max=3.5, trs=ZERO, start=START, inc=(0.04, 0.03, 0.02), N=4, k=10, beams=360,
          sources=("inj", "query"), noises=("host",), n_scans=3, seed=5, valid=None, var=DEFAULT_VAR, clamps=DEFAULT_CLAMPS, icp=True,
          u_at=None, resample_at=None, shard=None, window=None, walls_at=None, reset_at=(), threads=256, expect=None, res=RES):
    icp = (icp,) * n_scans if isinstance(icp, bool) else tuple(icp)
    assert len(icp) == n_scans
    return Case(id, group, half, int(math.ceil(2 * half / res)), room, range_max, trs, start, inc, N, k, beams, tuple(sources), tuple(noises),
                n_scans, seed, valid or {}, tuple(var), tuple(clamps), icp, u_at or {}, resample_at, shard, window, walls_at or {},
                tuple(reset_at), threads, expect or {}, res)


_ALL = (4e-4, 4e-3, 4e-3)          # tests/test_rbpf_gpu.py's widest spread: sigma 6 cm against 5 cm cells, every beam unstable
_BIG_WIN = (290, 410, 290, 410)    # +-3 m round the centre of a 700-cell map
_FAIL = dict(group="icp-failed", icp=False, sources=("inj", "query"), noises=("host", "dn"))


# look7-limit: beam 5 of scan 1 (5 degrees, as the scanner steps in float) ends on the centre of B from the centre of row 60
_L7_A5 = 5.0 * float(np.float32(np.deg2rad(1.0)))
_L7_RB = 0.15 / math.sin(_L7_A5)
_L7_X0 = 1.675 - _L7_RB * math.cos(_L7_A5) + 0.15      # the robot's x on scan 0; scans 1 and 2 are 0.15 and 0.3 m behind it


def _sizes():
    out = []
    for k in (1, 4, 63, 64, 65, 97, 98, 511, 512, 513, 577, 646):
        dn = k in (4, 65, 97, 98, 513, 646)
        out.append(_case(f"k-{k}", "sizes", k=k, noises=("host", "dn") if dn else ("host",), threads=512 if k >= 98 else 256,
                         expect=dict(more_samples_than_threads=k > 512)))
    out.append(_case("k-647", "sizes", k=647, n_scans=1, threads=None, expect=dict(unsupported=True)))
    return out


def _beams():
    both = ("host", "dn")
    out = [_case(f"valid-{n}", "beams", n_scans=4, valid={2: n}, k=10, noises=both if n in (1, 65) else ("host",), expect=dict(valid_at={2: n}))
           for n in (1, 3, 7, 63, 64, 65, 357)]
    out += [_case(f"valid-{n}-k170", "beams", n_scans=4, valid={2: n}, k=170, threads=512, noises=both if n == 7 else ("host",),
                  expect=dict(valid_at={2: n})) for n in (1, 7)]
    out.append(_case("beams-1080-k10", "beams", beams=1080, k=10, threads=512))
    out.append(_case("beams-1080-k120", "beams", beams=1080, k=120, threads=512))
    return out


CASES = tuple(_sizes() + _beams() + [
    # ---- split: the stable / unstable rule, the chunks of kUnCap unstable beams, the per-wave segments of the list
    _case("split-default", "split", half=3.0, N=8, k=20, n_scans=4, sources=("inj", "query", "window", "full"), noises=("host", "dn"),
          expect=dict(unstable=(0, 40))),
    _case("split-16", "split", half=3.0, n_scans=4, valid={2: 16, 3: 16}, var=_ALL, expect=dict(unstable_at={2: 16, 3: 16})),
    _case("split-17", "split", half=3.0, n_scans=4, valid={2: 17, 3: 17}, var=_ALL, expect=dict(unstable_at={2: 17, 3: 17})),
    _case("split-32", "split", half=3.0, n_scans=4, valid={2: 32, 3: 32}, var=_ALL, expect=dict(unstable_at={2: 32, 3: 32})),
    _case("split-33", "split", half=3.0, n_scans=4, valid={2: 33, 3: 33}, var=_ALL, noises=("host", "dn"), expect=dict(unstable_at={2: 33, 3: 33})),
    _case("split-all-360", "split", half=3.0, var=_ALL, expect=dict(unstable_at={1: 360, 2: 360})),
    _case("split-all-360-k98", "split", half=3.0, var=_ALL, k=98, threads=512, noises=("host", "dn"), expect=dict(unstable_at={1: 360, 2: 360})),
    # rotation alone: the samples' positions are the centre's to 1e-6 m, their headings differ by 1e-2 rad — only the angular term
    # of the bound can call a beam unstable; with Trs the SENSOR travels under that rotation (0.36 m x 1e-2 rad), the robot does not
    _case("rot-spread", "split", var=(1e-4, 1e-12, 1e-12), noises=("host", "dn"), expect=dict(unstable=(20, 360), discriminates="angular")),
    _case("trs-rot-spread", "split", half=3.0, var=(1e-4, 1e-12, 1e-12), trs=(0.3, 0.3, -0.2), expect=dict(unstable=(20, 360), discriminates="sensor")),
    # unstable beams in the first and the last wave's range only / in the last alone: hand-made scans whose end points sit in the middle
    # of their cells except for a few that sit 50 um from a border (every particle is put on the true pose first)
    _case("segments", "split", valid={2: "segments"}, reset_at=(2,), expect=dict(segments_at={2: (True, False, False, True)})),
    _case("last-wave-only", "split", valid={2: "last-wave"}, reset_at=(2,), expect=dict(segments_at={2: (False, False, False, True)})),
    _case("segments-512", "split", k=98, valid={2: "segments-8"}, reset_at=(2,), threads=512,
          expect=dict(segments_at={2: (True,) + (False,) * 6 + (True,)})),
    # ---- lookups (query mode): lookup_code_fast (look7), the deferred searches, the staging forms, the tiers of mix_term
    # the limit of the 7 x 7 look, on a hand-made map of two cells (the method of scanmatch_cases' slice-clear: single-beam scans, the robot
    # backing away 3 cells per scan along its heading 0): scan 0 marks A = (94, 60) with beam 0, scan 1 marks B = (93, 63) with beam 5, and
    # scan 2's only beam ends on L = (90, 60).  d2(L, A) = 16, four cells along the row and outside the look; d2(L, B) = 18, at (3, 3), its
    # corner.  The look alone answers 18, which `bw <= 9` refuses: the deferred search answers 16.  A limit of 18 would accept the 18.
    _case("look7-limit", "lookups", half=3.0, start=(0.0, _L7_X0, 0.025), inc=(0.0, -0.15, 0.0), sources=("query",), noises=("host", "dn"),
          valid={0: {0: 1.725 - _L7_X0}, 1: {5: _L7_RB}, 2: {0: 1.525 - (_L7_X0 - 0.3)}},
          expect=dict(look7=dict(at=2, A=(94, 60), B=(93, 63), L=(90, 60)))),
    _case("deferred-centre", "lookups", half=3.0, room=ROOM_TINY, inc=(0.05, 0.03, 0.02), n_scans=5, walls_at={3: ROOM_FAR}, sources=("query",),
          noises=("host", "dn"), expect=dict(unsettled_centre_at=(3,), settled_centre_at=(1, 2))),
    _case("deferred-pair", "lookups", half=3.0, var=(4e-4, 1e-2, 1e-2), sources=("query",), noises=("host", "dn"),
          expect=dict(unsettled_pair_at=(1, 2), unstable_at={1: 360, 2: 360})),
    _case("deferred-pair-k98", "lookups", half=3.0, k=98, threads=512, var=(4e-4, 1e-2, 1e-2), sources=("query",), noises=("host", "dn"),
          expect=dict(unsettled_pair_at=(1, 2), unstable_at={1: 360, 2: 360})),
    _case("lut-tiers", "lookups", half=4.0, room=ROOM_TINY, inc=(0.05, 0.03, 0.02), n_scans=5, walls_at={3: ROOM_TIERS}, sources=("query",),
          expect=dict(tiers_at=3, unsettled_centre_at=(3,))),
    _case("cells-512", "lookups", half=12.8, sources=("query",), window=(196, 316, 196, 316), expect=dict(staging="whole_table")),
    _case("cells-544", "lookups", half=13.6, sources=("query",), window=(212, 332, 212, 332), expect=dict(staging="ids")),
    _case("cells-700-ids", "lookups", half=17.5, range_max=3.5, sources=("query",), window=_BIG_WIN, expect=dict(staging="ids")),
    _case("cells-700-words", "lookups", half=17.5, range_max=12.0, threads=512, sources=("query",), window=_BIG_WIN, expect=dict(staging="words")),
    _case("cells-700-none", "lookups", half=17.5, range_max=16.0, sources=("query",), window=_BIG_WIN, expect=dict(staging="none")),
    _case("edge", "lookups", room=ROOM_EDGE, inc=(0.0, 0.03, 0.02), sources=("query",), var=(1e-8, 1e-6, 1e-6),
          expect=dict(staging="whole_table", slice_at_map_border=True)),
    # ---- ICP failed: the motion model's two branches, every wave looking up, both workgroup sizes, status 4 from this branch
    _case("fail-arc", u_at={s: (0.04, None) for s in range(3)}, **_FAIL),
    _case("fail-straight", inc=(0.0, 0.03, 0.02), u_at={s: (0.0, None) for s in range(3)}, expect=dict(straight=True), **_FAIL),
    _case("fail-nearly-straight", inc=(0.0, 0.03, 0.02), u_at={s: (1e-13, None) for s in range(3)}, expect=dict(straight=True), **_FAIL),
    _case("fail-1080", beams=1080, inc=(0.0, 0.03, 0.02), u_at={s: (0.0, None) for s in range(3)}, threads=512, expect=dict(straight=True), **_FAIL),
    _case("fail-after-ok", group="icp-failed", icp=(True, True, False, True), n_scans=4, noises=("host", "dn")),
    _case("fail-out-of-world", group="icp-failed", icp=(True, True, False), room=ROOM_EDGE, inc=(0.0, 0.03, 0.02), u_at={2: (0.0, 0.4)},
          expect=dict(status_at={2: 4})),
    # ---- clamps and statuses
    # (scan-max-binds: with the scan term at 1e-30 the pose term is held at 1e20, or eta would be zero to almost_equal)
    _case("open", "clamps", half=3.0, var=_ALL, clamps=(1e-300, 1e300, 1e-300, 1e300), noises=("host", "dn"),
          expect=dict(unstable_at={1: 360, 2: 360})),
    _case("open-k98", "clamps", half=3.0, var=_ALL, k=98, threads=512, clamps=(1e-300, 1e300, 1e-300, 1e300), noises=("host", "dn"),
          expect=dict(unstable_at={1: 360, 2: 360})),
    _case("scan-max-binds", "clamps", half=3.0, var=_ALL, clamps=(1e-300, 1e-30, 1e20, 1e300), expect=dict(scan_clamp="max-all")),
    _case("scan-max-some", "clamps", half=3.0, var=_ALL, clamps=(1e-300, 1.5, 1e-300, 1e300), expect=dict(scan_clamp="max-some")),
    _case("scan-min-binds", "clamps", half=3.0, var=_ALL, clamps=(1e30, 1e31, 1e-300, 1e300), expect=dict(scan_clamp="min-all")),
    _case("eta-zero", "clamps", clamps=(0.0, 1e-8, 0.0, 1e-8), expect=dict(status_at={0: 5})),
    _case("eta-small", "clamps", clamps=(0.0, 4e-7, 0.0, 1e-6), expect=dict(eta_near=4e-12)),
    _case("sample-out-of-world", "clamps", room=ROOM_EDGE, inc=(0.0, 0.03, 0.02), var=(1e-4, 1e-4, 1e-4), valid={2: "edge-beam"},
          reset_at=(2,), expect=dict(status_at={2: 4}, centre_inside_at=2)),
    # ---- geometry
    _case("trs", "geometry", trs=(0.3, 0.05, -0.02), half=3.0, noises=("host", "dn")),
    _case("trs-k98", "geometry", trs=(0.3, 0.05, -0.02), half=3.0, k=98, threads=512, noises=("host", "dn")),
    _case("heading-pi", "geometry", half=3.0, start=(3.1415, 0.0, 0.0), inc=(0.0, 0.03, 0.02), var=(1e-6, 1e-8, 1e-8), expect=dict(both_sides_of_pi=True)),
    _case("after-resample", "geometry", N=16, n_scans=4, resample_at=2, noises=("host", "dn"), expect=dict(resampled_at=(2,))),
    _case("rng-shard-even", "geometry", k=10, noises=("dn",), shard=(3, 5)),
    _case("rng-shard-odd", "geometry", k=11, noises=("dn",), shard=(3, 5)),
])


# ---- other cell sizes (group `res`): the quantities the kernel counts in cells — the slice's reach and margin, the mixture table's codes, the
# 7 x 7 look, the stable-beam bound against a cell's width — at the sizes of raycast_cases.RES_TABLE.  One case with the shipped spread and
# one with _ALL's (sigma 6 cm: 1.5 cells at 0.0394 m, an eighth of a cell at 0.5 m), each in every field source and noise form; what each
# claims (expect: unstable = (least, most) unstable beams of a particle after the first scan; tiers = the tiers of mix_term its lookups take;
# centre_settled = whether the 7 x 7 look settles every / some / no centre lookup; margin = the slice margin plan_propose ends on) was counted
# by tests/test_propose_cases.py from the oracle's numbers.
RES_SIZES = (0.0394, 0.0625, 0.07, 0.3, 0.5)
ROOM_RES = (-1.2, 1.1, -1.0, 1.3)           # on the +-2 m map with 0.6 m to spare: _ALL's samples (sigma 6 cm) keep every end point inside
_EVERY = dict(sources=("inj", "query", "window", "full"), noises=("host", "dn"))
ROOM_0394_IN, ROOM_0394_OUT = (-0.5, 0.5, -0.4, 0.45), (-1.85, 0.75, -0.4, 0.95)    # walls 34, 6, 0 and 13 cells of 0.0394 m beyond the first room's
RES_EXPECT = {
    "res-0p0394": dict(unstable=(3, 11), tiers=("lds",), centre_settled="every", margin=48),
    "res-0p0394-wide": dict(unstable=(360, 360), tiers=("lds",), centre_settled="every", margin=48),
    "res-0p0625": dict(unstable=(3, 7), tiers=("lds",), centre_settled="some", margin=48),
    "res-0p0625-wide": dict(unstable=(360, 360), tiers=("lds",), centre_settled="some", margin=48),
    "res-0p07": dict(unstable=(2, 10), tiers=("lds",), centre_settled="some", margin=48),
    "res-0p07-wide": dict(unstable=(360, 360), tiers=("lds",), centre_settled="some", margin=48),
    "res-0p3": dict(unstable=(0, 5), tiers=("lds",), centre_settled="some", margin=48),
    "res-0p3-wide": dict(unstable=(356, 360), tiers=("lds",), centre_settled="some", margin=48),
    "res-0p5": dict(unstable=(1, 2), tiers=("lds",), centre_settled="some", margin=48),
    "res-0p5-wide": dict(unstable=(275, 360), tiers=("lds",), centre_settled="some", margin=48),
    "res-0p07-k110": dict(unstable=(360, 360), tiers=("lds",), centre_settled="some", margin=48),
    # the one size at which a +-2 m map holds codes of all three tiers (32 cells are 1.26 m): lut-tiers' method
    "res-0p0394-tiers": dict(tiers_at=3, unsettled_centre_at=(3,), margin=48),
}


def res_tag(res):
    return repr(res).replace(".", "p")


def _res_cases():
    out = []
    for res in RES_SIZES:
        tag = res_tag(res)
        out.append(_case(f"res-{tag}", "res", res=res, room=ROOM_RES, expect=RES_EXPECT.get(f"res-{tag}"), **_EVERY))
        out.append(_case(f"res-{tag}-wide", "res", res=res, room=ROOM_RES, var=_ALL, expect=RES_EXPECT.get(f"res-{tag}-wide"), **_EVERY))
    # (the 512-thread instantiations at a cell size whose reciprocal is no double)
    out.append(_case("res-0p07-k110", "res", res=0.07, room=ROOM_RES, k=110, threads=512, var=_ALL, sources=("inj", "query"), noises=("host", "dn"),
                     expect=RES_EXPECT.get("res-0p07-k110")))
    out.append(_case("res-0p0394-tiers", "res", res=0.0394, room=ROOM_0394_IN, inc=(0.05, 0.03, 0.02), n_scans=5, walls_at={3: ROOM_0394_OUT},
                     sources=("query",), expect=RES_EXPECT.get("res-0p0394-tiers")))
    return out


CASES = CASES + tuple(_res_cases())
CASE = {c.id: c for c in CASES}
GROUPS = ("sizes", "beams", "split", "lookups", "icp-failed", "clamps", "geometry", "res")


_Slice = namedtuple("_Slice", "cells range_max res")     # what scanmatch_cases.slice_regime reads of a case


def runs_of(case):
    """The (source, noise) pairs a case runs in."""
    return [(s, n) for s in case.sources for n in case.noises]


# ---- the host expressions of csrc/rbpf_plan.hpp::plan_propose, restated (tests/test_rbpf_plan.py runs the C++ against these) -----------------------------------------------------------------------
def occ_half(case, source):
    """Half-width of the LDS slice of the occupancy bitmap; 0: none.  (scanmatch_cases.slice_regime is the restated loop; the handle's
    distance-field mode decides whether it runs: an injected field does not change the mode, `window` and `full` do.)"""
    return smc.slice_regime(_Slice(case.cells, case.range_max, case.res))[1] if source in ("inj", "query") else 0


def slice_bytes(case, source):
    half = occ_half(case, source)
    if half == 0:
        return 0
    rows, nw = min(case.cells, 2 * half + 1), min((case.cells + 63) // 64, (2 * half + 1 + 63) // 64 + 1)
    return rows * nw * 8 + rows * 4


def propose_lds(k, Bv, slice_b):
    bv = Bv if Bv > 0 else 1
    return 8 * ((12 + K_UNCAP) * k + 3 * bv) + 4 * 4 * bv + slice_b


def threads(k, Bv, slice_b):
    return 2 * K_PROPOSE_THREADS if propose_lds(k, Bv, slice_b) + 3072 > K_MAX_LDS // 4 else K_PROPOSE_THREADS


def fits(k, Bv, slice_b):
    return propose_lds(k, Bv, slice_b) <= K_MAX_LDS - 3072


def name(nt, dn):
    return f"rbpf_propose<{nt}, {'true' if dn else 'false'}>"


def staging(cells, half, sensor_cell, nt):
    """How rbpf_propose stages its slice of the bitmap round the sensor's cell: `whole_table` (the tile table in registers), `ids`
    (the ids of the tiles under the slice in st_ids), `words` (word by word through OccT::word) or `none`."""
    if half <= 0:
        return "none"
    sci, scj = sensor_cell
    tw = (cells + 31) >> K_TS_SHIFT
    R0, R1 = max(0, sci - half), min(cells - 1, sci + half)
    W0, W1 = max(0, scj - half) >> 6, min(cells - 1, scj + half) >> 6
    nW = W1 - W0 + 1
    whole = tw * tw <= nt and tw * tw <= 256
    ntc = min(2 * nW, tw - 2 * W0)
    n_ids = ((R1 >> K_TS_SHIFT) - (R0 >> K_TS_SHIFT) + 1) * ntc
    if ntc <= 12 and (whole or n_ids <= 256):
        return "whole_table" if whole else "ids"
    return "words"


def slice_box(cells, half, sensor_cell):
    """(R0, R1, C0, C1) of the staged slice."""
    sci, scj = sensor_cell
    R0, R1 = max(0, sci - half), min(cells - 1, sci + half)
    W0, W1 = max(0, scj - half) >> 6, min(cells - 1, scj + half) >> 6
    return R0, R1, W0 * 64, (W1 + 1) * 64 - 1


# ---- the kernel's rules, restated in float64 ------------------------------------------------------------------------------------------
def sensor_xy(case, pose):
    """Position of the sensor at T(pose) * Trs."""
    th, x, y = pose[..., 0], pose[..., 1], pose[..., 2]
    return np.stack([np.cos(th) * case.trs[1] - np.sin(th) * case.trs[2] + x, np.sin(th) * case.trs[1] + np.cos(th) * case.trs[2] + y], -1)


def cells_of(case, xy):
    """grid_mapper.cpp:852-887 for points inside the world: (i, j) and the distance of each point from its cell's nearest border."""
    d = (xy + case.half) / case.res
    ij = np.minimum(np.floor(d), case.cells - 1).astype(np.int64)
    border = np.abs(d - np.round(d)).min(-1) * case.res
    return ij, border


def inside(case, xy):
    return (np.abs(xy) <= case.half).all(-1)


def unstable_sets(case, centre, centre_xy, samples, samples_xy, z_theta, sensor_from="sensor", angular=True):
    """Per particle of one scan: U_true (beams some sample sees in another cell than the centre does) and U_rule (beams the kernel's
    bound `marg <= sdxy + |beam| * sdth + 1e-9` calls unstable; marg a float rounded down, |beam| the fp32 root rounded up).
    The kernel ALSO calls a beam unstable whose centre lookup gave no code (`ctag[b] >= 0x10000`: the centre's end point outside the world, or
    outside the refreshed window) — not restated here: callers pass centres that are inside the world, and no case misses its window.
    centre [3], centre_xy [Bv][2], samples [k][3], samples_xy [k][Bv][2], z_theta [k] the samples' first normals.
    sensor_from="robot" / angular=False: the two mutants of the bound the discrimination test needs."""
    cc, _ = cells_of(case, centre_xy)
    sc, _ = cells_of(case, samples_xy)
    u_true = (sc != cc[None]).any(-1).any(0)
    sens_c = sensor_xy(case, centre) if sensor_from == "sensor" else centre[1:]
    sens_s = sensor_xy(case, samples) if sensor_from == "sensor" else samples[:, 1:]
    sdxy = float(np.abs(sens_s - sens_c[None]).max()) if len(samples) else 0.0
    sdth = float(np.abs(math.sqrt(case.var[0]) * z_theta).max()) if (angular and len(samples)) else 0.0
    lo = centre_xy - (np.floor((centre_xy + case.half) / case.res) * case.res - case.half)
    marg = np.minimum(lo, case.res - lo).min(-1)
    marg32 = marg.astype(np.float32)
    marg32 = np.where(marg32.astype(np.float64) > marg, np.nextafter(marg32, np.float32(-1.0)), marg32).astype(np.float64)
    beam = centre_xy - sensor_xy(case, centre)[None]
    norm32 = np.sqrt((beam ** 2).sum(-1).astype(np.float32)) * np.float32(1.000001)
    delta = sdxy + norm32.astype(np.float64) * sdth + 1e-9
    return u_true, marg32 <= delta


def segment_counts(unstable, nt):
    """Unstable beams per wave's contiguous range of beams, kPW = NT / 64 waves."""
    kpw = nt // K_WAVE
    Bv = len(unstable)
    seg = (Bv + kpw - 1) // kpw
    return [int(unstable[w * seg:min(Bv, (w + 1) * seg)].sum()) for w in range(kpw)]


def nearest_d2(case, ij, occ):
    """Squared distance (cells) of every cell in ij [..., 2] to the nearest of the occupied cells (row-major indices)."""
    oi, oj = occ // case.cells, occ % case.cells
    flat = ij.reshape(-1, 2)
    return ((flat[:, None, 0] - oi[None]) ** 2 + (flat[:, None, 1] - oj[None]) ** 2).min(1).reshape(ij.shape[:-1])


def look7_fits(case, ij, box):
    """Whether the 7 x 7 look (csrc/rbpf_lookup.hpp: look7, what lookup_code_fast is in query mode) can run at all at the cells ij: its rows lie inside the slice's and its seven columns inside
    the slice's 32-bit pieces (`ci - 3 >= R0 && ci + 3 <= R1 && p0 >= 0 && wi + 1 < 2 * nW && cj <= C1`)."""
    R0, R1, C0, C1 = box
    ci, cj = ij[..., 0], ij[..., 1]
    nW2 = 2 * ((C1 + 1 - C0) // 64)
    return (ci - 3 >= R0) & (ci + 3 <= R1) & (cj - C0 - 3 >= 0) & (((cj - C0 - 3) >> 5) + 1 < nW2) & (cj <= C1)


def look7_settles(case, ij, occ, box):
    """Which lookups look7 settles (the others come back from lookup_code_fast as kNeedSearch): the look fits the slice (look7_fits), and the nearest occupied cell among its
    49 is within d2 <= 9 and <= clear^2."""
    R0, R1, C0, C1 = box
    oi, oj = occ // case.cells, occ % case.cells
    flat = ij.reshape(-1, 2)
    di, dj = flat[:, None, 0] - oi[None], flat[:, None, 1] - oj[None]
    d2 = np.where((np.abs(di) <= 3) & (np.abs(dj) <= 3), di * di + dj * dj, 1 << 30).min(1)
    ci, cj = flat[:, 0], flat[:, 1]
    fit = look7_fits(case, flat, box)
    clear = np.full(ci.shape, int(math.ceil(10.0 / case.res)) + 1)          # (cell_radius + 1: 201 at 0.05 m)
    if R0 > 0:
        clear = np.minimum(clear, ci - R0 + 1)
    if R1 < case.cells - 1:
        clear = np.minimum(clear, R1 - ci + 1)
    if C0 > 0:
        clear = np.minimum(clear, cj - C0 + 1)
    if C1 < case.cells - 1:
        clear = np.minimum(clear, C1 - cj + 1)
    return (fit & (d2 <= 9) & (d2 <= clear * clear)).reshape(ij.shape[:-1])


# ---- a run ------------------------------------------------------------------------------------------------------------------------
def common_params(case):
    lo = tuple(a - b for a, b in zip(case.start, case.inc))
    return dict(N=case.N, k=case.k, map_min=-case.half, map_max=case.half, pose0=lo, beam_delta_deg=360.0 / case.beams,
                range_max=case.range_max, Trs=list(case.trs), sample_range=list(case.var), resolution=case.res)


def oracle_params(case):
    c = case.clamps
    return orc.pf_params(scan_min=c[0], scan_max=c[1], pose_min=c[2], pose_max=c[3], **common_params(case))


def device_params_kw(case):
    c = case.clamps
    return dict(scan_likelihood_min=c[0], scan_likelihood_max=c[1], pose_likelihood_min=c[2], pose_likelihood_max=c[3], **common_params(case))


def oracle_filter(case, source):
    if source == "inj":
        assert case.window is None
        return orc.PfAPI(oracle_params(case))
    return orc.PfAPI(oracle_params(case), exact_field=True, window=case.window)


def room_at(case, s):
    room = case.room
    for first in sorted(case.walls_at):
        if s >= first:
            room = case.walls_at[first]
    return room


def _beam_angle(case, pose, b):
    return pose[0] + case.trs[0] + np.deg2rad(np.float32(360.0 / case.beams)) * b


# hand-made scans: the beams (of 360) that end 50 um inside a cell border; every other beam ends as far from its cell's borders as it can.
# 4 waves (256 threads) own beams [0, 90), [90, 180), [180, 270), [270, 360); 8 waves (512 threads) own 45 beams each.
_NEAR = {"segments": (5, 20, 40, 60, 80, 275, 300, 320, 340, 355),      # first and last of 4 ranges
         "last-wave": (275, 300, 320, 340, 355),                        # the last of 4 ranges alone
         "segments-8": (5, 20, 40, 320, 340, 355)}                      # first and last of 8 ranges


def _handmade(kind, case, pose, scan):
    """Hand-made scans, as seen from the true pose.  `edge-beam`: beam 0 ends 1 mm inside the map's +x border.  The kinds of _NEAR: the
    beams named there end 50 um past a cell border along the axis they mostly run along (unstable at the shipped spread of 1e-4 m);
    every other beam's range is moved by less than 3 cm to where its end point is farthest from its cell's borders (stable)."""
    sens = sensor_xy(case, np.asarray(pose, dtype=np.float64))
    out = scan.copy()
    if kind == "edge-beam":
        out[0] = np.float32((case.half - 1e-3 - sens[0]) / math.cos(_beam_angle(case, pose, 0)))
        return out
    near = {b * case.beams // 360 for b in _NEAR[kind]}
    offs = np.arange(-0.03, 0.03, 1e-4)
    for b in range(scan.size):
        a = _beam_angle(case, pose, b)
        dirv = np.array([math.cos(a), math.sin(a)])
        if b in near:
            ax = 0 if abs(dirv[0]) >= abs(dirv[1]) else 1
            at = sens[ax] + float(scan[b]) * dirv[ax]                                  # where the room's own range ends along that axis
            line = math.floor((at + case.half) / case.res) * case.res - case.half   # the border of that cell on the sensor's side
            out[b] = np.float32((line + 5e-5 * np.sign(dirv[ax]) - sens[ax]) / dirv[ax])
        else:
            r = float(scan[b]) + offs
            lo = (sens[None] + r[:, None] * dirv[None] + case.half) / case.res
            lo = (lo - np.floor(lo)) * case.res
            out[b] = np.float32(r[int(np.argmax(np.minimum(lo, case.res - lo).min(-1)))])
    return out


Scan = namedtuple("Scan", "s scan u cur prev guess normals icp_ok weights reset_pose")


def scans(case):
    """The inputs of every scan of the case, in order (normals: the host stream; a `dn` run replaces it)."""
    steps, poses = rc.trajectory(case.n_scans, inc=case.inc, start=case.start)
    rng = np.random.default_rng(case.seed)
    for s, (prev, cur, t_icp, u) in enumerate(steps):
        scan = orc.room_scan(poses[s], n_beams=case.beams, beam_delta_deg=360.0 / case.beams, walls=room_at(case, s), rng=rng,
                             range_max=case.range_max)
        if s in case.valid:
            nv = case.valid[s]
            if isinstance(nv, str):
                scan = _handmade(nv, case, poses[s], scan)
            else:
                keep = np.zeros(scan.size, dtype=bool)
                if isinstance(nv, dict):
                    for b, r in nv.items():
                        keep[b] = True; scan[b] = r
                elif nv:
                    keep[(np.arange(nv) * (scan.size // nv) + 7) % scan.size] = True
                scan = np.where(keep, scan, np.float32(0.01)).astype(np.float32)
        weights = None
        if case.resample_at == s:
            weights = np.full(case.N, 0.2 / case.N); weights[3] += 0.5; weights[case.N // 2] += 0.3; weights /= weights.sum()
        ok = case.icp[s]
        u = np.array(u, dtype=np.float64)
        if s in case.u_at:
            w, vx = case.u_at[s]
            u = np.array([w, u[1] if vx is None else vx, 0.0])
        normals = orc.normal_stream(900 + s, case.N * (3 * case.k + 3 if ok else 3) + 1, 0.0, 1.0)
        reset = np.tile(np.asarray(prev, dtype=np.float64), (case.N, 1)) if s in case.reset_at else None
        yield Scan(s, scan, u, cur, prev, np.asarray(t_icp), normals, ok, weights, reset)


def prepare(pf, sc, setter="set_particles"):
    """What a case does to a filter before a scan (either side: setter names the method)."""
    if sc.weights is not None:
        getattr(pf, setter)(w=sc.weights)
    if sc.reset_pose is not None:
        getattr(pf, setter)(pose=sc.reset_pose)


def n_valid(case, scan):
    return int(((scan >= np.float32(0.12)) & (scan < np.float32(case.range_max))).sum())
