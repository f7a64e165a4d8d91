"""The case table of the RBPF map update (csrc/rbpf_raycast.hip: the six instantiations of rbpf_raycast_box and the beam-ordered
rbpf_raycast) and the host's selection among them (csrc/rbpf_plan.hpp: plan_raycast, tile_cap_for), restated.  Plain data and host arithmetic, no device.
tests/test_raycast_cases.py proves on the CPU, with the oracle's GridMapper alone, that every case reaches what it names;
tests/test_raycast_gpu.py runs the table through tbnav_rbpf_integrate_scan_many and compares every particle's map with `==`.

A case: a map, a laser, Trs, N particles and a list of steps — a scan with one pose per particle (or a resample-style copy of
particles) — the forms it runs in, and what it claims to reach.  A form is a set of options; the kernel a form's launch is, and
the cells of its LDS array, follow from the restated selector (`select`) for every step.

Hand-made scans: range_min is 0.005 m, so a beam of 0.01 m is VALID and ends in the robot's own cell (a "zero-length" ray: no free
cell), 0.05 m from a cell centre ends in the neighbour, 0.11 m two cells on.  A range of 0 is invalid and thins the scan (Bv < n_beams);
beam indices in the kernel count the valid beams only.
"""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np

import oracle_api as orc

RES = 0.05                          # the shipped cell size, and the default of a case's `res`
RANGE_MIN = 0.005
ZERO_LEN = 0.01                     # a valid beam that ends in the robot's cell
kTS, kWave, kSl = 32, 64, 4
kBoxEv, kBoxEvFour, kHotSide, kHotMin, kVeryHot = 8, 4, 7, 16, 80
kMaxLds, kBoxStaticLds, kBoxSideMax, kMapTilesMax = 160 * 1024, 896, 176, 64

Step = namedtuple("Step", "scan poses mark gather")      # gather: parent of every particle (a resample's copies) INSTEAD of a scan
Case = namedtuple("Case", "id group map_min map_max range_max n_beams trs N steps forms opts claims res", defaults=(RES,))  # opts: options every form of the case gets on top of its own; res: the cell size

# ---- forms: the options a handle gets; warm = launches on spare particles first, so that the boxes' need is known at step 0 ----------
FORMS = {
    "box1024":     dict(opts=dict(THREADS=1024), warm=0),
    "box512w6":    dict(opts=dict(THREADS=512, ADAPT=0), warm=0),
    "box512w6c16": dict(opts=dict(THREADS=512, ADAPT=0, CELL16=2), warm=0),
    "box512w8":    dict(opts=dict(ADAPT=1), warm=2),
    "box512w8ev4": dict(opts=dict(ADAPT=3), warm=2),
    "box512w8c16": dict(opts=dict(ADAPT=1, CELL16=2), warm=2),
    "ordered":     dict(opts=dict(ORDERED=1), warm=0),
    "threads256":  dict(opts=dict(THREADS=256), warm=0),   # accepted, and selects the beam-ordered kernel (plan_raycast wants nt >= 512)
}
BOX_FORMS = ("box1024", "box512w6", "box512w6c16", "box512w8", "box512w8ev4", "box512w8c16")
ALL_FORMS = BOX_FORMS + ("ordered",)
# what the forms are FOR, when the box fits four workgroups per CU (small maps and rooms: every case but the ones that say otherwise)
FORM_KERNEL = {
    "box1024": "rbpf_raycast_box<1024, 8, false, 8>", "box512w6": "rbpf_raycast_box<512, 6, false, 8>",
    "box512w6c16": "rbpf_raycast_box<512, 6, true, 8>", "box512w8": "rbpf_raycast_box<512, 8, false, 8>",
    "box512w8ev4": "rbpf_raycast_box<512, 8, false, 4>", "box512w8c16": "rbpf_raycast_box<512, 8, true, 8>",
    "ordered": "rbpf_raycast", "threads256": "rbpf_raycast",
}
# combinations the selector cannot produce, and why (tests/test_raycast_cases.py checks that `select` never names them):
UNREACHABLE = {
    "rbpf_raycast_box<512, 6, false, 4>": "four-event slots exist only to fit FOUR workgroups per CU (wps 8)",
    "rbpf_raycast_box<512, 6, true, 4>": "the 16-bit form has eight-event slots only",
    "rbpf_raycast_box<512, 8, true, 4>": "the 16-bit form has eight-event slots only",
    "rbpf_raycast_box<1024, 8, true, 8>": "the 16-bit form is a 512-thread form",
    "rbpf_raycast_box<1024, 8, false, 4>": "four-event slots are a 512-thread form",
    "rbpf_raycast_box<256, *>": "THREADS = 256 falls through to rbpf_raycast",
}


# ---- plan_raycast's selection, restated (csrc/rbpf_plan.hpp; tests/test_rbpf_plan.py runs the C++ against this) ------------------------------------------------------------------------------
def box_lds_bytes(cap, bv, ev=kBoxEv):
    return 4 * cap + 2 * ev * bv + 8 * 64 + 4 * bv + 2 * ((bv + 1) & ~1)


def box16_hash_words(bv):
    h = 256
    while h < 2 * (bv + 64):
        h *= 2
    return h


def box16_lds_bytes(cap, bv, ev=kBoxEv):
    return box_lds_bytes(cap, bv, ev) - 2 * cap + 4 * box16_hash_words(bv)


def _trunc_div(a, b):
    return int(a / b) if a < 0 else a // b


def tile_cap_of(range_max, trs, ordered, res=RES):
    """create's rule (and TBNAV_RBPF_OPT_RAYCAST_ORDERED's; csrc/rbpf_plan.hpp: tile_cap_for): 0 = the box kernel is never used."""
    reach = float(np.float32(range_max)) + math.hypot(trs[1], trs[2])
    side = 2 * (int(math.ceil(reach / res)) + 2) + 1
    return side * side if (side * side <= 30000 and not ordered) else 0


def select(range_max, trs, opts, bv, rmax, need, res=RES):
    """(kernel name, cells of the LDS array or None) of one map-update launch: bv valid beams, the longest of them rmax metres,
    `need` = what the handle's mapped word holds (0: not known yet)."""
    tile_cap = tile_cap_of(range_max, trs, opts.get("ORDERED", 0), res)
    bvn = max(bv, 1)
    nt = opts.get("THREADS", 0)
    nt_auto = nt == 0
    if nt == 0:
        nt = 1024
    adapt, cell16, band_rows = opts.get("ADAPT", 1), opts.get("CELL16", 1), opts.get("BAND_ROWS", 0)
    cap_win = cap4 = 0
    if tile_cap > 0:
        reach = rmax + math.hypot(trs[1], trs[2])
        side = int(math.floor(2.0 * reach / res)) + 3
        least = (side + 9) & ~7
        cap_win = (side * ((side + 2) & ~1) + 7) & ~7
        cap_fit = _trunc_div(78 * 1024 - box_lds_bytes(0, bvn) - kBoxStaticLds, 4) & ~7
        if cap_win > cap_fit:
            cap_win = max(cap_fit, least)
        if band_rows > 0:
            cap_win = min(cap_win, (band_rows * ((side + 2) & ~1) + 7) & ~7)
        nd = need if adapt else 0
        if nd > 0:
            want = (nd + nd // 8 + 512 + 7) & ~7
            cap_win = min(cap_win, max(want, least))
            cap4 = max((nd + 256 + 7) & ~7, least)
    fits = lambda R, b: R * (b + kBoxStaticLds) <= kMaxLds        # noqa: E731
    may4 = adapt != 2 and cap4 > 0 and cap4 <= cap_win
    wps, c16, ev = 8, False, kBoxEv
    pick = nt_auto or nt == 512
    c16_ok = cell16 != 0 and 0 < cap_win < 65528 and bv + 64 < 32768
    force4 = adapt == 3
    if pick and may4 and not force4 and fits(4, box_lds_bytes(cap4, bvn, kBoxEv)):
        nt, cap_win = 512, cap4
    elif pick and may4 and fits(4, box_lds_bytes(cap4, bvn, kBoxEvFour)):
        nt, cap_win, ev = 512, cap4, kBoxEvFour
    elif pick and cap_win > 0 and fits(3, box_lds_bytes(cap_win, bvn)):
        nt, wps = 512, 6
    elif pick and may4 and c16_ok and fits(4, box16_lds_bytes(cap4, bvn, kBoxEv)):
        nt, cap_win, c16 = 512, cap4, True
    elif pick and c16_ok and fits(3, box16_lds_bytes(cap_win, bvn)):
        nt, wps, c16 = 512, 6, True
    elif nt == 512:
        wps = 6
    if cell16 == 2 and c16_ok and nt == 512:
        c16 = True
    if c16:
        ev = kBoxEv
    lds_win = box16_lds_bytes(cap_win, bvn, ev) if c16 else box_lds_bytes(cap_win, bvn, ev)
    if cap_win > 0 and bv < 32768 - kWave and nt >= 512 and lds_win <= kMaxLds - 4096:
        return f"rbpf_raycast_box<{512 if nt == 512 else 1024}, {wps}, {'true' if c16 else 'false'}, {ev}>", cap_win
    return "rbpf_raycast", None


def kernel_shape(name):
    """(threads, events a slot) of a box instantiation's name."""
    nt, _, _, ev = name[len("rbpf_raycast_box<"):-1].split(", ")
    return int(nt), int(ev)


def segments(nt, bv):
    return min(4, max(1, nt // bv)) if bv > 0 else 1


def box_of(ends, robot, cells):
    """The kernel's bounding box of one particle: (minx, miny, bh, bw) from its end-point cells and the robot's (row-major indices)."""
    idx = np.append(np.asarray(ends, dtype=np.int64), robot)
    cx, cy = idx // cells, idx % cells
    minx, maxx, miny, maxy = int(cx.min()), int(cx.max()), int(cy.min()) & ~1, int(cy.max())
    return minx, miny, maxx - minx + 1, ((maxy | 1) + 1) - miny


def bands_of(box, cap):
    minx, _, bh, bw = box
    rows_fit = cap // bw
    return [(x0, min(rows_fit, minx + bh - x0)) for x0 in range(minx, minx + bh, rows_fit)]


class Need:
    """The boxes' need as the host sees it: a box launch reports max(bh * bw) over its workgroups 1, 17, 33, ...; the host reads it
    two box launches later (launch j hands launch j - 1's maximum over, and the host reads the word before it launches)."""

    def __init__(self):
        self.reports = []

    def seen(self):
        return self.reports[-2] if len(self.reports) >= 2 else 0

    def launched(self, boxes):
        rep = [b[2] * b[3] for i, b in enumerate(boxes) if (i & 15) == 1]
        self.reports.append(max(rep) if rep else None)       # (None: fewer than two workgroups — nothing reported, nothing handed over)


# ---- the world ---------------------------------------------------------------------------------------------------------------------------
def cells_of(case):
    return int(math.ceil((case.map_max - case.map_min) / case.res))


def laser_of(case):
    d2r = np.pi / 180.0
    return np.array([0.0, 360.0 * d2r, (360.0 / case.n_beams) * d2r, RANGE_MIN, case.range_max], dtype=np.float32)


def grid_of(case):
    return (case.res, case.map_min, case.map_max, case.map_min, case.map_max)


def oracle_grid(case):
    return orc.GridAPI("orc", grid=grid_of(case), laser=laser_of(case), trs=case.trs)


def device_params(case, n_particles):
    """Keyword arguments of rtn_amd.rbpf.default_params."""
    return dict(N=n_particles, k=2, map_min=case.map_min, map_max=case.map_max, beam_delta_deg=360.0 / case.n_beams,
                range_min=RANGE_MIN, range_max=case.range_max, Trs=list(case.trs), resolution=case.res)


def centre(case, i, j, off=(0.001, 0.001)):
    return case_xy(case.map_min, i, j, off, case.res)


def case_xy(map_min, i, j, off=(0.001, 0.001), res=RES):
    return map_min + (i + 0.5) * res + off[0], map_min + (j + 0.5) * res + off[1]


def shifts(N, kind="spread"):
    """Cell shifts per particle: every alignment of the box against the 32-cell tiles and the even-column padding."""
    if kind == "diag":
        return [(p, 31 - p) for p in range(N)]
    if kind == "none":
        return [(0, 0)] * N
    return [((11 * p) % 32, (7 * p + 5) % 32) for p in range(N)]


def poses_at(map_min, base, sh, thetas=None, res=RES):
    out = []
    for p, (a, b) in enumerate(sh):
        x, y = case_xy(map_min, base[0] + a, base[1] + b, res=res)
        out.append(((thetas[p] if thetas is not None else 0.0), x, y))
    return np.array(out)


def beam_at(n_beams, deg):
    return int(round(deg / (360.0 / n_beams))) % n_beams


LONG_DEG, LONG_RANGE = 225.0, 0.8


def hand(n_beams, ranges, fill=ZERO_LEN, long=True):
    """A hand-made scan: beam -> range in metres; every other beam `fill` (ZERO_LEN: valid, ends in the robot's cell; 0: invalid).
    long: one beam of 0.8 m down the diagonal at 225 degrees, away from every target cell — the host bounds the LDS array by the
    scan's longest beam, and without it the array of a hand-made scan is smaller than need + 256: no four-per-CU form."""
    s = np.full(n_beams, fill, dtype=np.float32)
    if long:
        s[beam_at(n_beams, LONG_DEG)] = LONG_RANGE
    for b, r in ranges.items():
        s[b % n_beams] = r
    return s


def thin(scan, bv):
    """Exactly bv of the scan's beams stay valid, spread round the scan."""
    keep = np.zeros(scan.size, dtype=bool)
    keep[np.unique(np.round(np.linspace(0, scan.size - 1, bv)).astype(int))] = True
    assert keep.sum() == bv
    return np.where(keep, scan, np.float32(0.0)).astype(np.float32)


def room(n_beams, walls=(-0.62, 0.57, -0.48, 0.66), seed=1, range_max=3.5):
    return orc.room_scan((0.0, 0.0, 0.0), n_beams=n_beams, beam_delta_deg=360.0 / n_beams, walls=walls, rng=np.random.default_rng(seed),
                         range_max=range_max)


def _case(id, group, steps, N=18, half=2.0, map_max=None, range_max=3.5, n_beams=360, trs=(0.0, 0.0, 0.0), forms=ALL_FORMS, opts=None,
          claims=None, mark_all=False, res=RES):
    steps = tuple(s if isinstance(s, Step) else Step(s[0], np.asarray(s[1], dtype=np.float64), mark_all, None) for s in steps)
    steps = steps[:-1] + (steps[-1]._replace(mark=True),)
    return Case(id, group, -half, half if map_max is None else map_max, range_max, n_beams, tuple(trs), N, steps, tuple(forms),
                dict(opts or {}), claims or {}, res)


BASE = (24, 24)          # the robot's cell before the shifts, on the 80-cell map: shifts of up to 31 cells and 18 cells of reach stay inside
N_HAND = 1440            # beams of the hand-made scans: 0.25 degrees apart


def _thetas(N):
    return [0.17 * p for p in range(N)]


def _room_case(id, group, n_beams=360, bv=None, N=18, forms=ALL_FORMS, repeats=2, claims=None, **kw):
    sc = room(n_beams)
    if bv is not None:
        sc = thin(sc, bv)
    po = poses_at(-2.0, BASE, shifts(N), _thetas(N))
    cl = dict(claims or {})
    if bv is not None:
        cl["bv"] = bv
    return _case(id, group, [(sc, po)] * repeats, N=N, n_beams=n_beams, forms=forms, claims=cl, **kw)


def _hand_case(id, group, scans, N=18, forms=ALL_FORMS, claims=None, sh="spread", n_beams=N_HAND, **kw):
    po = poses_at(-2.0, BASE, shifts(N, sh))
    return _case(id, group, [(s, po) for s in scans], N=N, n_beams=n_beams, forms=forms, claims=claims, mark_all=True, **kw)


# the target cell of the slot cases is T = robot + (0, 1) (beams round 90 degrees); F = robot + (0, 2) is where a 0.11 m beam ends
B90 = beam_at(N_HAND, 90.0)
R_END, R_THROUGH = 1.0 * RES, 2.2 * RES           # one cell / 2.2 cells (0.05 and 0.11 m, the same float32 ranges)


# ends (e) and frees (f) in beam order: sequences whose reversal gives other float64 bits from the prior value _prior_scan leaves
# (tests/test_raycast_cases.py checks that); plain alternation of an odd count is a palindrome
EVENT_PATTERNS = {3: "eff", 4: "efef", 5: "efeff", 7: "efefeff", 8: "efefefef", 9: "efefefeff"}


def _events_scan(k, first=None):
    """k consecutive beams round 90 degrees, ending in T (e) or passing through it (f): T takes exactly k events."""
    first = B90 - k // 2 if first is None else first
    return hand(N_HAND, {first + i: (R_END if kind == "e" else R_THROUGH) for i, kind in enumerate(EVENT_PATTERNS[k])})


def _prior_scan():
    """One beam through T and one ending there: a prior value of T from which the order of later adds shows in the bits."""
    return hand(N_HAND, {B90: R_THROUGH, B90 + 1: R_THROUGH, B90 + 2: R_END})


def _hot_scan(k, end_too=False, fill=0.0):
    """k consecutive beams round 90 degrees pass through T and end in F: T takes k free adds and no end point (unless end_too: one
    more beam ends in T).  fill = 0: the other beams are invalid, so the robot's own cell is no end point either."""
    d = {B90 - k // 2 + i: R_THROUGH for i in range(k)}
    if end_too:
        d[B90 - k // 2 + k] = R_END
    return hand(N_HAND, d, fill=fill)


def _arc_scan(n, r=0.52, first=0, fill=ZERO_LEN):
    d = {first + i: r for i in range(n)}
    d[beam_at(N_HAND, 330.0)] = LONG_RANGE            # (the long beam, outside the arc)
    return hand(N_HAND, d, fill=fill, long=False)


def _fan(n_beams, lo_deg, hi_deg, r, fill=0.0, seed=3):
    rng = np.random.default_rng(seed)
    lo, hi = beam_at(n_beams, lo_deg), beam_at(n_beams, hi_deg)
    return hand(n_beams, {b: r + 0.2 * rng.random() for b in range(lo, hi + 1)}, fill=fill, long=False)


def _build():
    cs = []
    N = 18
    # ---- bv: alignments, map edges, the sensor offset, ragged scans ----------------------------------------------------------------------
    sc = room(360)
    cs.append(_case("align", "bv", [(sc, poses_at(-2.0, BASE, shifts(32, "diag"), _thetas(32)))] * 2, N=32))
    # the map's last column: the particles in column 77 look at a wall in column 79 — the box's last cell PAIR (78, 79) is the map's.
    # (An odd-sided map, where that pair would stick out of the map, cannot be made: create refuses an odd side with
    #  TBNAV_ERR_UNSUPPORTED — tests/test_raycast_gpu.py pins that.)
    po = np.array([(0.0,) + case_xy(-2.0, 20 + 2 * p + (p & 1), 77) for p in range(N)])
    cs.append(_case("map_edge_last_pair", "bv", [(room(360, walls=(-0.4, 0.4, -0.4, 0.09), seed=2), po)] * 2, claims=dict(last_column=79)))
    # the robot in the four corner cells (and next to them), a 90-degree fan that stays inside
    corner, cpo = [], []
    for p in range(N):
        q, d = p % 4, p // 4
        i, j = (d if q in (0, 1) else 79 - d), (d if q in (0, 2) else 79 - d)
        cpo.append((0.0,) + case_xy(-2.0, i, j))
        corner.append((i, j))
    # one scan for all: beams in every quadrant would leave the map, so every particle turns its fan inwards by its heading
    fan = _fan(360, 5.0, 85.0, 0.5, fill=ZERO_LEN)
    heads = {0: 0.0, 1: -math.pi / 2, 2: math.pi / 2, 3: math.pi}
    cpo = np.array([(heads[p % 4], x, y) for p, (_, x, y) in enumerate(cpo)])
    cs.append(_case("corner", "bv", [(fan, cpo)] * 2, claims=dict(corners=((0, 0), (0, 79), (79, 0), (79, 79)))))
    cs.append(_room_case("sensor_offset", "bv", trs=(0.3, 0.05, -0.02)))
    for bv in (1, 2, 63, 64, 65, 127, 128, 129, 170, 171, 255, 256, 257, 341, 342, 511, 512, 513, 1023, 1024, 1025):
        cs.append(_room_case(f"bv_{bv}", "bv", n_beams=1080, bv=bv))
    # the LDS limit of the box kernel: the largest Bv its layout takes, and one beam more (the beam-ordered kernel)
    rmax_room = float(room(360).max())
    last = max(b for b in range(6000, 8000) if select(3.5, (0, 0, 0), dict(THREADS=1024), b, rmax_room, 0)[1] is not None)
    sc = room(last + 1)
    cs.append(_case("bv_lds_last", "bv", [(thin(sc, last), poses_at(-2.0, BASE, shifts(N), _thetas(N)))], n_beams=last + 1,
                    forms=("box1024", "box512w6", "box512w6c16", "ordered"), claims=dict(bv=last, box=True)))
    cs.append(_case("bv_lds_first_ordered", "bv", [(sc, poses_at(-2.0, BASE, shifts(N), _thetas(N)))], n_beams=last + 1,
                    forms=("box1024", "box512w6"), claims=dict(bv=last + 1, box=False)))
    cs.append(_hand_case("all_zero_length", "bv", [hand(N_HAND, {}, long=False)] * 2, claims=dict(zero_length=N_HAND)))
    cs.append(_hand_case("zero_length_but_one", "bv", [hand(N_HAND, {B90 + 33: 0.31}, long=False)] * 2, claims=dict(zero_length=N_HAND - 1)))
    cs.append(_room_case("threads_256", "bv", forms=("threads256",)))
    # ---- slots -----------------------------------------------------------------------------------------------------------------------------
    # stray: beams 80 apart end in T, one more passes through it, every beam between ends in the robot's cell
    stray = hand(N_HAND, {B90 - 40: R_END, B90 + 40: R_END, B90 + 41: R_THROUGH, B90 - 39: R_THROUGH})
    cs.append(_hand_case("stray", "slots", [_prior_scan(), stray], claims=dict(order=True, stray=True, events=4)))
    # wrap: T = robot + (1, 0), the slot's events come from beams Bv - 2, Bv - 1, 0, 1
    # (in the reference's order — beams 0, 1, Bv - 2, Bv - 1 — the kinds are f f e e: walking the mask's two halves the other way round
    #  gives e e f f, other bits; an alternating e f e f would read the same either way)
    wrap = hand(N_HAND, {N_HAND - 2: R_END, N_HAND - 1: R_END, 0: R_THROUGH, 1: R_THROUGH})
    wprior = hand(N_HAND, {0: R_THROUGH, 1: R_THROUGH, 2: R_END})
    cs.append(_hand_case("wrap", "slots", [wprior, wrap], claims=dict(order=True, wrap=(N_HAND - 2, N_HAND - 1, 0, 1), events=4, target=(1, 0))))
    for k in (3, 4, 5, 7, 8, 9):
        cs.append(_hand_case(f"events_{k}", "slots", [_prior_scan(), _events_scan(k)], claims=dict(order=True, events=k)))
    # the robot's own cell as an end point of FEWER beams than a slot holds (the zero-length fill of the other cases overflows its slot
    # anyway): two zero-length beams among five rays that start there — the slot lists two events, the cell takes seven, so the kernel
    # must send it to the exhaustive replay whatever its count says
    own = hand(N_HAND, {100: 0.3, 200: ZERO_LEN, 300: 0.3, 400: ZERO_LEN, 500: 0.3, 600: 0.3}, fill=0.0)
    cs.append(_hand_case("robot_cell_endpoint", "slots", [own, own], claims=dict(order=True, robot_ends=2, robot_frees=5)))
    # overflowed slots: an arc of beams at 0.52 m (17 beams per cell of the ring) over zero-length beams, whose slot — the robot's own
    # cell — overflows too; the arcs' lengths were found by growing them beam by beam on the oracle's geometry, the CPU test counts
    for name, (n_arc, n_ovf) in OVERFLOW_ARCS.items():
        cs.append(_hand_case(name, "slots", [_arc_scan(n_arc)] * 2, claims=dict(order=True, overflow=n_ovf)))
    # ---- hot cells -------------------------------------------------------------------------------------------------------------------------
    for k in (15, 16, 79, 80):
        cs.append(_hand_case(f"hot_{k}", "hot", [_prior_scan(), _hot_scan(k)], claims=dict(hot=k)))
    cs.append(_hand_case("hot_is_endpoint", "hot", [_prior_scan(), _hot_scan(30, end_too=True)], claims=dict(hot=30, hot_end=True)))
    cs.append(_hand_case("hot_window_leaves_box", "hot", [_fan(N_HAND, 0.0, 90.0, 0.4)] * 2, claims=dict(window_leaves_box=True)))
    # ---- bands -----------------------------------------------------------------------------------------------------------------------------
    # by themselves: range_max 4.2 m is the longest create gives the box kernel (side 173), an open scan's box exceeds the 78 KB array
    rng = np.random.default_rng(4)
    open_scan = (4.0 + 0.15 * rng.random(360)).astype(np.float32)
    po = np.array([(0.1 * p,) + case_xy(-5.0, 100 + (5 * p) % 13, 100 + (7 * p) % 12) for p in range(N)])
    cs.append(_case("bands_natural_4p2m", "bands", [(open_scan, po)] * 2, half=5.0, range_max=4.2, claims=dict(bands=2)))
    for rows in (1, 3, 4, 5):
        cs.append(_room_case(f"band_rows_{rows}", "bands", opts=dict(BAND_ROWS=rows), claims=dict(band_rows=rows)))
    # the robot's row in the LAST band: a fan that looks towards -x only (the other beams invalid: the robot's cell is no end point)
    cs.append(_hand_case("robot_in_last_band", "bands", [_fan(N_HAND, 120.0, 240.0, 0.5)] * 2, opts=dict(BAND_ROWS=4),
                         claims=dict(robot_last_band=True)))
    # a box that outgrows the need two launches back takes a second band: the only bands of the four-per-CU instantiations
    # (BAND_ROWS caps the array below need + 256, which rules them out)
    small, big = room(360, walls=(-0.31, 0.28, -0.24, 0.33), seed=5), room(360)
    po = poses_at(-2.0, BASE, shifts(N), _thetas(N))
    cs.append(_case("bands_outgrown", "bands", [(small, po), (small, po), (big, po), (big, po)], claims=dict(outgrown_at=(2, 3))))
    # ---- copy-on-write across bands ------------------------------------------------------------------------------------------------------
    parents = [p - (p & 1) for p in range(N)]                      # every odd particle becomes a copy of its even neighbour
    po2 = poses_at(-2.0, BASE, [(a + (p & 1), b + 2 * (p & 1)) for p, (a, b) in enumerate(shifts(N))], [0.17 * p + 0.4 * (p & 1) for p in range(N)])
    cs.append(_case("cow_across_bands", "cow", [(big, po), Step(None, None, True, tuple(parents)), (big, po2), (big, po2)], opts=dict(BAND_ROWS=3),
                    claims=dict(tile_in_bands=3)))
    cs.append(_case("cow_outgrown", "cow", [(small, po), (small, po), Step(None, None, False, tuple(parents)), (big, po2), (big, po2)],
                    claims=dict(outgrown_at=(3, 4))))
    # ---- the occupancy bits, per writer ----------------------------------------------------------------------------------------------------
    b0, b180, b270, b45 = 0, beam_at(N_HAND, 180.0), beam_at(N_HAND, 270.0), beam_at(N_HAND, 45.0)
    up = {B90: R_END, b0: R_END, b270: R_END}
    up.update({b180 - 4 + i: (R_END if i % 3 == 0 else R_THROUGH) for i in range(9)})       # 3 ends + 6 frees in robot + (-1, 0)
    up.update({b45 + i: ZERO_LEN for i in range(9)})                                        # the robot's cell: 9 ends against 12 frees
    down = {B90 - 10 + i: R_THROUGH for i in range(20)}                                     # hot: 20 frees through robot + (0, 1)
    down[b0] = R_THROUGH                                                                    # plain: one free add in robot + (1, 0)
    down.update({b270 - 2 + i: (R_END if i == 1 else R_THROUGH) for i in range(5)})         # 3a (3b with four-event slots): 1 end + 4 frees
    down.update({b180 - 4 + i: (R_END if i == 2 else R_THROUGH) for i in range(9)})         # 3b: 1 end + 8 frees
    cs.append(_hand_case("toggle_each_writer", "toggle", [hand(N_HAND, up, fill=0.0), hand(N_HAND, down, fill=0.0)],
                         claims=dict(order=True, toggles=True)))
    return cs + _res_cases()


# ---- other cell sizes (group `res`) ----------------------------------------------------------------------------------------------------------
# res -> why (create admits every cell size whose brushfire radius ceil(10 / res) is at most 254; every map here is +-2.0 m: 102, 64, 58,
# 14 and 8 cells a side, all even)
RES_TABLE = {
    0.0394: "finest admitted (radius 254); 1 / res is no double; the last cell is ragged (101.52 cells); range_max 3.5 -> tile cap 0",
    0.0625: "dyadic: 1 / res = 16 and every cell border are exact doubles",
    0.07: "1 / res is no double; ragged (57.14 cells); radius 143",
    0.3: "coarse; 1 / res is no double; ragged (13.33 cells); radius 34",
    0.5: "coarsest useful: radius 20 covers the map; 8 cells a side (12 with +-3.0 m)",
}
RAGGED = (0.0394, 0.07, 0.3)
TRS_OFFSET = (0.3, 0.05, -0.02)          # sensor_offset's


# What a 360-beam room scan reaches BY ITSELF on a coarse map, counted per particle and step by tests/test_raycast_cases.py with `events`
# ((least, most) over the particles): end-point cells past kBoxEv events, cells that hold no end point with >= kHotMin / >= kVeryHot free adds,
# those of them outside the 7 x 7 window, and slots replayed exhaustively (more than kBoxEv events, or the robot's cell).
# What these geometries CANNOT produce: with walls at most 0.66 m off, every cell a ray crosses is within 3 cells of the robot at 0.3 m
# (no hot cell outside the window: res_0p3_wide_20 has them) and holds an end point itself at 0.5 m (no hot cell at all); and a map of
# 14 x 14 or 8 x 8 cells has fewer end-point cells than the kWave = 64 slots of the overflow list (overflow_64 / _65 fill it at 0.05 m).
COARSE_COUNTS = {
    "res_0p3_room": dict(count_past_ev=(14, 17), count_hot=(5, 8), count_very_hot=(0, 2), count_hot_outside=(0, 0), count_overflowed=(14, 17)),
    "res_0p3_trs": dict(count_past_ev=(15, 18), count_hot=(4, 7), count_very_hot=(0, 2), count_hot_outside=(0, 0), count_overflowed=(15, 18)),
    "res_0p5_room": dict(count_past_ev=(8, 10), count_hot=(0, 0), count_very_hot=(0, 0), count_hot_outside=(0, 0), count_overflowed=(8, 10)),
    "res_0p5_trs": dict(count_past_ev=(8, 10), count_hot=(0, 0), count_very_hot=(0, 0), count_hot_outside=(0, 0), count_overflowed=(8, 10)),
    "res_0p5_room_12": dict(count_past_ev=(8, 10), count_hot=(0, 0), count_very_hot=(0, 0), count_hot_outside=(0, 0), count_overflowed=(8, 10)),
    "res_0p3_wide_20": dict(count_past_ev=(15, 27), count_hot=(39, 46), count_very_hot=(0, 0), count_hot_outside=(4, 12), count_overflowed=(15, 27)),
}


def res_tag(res):
    return repr(res).replace(".", "p")


def _res_poses(res, N, half=2.0):
    """align's poses at another cell size: cell-centre poses (+ 1 mm) shifted in whole cells over about the same 1.55 m and turned."""
    span = max(2, min(32, int(1.55 / res)))
    base = int(round((half - 0.775) / res - 0.5))
    sh = [((11 * p) % span, (7 * p + 5) % span) for p in range(N)]
    return poses_at(-half, (base, base), sh, _thetas(N), res=res)


def _along(res, cells, half, d, upper):
    """A coordinate `d` steps in from a map border: on the border itself, in the middle of the border's cell (the ragged last cell's own middle), then cell centres + 1 mm."""
    if d == 0:
        return half if upper else -half
    i = cells - d if upper else d - 1
    lo, hi = -half + i * res, min(half, -half + (i + 1) * res)
    return 0.5 * (lo + hi) + (0.001 if d >= 2 else 0.0)


def reciprocal_traps(res, half=2.0):
    """Coordinates on (or one ulp beside) a cell border at which the reciprocal product floors to another cell than the reference's
    division: floor(fl(d * fl(1 / res))) != floor(fl(d / res)) with d = fl(x + half).  cell_floor (csrc/rbpf_device.hpp) forms the product
    first and must fall back to the division there; a cell size whose reciprocal is a double has none."""
    inv, out = 1.0 / res, []
    for i in range(1, int(math.ceil(2 * half / res))):
        for x in (np.nextafter(-half + i * res, -np.inf), -half + i * res, np.nextafter(-half + i * res, np.inf)):
            d = float(x) + half
            if -half <= x <= half and math.floor(d * inv) != math.floor(d / res):
                out.append(float(x))
    return out


def _res_cases():
    cs, N, half = [], 18, 2.0
    for res in RES_TABLE:
        tag, cells = res_tag(res), int(math.ceil(2 * half / res))
        sc, po = room(360), _res_poses(res, N)
        why = dict(res=res, cells=cells)
        cs.append(_case(f"res_{tag}_room", "res", [(sc, po)] * 2, res=res, claims=dict(why, **COARSE_COUNTS.get(f"res_{tag}_room", {}))))
        cs.append(_case(f"res_{tag}_trs", "res", [(sc, po)] * 2, res=res, trs=TRS_OFFSET, claims=dict(why, **COARSE_COUNTS.get(f"res_{tag}_trs", {}))))
        if res not in RAGGED:
            continue
        # corner: the robot ON the map's four corners (xmin / xmax themselves), in the corner cells — the upper ones ragged — and next to
        # them; the fan turned inwards; the other beams invalid (a zero-length beam from a border pose would leave the world)
        fan = _fan(360, 5.0, 85.0, 0.5, fill=0.0)
        heads = {0: 0.0, 1: -math.pi / 2, 2: math.pi / 2, 3: math.pi}
        cpo = np.array([(heads[p % 4], _along(res, cells, half, p // 4, p % 4 in (2, 3)), _along(res, cells, half, p // 4, p % 4 in (1, 3))) for p in range(N)])
        cs.append(_case(f"res_{tag}_corner", "res", [(fan, cpo)] * 2, res=res, claims=dict(why, on_corner=4, in_ragged_cell=True)))
        # edge: the robot in the map's last, partial column — on ymax itself (even particles) or in the column's middle — looking back into the map
        back = _fan(360, 20.0, 160.0, 0.5, fill=0.0, seed=6)
        epo = np.array([(math.pi + 0.02 * (p - 9), -1.2 + 2.4 * p / (N - 1), _along(res, cells, half, p & 1, True)) for p in range(N)])
        cs.append(_case(f"res_{tag}_edge", "res", [(back, epo)] * 2, res=res, claims=dict(why, last_column=cells - 1)))
    # the robot ON cell borders where the product with fl(1 / res) and the division disagree about the cell (reciprocal_traps): x, y or both;
    # a small room round it (0.0394 m with range_max 3.3, so that the box kernels run as well)
    for res, rmax in ((0.0394, 3.3), (0.07, 3.5)):
        traps = [t for t in reciprocal_traps(res) if abs(t) <= 1.6]
        mid = [case_xy(-half, int((0.8 + 0.13 * p) / res), 0, res=res)[0] for p in range(N)]      # cell centres (+ 1 mm) between -1.2 and 1.0 m
        tpo = np.array([(0.17 * p, traps[p % len(traps)] if p % 3 != 1 else mid[p], traps[(5 * p + 1) % len(traps)] if p % 3 != 0 else mid[p]) for p in range(N)])
        cs.append(_case(f"res_{res_tag(res)}_lattice", "res", [(room(360, walls=(-0.31, 0.28, -0.24, 0.33), seed=5, range_max=rmax), tpo)] * 2, res=res,
                        range_max=rmax, claims=dict(res=res, cells=int(math.ceil(2 * half / res)), traps=len(traps))))
    cs.append(_case("res_0p5_room_12", "res", [(room(360), _res_poses(0.5, N, 3.0))] * 2, half=3.0, res=0.5,
                    claims=dict(res=0.5, cells=12, **COARSE_COUNTS["res_0p5_room_12"])))
    # a room whose walls are six cells off at 0.3 m (+-3.0 m: 20 cells): what the small room cannot give a coarse map — hot cells OUTSIDE the 7 x 7 window
    wide = room(360, walls=(-1.9, 1.8, -1.7, 1.85), seed=8)
    wpo = poses_at(-3.0, (9, 9), [((11 * p) % 3, (7 * p + 5) % 3) for p in range(N)], _thetas(N), res=0.3)
    cs.append(_case("res_0p3_wide_20", "res", [(wide, wpo)] * 2, half=3.0, res=0.3, claims=dict(res=0.3, cells=20, **COARSE_COUNTS["res_0p3_wide_20"])))
    # the largest box the tile-cap rule admits: range_max 3.3 at 0.0394 m is side 173 (cap 29929), 3.5 (the two cases above) side 183 -> 0
    cs.append(_case("res_0p0394_room_3p3", "res", [(room(360, range_max=3.3), _res_poses(0.0394, N))] * 2, res=0.0394, range_max=3.3,
                    claims=dict(res=0.0394, cells=102, tile_cap=173 * 173)))
    # exact borders at 0.0625 m.  BORDER_MIN-style distances do not apply: this case is ABOUT end points and sensors on borders, and it may
    # be, because here a border is decided exactly on both sides — theta = 0, Trs = 0, beam 0 runs along +x with cos = 1 and sin = 0
    # exactly, the range is a float32 multiple of res and the sensor sits on lattice points, so x + r and y are doubles without rounding
    # and d / res (a division by a power of two) is the exact quotient: no arithmetic on either side can put the point elsewhere.
    # Step 0: beam 0 = 8 cells (0.5 m) from lattice points, one of them 8 cells before the map's upper corner (the END POINT is the corner:
    # the clamp binds for both indices), two more beams (300 and 330 degrees) end inside cells.  Step 1: the sensor on lattice points again, one
    # of them the map's upper corner (the clamp binds for the robot's cell), beam 0 invalid, a fan into the third quadrant.
    lat = lambda i, j: (0.0, -half + i * 0.0625, -half + j * 0.0625)       # noqa: E731
    s0 = hand(360, {0: 8 * 0.0625, 300: 0.33, 330: 0.41}, fill=0.0, long=False)
    p0 = np.array([lat(56, 64), lat(56, 63), lat(55, 64), lat(0, 8), lat(1, 8), lat(32, 32), lat(31, 33)] + [lat(8 + 2 * p, 40 - p) for p in range(N - 7)])
    s1 = _fan(360, 185.0, 265.0, 0.5, fill=0.0, seed=7)
    p1 = np.array([lat(64, 64), lat(64, 63), lat(63, 64), lat(32, 32)] + [lat(20 + 2 * p, 50 - p) for p in range(N - 4)])
    cs.append(_case("res_0p0625_borders", "res", [(s0, p0), (s1, p1)], res=0.0625, mark_all=True,
                    claims=dict(res=0.0625, cells=64, border_beam=0, border_cells=8, end_on_corner=0, robot_on_corner=0)))
    return cs


# case -> (beams of the arc, overflowed slots with (eight-event, four-event) slots)
OVERFLOW_ARCS = {"overflow_64_ev4": (1138, (63, 64)), "overflow_64": (1150, (64, 65)), "overflow_65": (1170, (65, 66))}


@lru_cache(maxsize=None)
def cases():
    cs = _build()
    assert len({c.id for c in cs}) == len(cs)
    return tuple(cs)


def case(cid):
    return {c.id: c for c in cases()}[cid]


def form_opts(c, form):
    o = dict(FORMS[form]["opts"])
    o.update(c.opts)
    return o


# ---- the geometry of a step, from the oracle's GridMapper ----------------------------------------------------------------------------------
def geometry(g, scan, pose):
    """(end points [Bv][2], their cells, the robot's cell) of a scan integrated at pose: row-major cell indices i * xsize + j."""
    pts = g.end_points(scan, pose)
    ends = np.array([g.world2rowmajor(x, y) for x, y in pts], dtype=np.int64)
    return pts, ends, g.world2rowmajor(pose[1], pose[2])


def events(g, pts, ends, pose):
    """cell -> [(beam, kind)] in the reference's order of adds (grid_mapper.cpp:153-177): beam by beam, the ray's free cells (kind 0),
    then its end point (kind 1).  Beams count the VALID beams, as the kernel's do."""
    ev = {}
    for b in range(len(ends)):
        for q in g.free_index(pts[b], pose):
            ev.setdefault(int(q), []).append((b, 0))
        ev.setdefault(int(ends[b]), []).append((b, 1))
    return ev


def replay(v, evs, d_free, d_occ):
    for _, kind in evs:
        v = v + (d_occ if kind else d_free)
    return v


def scan_stats(scan, range_max):
    """(Bv, the longest valid range as the host sees it) of a scan."""
    s = np.asarray(scan, dtype=np.float32)
    ok = (s >= np.float32(RANGE_MIN)) & (s < np.float32(range_max))
    return int(ok.sum()), (float(s[ok].max()) if ok.any() else 0.0)


def plan(c, form, boxes_of_step):
    """Per step of the case in this form: (kernel name, cells of the LDS array or None, need the launch saw) — None for a copy step.
    boxes_of_step[s] = the particles' boxes at step s (box_of).  Warm-up launches (FORMS[form]['warm']) repeat step 0 on spare particles."""
    need, opts, out = Need(), form_opts(c, form), []
    first = next(s for s, st in enumerate(c.steps) if st.scan is not None)
    launches = [first] * FORMS[form]["warm"] + list(range(len(c.steps)))
    for n, s in enumerate(launches):
        st = c.steps[s]
        if st.scan is None:
            out.append(None)
            continue
        bv, rmax = scan_stats(st.scan, c.range_max)
        seen = need.seen() or 0
        name, cap = select(c.range_max, c.trs, opts, bv, rmax, seen, c.res)
        if cap is not None:
            need.launched(boxes_of_step[s])
        if n >= FORMS[form]["warm"]:
            out.append((name, cap, seen if opts.get("ADAPT", 1) else 0))
    return out


# ---- the oracle's run of a case ------------------------------------------------------------------------------------------------------------
def event_particles(c):
    """Particles whose per-cell events the CPU test works out: all of a hand-made case (its claims must hold for every particle),
    the first and the last of a room case (where they only check the restatement against the oracle)."""
    if c.n_beams == N_HAND or (c.group == "res" and cells_of(c) <= 20):      # (the coarse maps: the claims count events for every particle)
        return tuple(range(c.N))
    return (0,) if c.n_beams > 2000 else (0, c.N - 1)


@lru_cache(maxsize=None)
def reference(cid, with_events=False):
    """The case on the oracle's GridMapper, one per particle (no brushfire).  Per step a dict: rc (statuses), boxes, robots, ends (per
    particle; None for a copy step), maps (at a marked step: per particle (log-odds, sorted occupied cells, exported map)), and with
    with_events, for event_particles: events, before / after (log-odds), occ_before / occ_after (sets)."""
    c = case(cid)
    cells = cells_of(c)
    g0 = oracle_grid(c)
    assert (g0.xsize, g0.ysize) == (cells, cells), (cid, g0.xsize, cells)
    k = g0.constants()
    grids = [g0.clone() for _ in range(c.N)]
    out = []
    for st in c.steps:
        rec = dict(rc=None, boxes=None, robots=None, ends=None, maps=None, ev={})
        if st.scan is None:
            new = [grids[par].clone() for par in st.gather]
            for g in grids:
                g.close()
            grids = new
        else:
            rec.update(rc=[], boxes=[], robots=[], ends=[])
            for p in range(c.N):
                g, pose = grids[p], st.poses[p]
                pts, ends, robot = geometry(g, st.scan, pose)
                rec["robots"].append(robot); rec["ends"].append(ends)
                rec["boxes"].append(box_of(ends, robot, cells) if (robot >= 0 and (ends >= 0).all()) else None)
                e = None
                if with_events and p in event_particles(c):
                    e = dict(events=events(g, pts, ends, pose), before=g.dump()["log_odds"].copy(), occ_before=set(g.occ_cells().tolist()))
                rec["rc"].append(g.integrate_scan(st.scan, pose, esdf=False))
                if e is not None:
                    e.update(after=g.dump()["log_odds"].copy(), occ_after=set(g.occ_cells().tolist()))
                    rec["ev"][p] = e
        if st.mark:
            rec["maps"] = [(g.dump()["log_odds"].copy(), np.sort(g.occ_cells()), g.grid_map().copy()) for g in grids]
        out.append(rec)
    for g in grids:
        g.close()
    g0.close()
    return dict(steps=out, d_free=k[2] - k[0], d_occ=k[1] - k[0], cells=cells)


def plans(cid):
    """form -> plan(...) of the case, from the oracle's boxes."""
    c = case(cid)
    ref = reference(cid)
    boxes = [r["boxes"] for r in ref["steps"]]
    return {f: plan(c, f, boxes) for f in c.forms}
