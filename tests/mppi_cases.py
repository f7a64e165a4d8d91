"""The MPPI kernels' instantiations as a table of cases, used by the CPU tests (tests/test_mppi_cases.py) and the GPU tests
(tests/test_mppi_instantiations_gpu.py, tests/test_mppi_combine_gpu.py) alike.

A case is plain data: the options to set on a fresh handle (names of TBNAV_MPPI_OPT_*, in order), the dynamics, (K, T) and the
exact strings tbnav_mppi_last_kernel_names reports for the tick.  Shapes are the smallest at which the form can still go wrong:
K = 2R + 1 leaves ONE live rollout in the fused kernel's last workgroup, K = 70 a ragged wave whose dead lanes shadow rollout
K - 1, the horizons sit on the edges of steps-per-lane, chunk counts and LDS staging.  dt is the shipped 0.01; horizon(T) lies
half a step past T * dt, so that int(horizon / dt) == T whatever the quotient's rounding (asserted against m.steps).

Which instantiations exist is read from the shipped listing by the CPU test: every mppi_rollout_fused / _scan / _cost and
mppi_combine<*, 0> in it must be named by a case here; kernels of other families must match OUT_OF_SCOPE."""
import re
from collections import namedtuple

import numpy as np

DT = 0.01
WAVE = 64
COMBINE_2 = "mppi_combine<2, 0>"

Case = namedtuple("Case", "id group K T opts dyn rollout combine")


def horizon(T):
    return (T + 0.5) * DT


def _case(group, K, T, opts, dyn, rollout, combine=COMBINE_2, tag=""):
    o = ",".join(f"{n}={v}" for n, v in opts)
    ident = re.sub(r"[^A-Za-z0-9=-]+", "_", f"{rollout.replace('mppi_rollout_', '')}-K{K}-T{T}-{dyn}-{o}{tag}").strip("_")
    return Case(ident, group, K, T, tuple(opts), dyn, rollout, combine)


# how a handle is brought to the template argument TR: (TBNAV_MPPI_OPT_TRIG or None, dynamics)
FUSED_TR = {2: ((1, "rk4"), (2, "rk4")), 3: ((3, "rk4"),), 4: ((None, "arc"),)}
FUSED_T = {1: (1, 64), 2: (65, 128)}          # steps per lane TL -> its shortest and its longest horizon


def _trig_opts(trig):
    return [] if trig is None else [("TRIG", trig)]


def fused_resident_cases():
    """mppi_rollout_fused<TR, R, TL, 0>: 18 instantiations at both ends of TL's range, K = 2R + 1; one case at K = 1."""
    out = []
    for tr in (2, 3, 4):
        for R in (4, 8, 16):
            for tl in (1, 2):
                for n, T in enumerate(FUSED_T[tl]):
                    trig, dyn = FUSED_TR[tr][n % len(FUSED_TR[tr])]     # (TR = 2 is reached by TRIG 1 and by TRIG 2: one horizon each)
                    out.append(_case("fused", 2 * R + 1, T, [("KERNEL", -R)] + _trig_opts(trig), dyn, f"mppi_rollout_fused<{tr}, {R}, {tl}, 0>"))
    out.append(_case("fused", 1, 64, [("KERNEL", -8)], "rk4", "mppi_rollout_fused<2, 8, 1, 0>"))
    return out


def fused_rng_cases():
    """mppi_rollout_fused<TR, R, TL, RG>, RG = 1 (TBNAV_MPPI_OPT_SAMPLER 0) and 2 (SAMPLER 1): 24 instantiations, K = 2R + 1; with
    8 rollouts per workgroup under TBNAV_MPPI_OPT_NOISE_AHEAD 0 and 1.  `rollout` names the in-kernel-noise handle's kernel; the
    second handle (sample, then tick) runs the <TR, R, TL, 0> that fused_resident_cases holds to the oracle."""
    out = []
    for rg in (1, 2):
        for R in (8, 16):
            for tr in (2, 3, 4):
                trig, dyn = FUSED_TR[tr][0]
                for tl in (1, 2):
                    T = FUSED_T[tl][rg - 1]      # RG 1 at the short end of TL's range, RG 2 at the long end
                    for ahead in ((0, 1) if R == 8 else (None,)):
                        opts = [("KERNEL", -R), ("SAMPLER", rg - 1)] + _trig_opts(trig) + ([] if ahead is None else [("NOISE_AHEAD", ahead)])
                        out.append(_case("fused_rng", 2 * R + 1, T, opts, dyn, f"mppi_rollout_fused<{tr}, {R}, {tl}, {rg}>"))
    return out


# (steps per thread, T): one chunk, the most chunks each form admits, the switch from MW = 12 to MW = 16, a ragged last chunk
SCAN_TC_T = [(4, 7), (4, 48), (4, 49), (4, 64), (5, 1), (5, 58), (6, 71), (7, 5), (7, 106), (7, 112), (8, 96), (8, 97), (8, 128),
             (10, 119), (12, 143), (16, 190), (20, 221), (20, 240)]


def scan_mw(tc, T):
    """Most waves per workgroup of the instantiation the launcher names for (tc, T) — restated from the chunk count, not read
    from the launcher."""
    chunks = -(-T // tc)
    assert chunks <= (16 if tc in (4, 7, 8) else 12), (tc, T)
    return 16 if tc == 7 or (tc in (4, 8) and chunks > 12) else 12


def scan_cases():
    out = []
    for trig in (1, 3):
        for tc, T in SCAN_TC_T:
            out.append(_case("scan", 70, T, [("KERNEL", tc), ("TRIG", trig)], "rk4", f"mppi_rollout_scan<{trig}, {tc}, {scan_mw(tc, T)}>"))
    out.append(_case("scan", 1, 49, [("KERNEL", 4), ("TRIG", 1)], "rk4", "mppi_rollout_scan<1, 4, 16>"))
    # TRIG 2 has no time-parallel form of its own: it takes the three-evaluation one
    out.append(_case("scan", 70, 58, [("KERNEL", 5), ("TRIG", 2)], "rk4", "mppi_rollout_scan<3, 5, 12>"))
    # the arc dynamics live in the fused and the sequential kernels: a forced chunk size runs the sequential one
    out.append(_case("scan", 70, 58, [("KERNEL", 5)], "arc", "mppi_rollout_cost<4>"))
    return out


def sequential_cases():
    """mppi_rollout_cost<1..4> at K = 70: T = 28 (whole groups of steps plus a tail), T = 400 (the early steps' losses do not fit
    LDS: lds_from > 0), T = 28 with nothing staged in LDS."""
    out = []
    for tr, (trig, dyn) in {1: (1, "rk4"), 2: (2, "rk4"), 3: (3, "rk4"), 4: (None, "arc")}.items():
        for T, extra in ((28, []), (400, []), (28, [("NO_LDS_STAGING", 1)])):
            out.append(_case("sequential", 70, T, [("KERNEL", 0)] + _trig_opts(trig) + extra, dyn, f"mppi_rollout_cost<{tr}>"))
    return out


# TBNAV_MPPI_OPT_KERNEL values that must come back as TBNAV_ERR_INVALID_ARG: (T, value, why)
REJECTIONS = [(50, 9, "not a chunk size"), (65, 4, "17 chunks, the form admits 16"), (61, 5, "13 chunks, the form admits 12"),
              (129, -8, "a fused form needs T <= 128"), (50, -5, "not a fused workgroup size")]

# ---- the combine ---------------------------------------------------------------------------------------------------------------
LAMBDA = 0.01          # the shipped lambda
UMAX = 6.35495         # the shipped max_wheel_vel
COMBINE_T = (1, 5, 70)   # 70: several workgroups, the last with lanes past T
# handle's K (records per step and group S = ceil(K / 2048)) -> the group counts G of the synthetic record sets
COMBINE_G = {64: (1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1024, 1500),
             2049: (1, 3, 32, 64, 65, 128, 129, 256, 257, 300)}


def combine_name(records, wide=False):
    """The combine the launcher names for `records` records per time step in one process (wide: one group of more than 256 and at
    most 1024 records with TBNAV_MPPI_OPT_WIDE_COMBINE on)."""
    if wide and 4 * WAVE < records <= 16 * WAVE:
        return "mppi_combine_wide"
    keep = 8 if 4 * WAVE < records <= 8 * WAVE else 4 if 2 * WAVE < records <= 4 * WAVE else 2
    return f"mppi_combine<{keep}, 0>"


# whole ticks through the fused kernel with 4 rollouts per workgroup (S = ceil(K / 4) records per step): K -> what each S is for
COMBINE_TICK_K = {509: "S = 128, straight <2, 0>, a short last record", 512: "S = 128, straight <2, 0>", 513: "S = 129, <4, 0> general",
                  1024: "S = 256, straight <4, 0>", 1025: "S = 257", 2048: "S = 512", 2049: "S = 513", 4096: "S = 1024",
                  4097: "S = 1025, past the wide form"}
COMBINE_TICK_T = (3, 9)


def combine_tick_cases():
    out = []
    for K in COMBINE_TICK_K:
        S = -(-K // 4)
        for T in COMBINE_TICK_T:
            for wide in (1, 0):
                if wide == 0 and combine_name(S, True) == combine_name(S, False):
                    continue                   # (the option changes nothing below 257 records; K = 4097 keeps one case with it off)
                out.append(_case("combine_tick", K, T, [("KERNEL", -4), ("WIDE_COMBINE", wide)], "rk4", f"mppi_rollout_fused<2, 4, 1, 0>",
                                 combine_name(S, bool(wide))))
    out.append(_case("combine_tick", 4097, 3, [("KERNEL", -4), ("WIDE_COMBINE", 0)], "rk4", "mppi_rollout_fused<2, 4, 1, 0>", COMBINE_2))
    return out


def synthetic_combine_names():
    return {combine_name(G * -(-K // 2048)) for K, Gs in COMBINE_G.items() for G in Gs}


# ---- the overflow rule: a rollout whose cost overflows to +inf weighs nothing -------------------------------------------------
OVERFLOW_NOISE = 1e160     # (u + 1e160)^2 * R overflows; the state stays finite


def overflow_noise(noise, rollouts):
    """`noise` [K][T][2] with the second half of the horizon of every rollout in `rollouts` set to OVERFLOW_NOISE (a copy)."""
    bad = np.array(noise, dtype=np.float64, copy=True)
    T = bad.shape[1]
    for k in rollouts:
        bad[k, T // 2:, :] = OVERFLOW_NOISE
    return bad


def overflow_sets(K, R):
    """The cases at K = 2R + 1: the last workgroup's only live rollout; all R rollouts of the middle workgroup; every rollout
    (there the reference itself gives NaN); and one rollout among the finite ones of the first workgroup."""
    assert K == 2 * R + 1
    return {"last": [2 * R], "middle": list(range(R, 2 * R)), "all": list(range(K)), "mixed": [1]}


# (id, kernel option or None for the handle's own choice, R that shapes the overflow sets, K, T, expected rollout kernel)
OVERFLOW_PRODUCERS = (
    [(f"fused{R}-T{T}", -R, R, 2 * R + 1, T, f"mppi_rollout_fused<2, {R}, {1 if T <= 64 else 2}, 0>") for R in (4, 8, 16) for T in (50, 100)]
    + [("scan", 5, 8, 17, 50, "mppi_rollout_scan<1, 5, 12>"), ("sequential", 0, 8, 17, 50, "mppi_rollout_cost<1>")])
OVERFLOW_DEFAULT = (1025, 50, "mppi_rollout_fused<2, 8, 1, 0>")    # K % 8 == 1 at the handle's own choice: rollout 1024 overflows


# ---- what a handle picks by itself and what a tick then launches, restated from the rules in words -----------------------------
# (csrc/mppi_plan.hpp is the C++; tests/test_mppi_plan.py holds the two against each other with `==` on the CPU, and
#  tests/test_mppi_gpu.py holds the launched kernels' names against this file on the device's own CU count)
LDS_BYTES = 160 * 1024
Choice = namedtuple("Choice", "K T S lds_from prefix_rg scan_tc fused_dev fused_rng fused_r fused_S")


def _ceil(a, b):
    return -(-a // b)


def default_choice(K, T, cus):
    """What tbnav_mppi_create decides for K rollouts of T steps on a chip of `cus` CUs."""
    waves = _ceil(K, WAVE)                      # one-wave workgroups of the one-lane-per-rollout kernels
    # losses staged in LDS: the whole grid is to be resident in one round, so the (1 .. 8) workgroups a CU gets share its 160 KB;
    # each keeps 512 B spare and both control rows (16 B a step), and a staged step takes a wave of doubles.  The steps that do
    # not fit come first, in whole groups of four
    share = LDS_BYTES // min(max(_ceil(waves, cus), 1), 8)
    staged = min(max(share - 512 - 16 * T, 0) // (8 * WAVE), T)
    lds_from = min(_ceil(T - staged, 4) * 4, T)
    # the prefix form: whole groups of four steps, two workgroups per CU or more, and a late region of 1, 2 or 3 groups that
    # leaves whole rounds of three groups, at least one
    prefix_rg = 0
    if T % 4 == 0 and waves >= 2 * cus:
        prefix_rg = next((rg for rg in (1, 2, 3) if (T // 4 - rg) % 3 == 0 and T // 4 - rg >= 3), 0)
    # the time-parallel kernel: the fewest steps per thread that give at most 12 chunks; not past 2.5 workgroups per CU
    scan_tc = next((tc for tc in (4, 5, 6, 8, 10, 12, 16, 20) if _ceil(T, tc) <= 12), 0)
    if waves > 2.5 * cus:
        scan_tc = 0
    # the fused kernel: two steps per lane at most, where the time-parallel kernel could run, up to half a workgroup per CU;
    # 8 rollouts per workgroup up to an eighth of a workgroup per CU, 16 beyond
    fused = T <= 2 * WAVE and scan_tc > 0 and waves <= cus / 2
    fused_r = (8 if waves <= cus / 8 else 16) if fused else 0
    return Choice(K, T, _ceil(K, 2048), lds_from, prefix_rg, scan_tc, fused, fused, fused_r, _ceil(K, fused_r) if fused_r else 0)


SCAN_MAX_CHUNKS = {4: 16, 5: 12, 6: 12, 7: 16, 8: 16, 10: 12, 12: 12, 16: 12, 20: 12}


def kernel_option(choice, value):
    """`choice` after TBNAV_MPPI_OPT_KERNEL = value, or None where the value is refused (and the handle stays as it was)."""
    K, T = choice.K, choice.T
    if value < 0:
        if -value not in (4, 8, 16) or T > 2 * WAVE:
            return None
        return choice._replace(scan_tc=0, fused_dev=True, fused_rng=-value in (8, 16), fused_r=-value, fused_S=_ceil(K, -value))
    if value > 0 and (value not in SCAN_MAX_CHUNKS or _ceil(T, value) > SCAN_MAX_CHUNKS[value]):
        return None
    return choice._replace(scan_tc=value, fused_dev=False, fused_rng=False, fused_r=0, fused_S=0)


def staged_lds(T, lds_from):
    return 16 * T + (T - lds_from) * 8 * WAVE


def rollout_launch(choice, trig, dyn, field):
    """The rollout kernel of the three-kernel tick: (name, workgroups, waves per workgroup, dynamic LDS bytes, the lds_from the
    kernel is told, rows of J left as exclusive prefixes)."""
    K, T = choice.K, choice.T
    grid, arc = _ceil(K, WAVE), dyn == "arc"
    if field:               # a cost field: its own kernel, whatever else the handle chose; TRIG 2 has no form there
        return f"mppi_rollout_field<{4 if arc else 1 if trig == 1 else 3}>", grid, 1, staged_lds(T, choice.lds_from), choice.lds_from, 0
    if choice.scan_tc and not arc:      # TRIG 2 has no time-parallel form either
        tc = choice.scan_tc
        chunks = _ceil(T, tc)
        return f"mppi_rollout_scan<{1 if trig == 1 else 3}, {tc}, {scan_mw(tc, T)}>", grid, chunks, 8 * (2 * T + 4 * chunks * WAVE), 0, 0
    if choice.prefix_rg and not arc and trig == 1:
        return f"mppi_rollout_prefix<{choice.prefix_rg}>", grid, 1, 16 * T, 0, T - 4 * choice.prefix_rg
    return f"mppi_rollout_cost<{4 if arc else trig}>", grid, 1, staged_lds(T, choice.lds_from), choice.lds_from, 0


def fused_launch(choice, trig, dyn, in_kernel_noise, sampler):
    """The fused kernel of a handle that runs it: (name, workgroups, threads, dynamic LDS bytes).  sampler: TBNAV_MPPI_OPT_SAMPLER."""
    R, T = choice.fused_r, choice.T
    tr = 4 if dyn == "arc" else 3 if trig == 3 else 2
    rg = (2 if sampler == 1 else 1) if in_kernel_noise else 0
    return f"mppi_rollout_fused<{tr}, {R}, {1 if T <= WAVE else 2}, {rg}>", choice.fused_S, WAVE * R, 24 * T * (R + 1)


def in_kernel_noise_runs(choice, field):
    """A device-noise tick draws its perturbations inside the fused kernel (otherwise it samples first and runs the resident-noise tick)."""
    return choice.fused_rng and not field and choice.fused_r in (8, 16)


def noise_ahead_wanted(choice):
    return choice.fused_rng and choice.fused_r == 8


def rollout_name(choice, trig, dyn, field, in_kernel_noise, sampler):
    """The rollout kernel of one tick: in_kernel_noise = a device-noise tick (tbnav_mppi_enqueue_rng), else resident noise."""
    if in_kernel_noise and in_kernel_noise_runs(choice, field):
        return fused_launch(choice, trig, dyn, True, sampler)[0]
    if choice.fused_dev and not field:
        return fused_launch(choice, trig, dyn, False, sampler)[0]
    return rollout_launch(choice, trig, dyn, field)[0]


def combine_plan(T, K, G, S, direct, err, wide, ahead):
    """The combine of G groups of S records per step: (name, log2 of the lanes per time step, workgroups for the time steps,
    sampler workgroups behind them, workgroups launched, threads).  direct: the direct exchange; err: the exchange's error words
    exist (a communicator is attached); wide: TBNAV_MPPI_OPT_WIDE_COMBINE; ahead: the next tick's noise is drawn in this launch."""
    n = G * S
    log2 = 0
    while (1 << log2) < min(n, WAVE):         # lanes per time step: the power of two that holds the records, a wave at most
        log2 += 1
    blocks = _ceil(T, WAVE >> log2)           # one wave per workgroup
    mode = 2 if direct else 1 if (G > 1 and err) else 0
    if mode == 0 and G == 1 and combine_name(S, wide) == "mppi_combine_wide":
        return "mppi_combine_wide", log2, blocks, 0, T, 4 * WAVE
    ahead_blocks = _ceil(K * T, WAVE) if (ahead and mode == 0) else 0        # one pair per lane
    return combine_name(n).replace(", 0>", f", {mode}>"), log2, blocks, ahead_blocks, blocks + ahead_blocks, WAVE


def tick_names(choice, opts, dyn, device_noise=False, comm=False):
    """(rollout, combine) of a single-GPU tick of a handle that started as `choice` and had `opts` (a case's, in order) set."""
    o = dict(TRIG=1, SAMPLER=1, WIDE_COMBINE=1, NOISE_AHEAD=1)
    for name, v in opts:
        if name == "KERNEL":
            choice = kernel_option(choice, v) or choice
        elif name == "NO_LDS_STAGING" and v:
            choice = choice._replace(lds_from=choice.T, prefix_rg=0)
        elif name == "PREFIX_FORM" and not v:
            choice = choice._replace(prefix_rg=0)
        else:
            o[name] = v
    rollout = rollout_name(choice, o["TRIG"], dyn, False, device_noise, o["SAMPLER"])
    fused = "fused" in rollout
    ahead = device_noise and in_kernel_noise_runs(choice, False) and noise_ahead_wanted(choice) and bool(o["NOISE_AHEAD"]) and not comm
    return rollout, combine_plan(choice.T, choice.K, 1, choice.fused_S if fused else choice.S, False, comm, bool(o["WIDE_COMBINE"]), ahead)[0]


# ---- which kernels the table names ------------------------------------------------------------------------------------------------
def all_cases():
    return fused_resident_cases() + fused_rng_cases() + scan_cases() + sequential_cases() + combine_tick_cases()


def covered_kernels():
    """Every kernel name a case of this module asserts."""
    names = set()
    for c in all_cases():
        names.add(c.rollout); names.add(c.combine)
        if c.group == "fused_rng":
            names.add(re.sub(r", \d>$", ", 0>", c.rollout))     # the second handle's kernel
    names |= synthetic_combine_names()
    names |= {p[5] for p in OVERFLOW_PRODUCERS} | {OVERFLOW_DEFAULT[2]}
    return names


# the families every instantiation of which must have a case
HELD_FAMILIES = (r"mppi_rollout_fused<", r"mppi_rollout_scan<", r"mppi_rollout_cost<", r"mppi_combine<\d+, 0>")
# kernels of the listing that this table leaves to other tests or to nobody, with the reason (regular expressions on the name)
OUT_OF_SCOPE = {
    r"mppi_rollout_prefix<[123]>": "needs K >= 32768; tests/test_mppi_gpu.py holds all three RG to the oracle (and the overflow rule)",
    r"mppi_rollout_field<\d+>": "the cost-field kernels have their own file, tests/test_mppi_field_gpu.py",
    r"mppi_combine<[248], [12]>": "the exchange forms: <2, 1|2> run in the sharded tests; <4|8, 1|2> need more than 128 records per step "
                                  "across ranks, i.e. more than 262144 rollouts, and are held by no test",
    r"mppi_combine_wide": "named by the whole-tick combine cases here and by tests/test_mppi_gpu.py",
}


def demangled_kernel_names(listing_lines):
    """The .amdhsa_kernel names of a listing of csrc/mppi_rollout.hip or csrc/mppi_softmin.hip, spelled as tbnav_mppi_last_kernel_names
    spells them; kernels that are not rollouts or combines are left out."""
    out = set()
    for l in listing_lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+_ZN8tbnav_mk\d+(mppi_rollout_[a-z]+|mppi_combine(?:_wide)?)(I(?:Li\d+E)+)?E", l)
        if m:
            args = re.findall(r"Li(\d+)E", m.group(2) or "")
            out.add(m.group(1) + (f"<{', '.join(args)}>" if args else ""))
    return out
