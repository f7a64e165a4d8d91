"""csrc/mppi_plan.hpp — which kernel a (K, T) takes, what a forced TBNAV_MPPI_OPT_KERNEL turns that into, which instantiation a
tick launches and with what grid, block and LDS, as plain host arithmetic — compiled into tests/mppi_plan_check.cpp with g++ alone
(no HIP, no library, no GPU) and held with `==` against the independent statements of the same rules in tests/mppi_cases.py:
default_choice, kernel_option, rollout_launch, fused_launch, combine_plan.  The GPU suite ties the launched kernels to the same
Python (tests/test_mppi_gpu.py, tests/test_mppi_instantiations_gpu.py); this ties the C++ that chooses them to it on every machine."""
import itertools
import os
import re
import subprocess

import pytest

import mppi_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = (1, 64, 256, 304)
TS = tuple(range(1, 261)) + (400, 1000)
DYN = {"rk4": 0, "arc": 1}
# the lists of forms, written out here from the families' template arguments (not read from the header)
FUSED = {f"mppi_rollout_fused<{tr}, {r}, {tl}, {rg}>" for tr in (2, 3, 4) for tl in (1, 2) for r, rg in
         ((4, 0), (8, 0), (16, 0), (8, 1), (16, 1), (8, 2), (16, 2))}
SCAN = {f"mppi_rollout_scan<{tr}, {tc}, {mw}>" for tr in (1, 3) for tc, mw in
        ((4, 16), (4, 12), (5, 12), (6, 12), (7, 16), (8, 16), (8, 12), (10, 12), (12, 12), (16, 12), (20, 12))}
COST = {f"mppi_rollout_cost<{tr}>" for tr in (1, 2, 3, 4)}
PREFIX = {f"mppi_rollout_prefix<{rg}>" for rg in (1, 2, 3)}
FIELD = {f"mppi_rollout_field<{tr}>" for tr in (1, 3, 4)}
COMBINE = {f"mppi_combine<{keep}, {mode}>" for keep in (2, 4, 8) for mode in (0, 1, 2)}


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mppi_plan") / "mppi_plan_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "ros-turtlebot-navigation_amd", "csrc"),
                    os.path.join(ROOT, "tests", "mppi_plan_check.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out = r.stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return run


def sweep_K(cus):
    """Every threshold of create's rules in one-wave workgroups (cus / 8, cus / 2, 2 cus, 2.5 cus), one wave and one rollout to
    either side of each, plus 1 and 70 — and the ensemble sizes the notes on default_choice's edges name."""
    ks = {1, 70, 16389, 40000, 45000, 65536}
    for eighths in (1, 4, 16, 20):
        k = 64 * cus * eighths // 8
        ks |= {k - 64, k - 1, k, k + 1, k + 64}
    return sorted(k for k in ks if k >= 1)


def _choice_of(text, K, T):
    S, lds_from, rg, tc, fd, fr, R, fS = (int(v) for v in text.split())
    return mc.Choice(K, T, S, lds_from, rg, tc, bool(fd), bool(fr), R, fS)


# ---- create ------------------------------------------------------------------------------------------------------------------------------
def test_plan_create_is_the_restated_choice_over_the_sweep(ask):
    keys = [(K, T, cus) for cus in CUS for K in sweep_K(cus) for T in TS]
    assert len(keys) > 20000
    got = ask(["C %d %d %d" % k for k in keys])
    seen = set()
    for (K, T, cus), g in zip(keys, got):
        c = mc.default_choice(K, T, cus)
        assert _choice_of(g, K, T) == c, ((K, T, cus), g)
        seen.add((c.prefix_rg, c.scan_tc, c.fused_r, c.lds_from > 0))
    assert {s[0] for s in seen} == {0, 1, 2, 3} and {s[1] for s in seen} == {0, 4, 5, 6, 8, 10, 12, 16, 20}
    assert {s[2] for s in seen} == {0, 8, 16} and {s[3] for s in seen} == {False, True}


def test_the_restated_choice_at_256_cus_is_what_the_gpu_test_expects_and_has_the_stated_edges():
    def name(K, T):
        return mc.rollout_name(mc.default_choice(K, T, 256), 1, "rk4", False, False, 1)
    want = [(1024, 25, "fused<2, 8"), (2048, 50, "fused<2, 8"), (4096, 100, "fused<2, 16"), (8192, 100, "fused<2, 16"), (16389, 50, "scan"),
            (40000, 25, "scan"), (45000, 12, "cost"), (45000, 60, "prefix")]
    for K, T, part in want:
        assert part in name(K, T), (K, T, name(K, T))
    d = lambda K, T=50: mc.default_choice(K, T, 256)       # noqa: E731
    assert (d(2048).fused_r, d(2049).fused_r, d(8192).fused_r, d(8193).fused_r) == (8, 16, 16, 0)
    assert d(40960).scan_tc > 0 and d(40961).scan_tc == 0
    assert d(32704, 60).prefix_rg == 0 and d(32705, 60).prefix_rg > 0
    assert (d(70, 400).lds_from, d(65536, 100).lds_from, d(65536, 400).lds_from) == (96, 28, 336)


# ---- TBNAV_MPPI_OPT_KERNEL ---------------------------------------------------------------------------------------------------------------
VALUES = tuple(range(-17, 22))


def test_plan_kernel_option_accepts_and_refuses_as_restated(ask):
    keys = [(T, K, v) for T in TS for K in (1, 70, 2049) for v in VALUES]
    got = ask(["O %d %d %d" % k for k in keys])
    base = mc.Choice(0, 0, 0, 0, 0, 4, True, True, 8, 1)     # (whatever the handle held: an accepted value replaces all five)
    accepted = set()
    for (T, K, v), g in zip(keys, got):
        ok, tc, R, fS, fd, fr = (int(x) for x in g.split())
        c = mc.kernel_option(base._replace(K=K, T=T), v)
        if c is None:
            assert (ok, tc, R, fS, fd, fr) == (0, 0, 0, 0, 0, 0), ((T, K, v), g)
        else:
            assert (ok, tc, R, fS, bool(fd), bool(fr)) == (1, c.scan_tc, c.fused_r, c.fused_S, c.fused_dev, c.fused_rng), ((T, K, v), g)
            accepted.add(v)
    assert accepted == {-16, -8, -4, 0, 4, 5, 6, 7, 8, 10, 12, 16, 20}
    for T, v, why in mc.REJECTIONS:
        assert ask(["O %d 70 %d" % (T, v)])[0].split()[0] == "0", why
        assert mc.kernel_option(base._replace(K=70, T=T), v) is None, why


# ---- the rollout launch, the fused launch, the predicates ------------------------------------------------------------------------------
def _variants(c):
    """The handle's own choice, the choice after every TBNAV_MPPI_OPT_KERNEL value (a refused value leaves it as it was), after
    NO_LDS_STAGING and after PREFIX_FORM 0."""
    out = {c, c._replace(lds_from=c.T, prefix_rg=0), c._replace(prefix_rg=0)}
    for v in VALUES:
        out.add(mc.kernel_option(c, v) or c)
    return out


def test_plan_rollout_and_plan_fused_are_the_restatements_over_the_sweep(ask):
    choices = set()
    for cus in CUS:
        for K in sweep_K(cus):
            for T in TS:
                choices |= _variants(mc.default_choice(K, T, cus))
    modes = list(itertools.product((1, 2, 3), ("rk4", "arc"), (False, True)))
    r_keys, f_keys, q_keys = [], [], set()
    for c in choices:
        for trig, dyn, field in modes:
            r_keys.append((c, trig, dyn, field))
        if c.fused_dev:
            f_keys += [(c, trig, dyn, False, s) for trig in (1, 2, 3) for dyn in DYN for s in (0, 1)]
        for field in (False, True):
            q_keys.add((c.fused_rng and not field, c.fused_r, c.K))
            if mc.in_kernel_noise_runs(c, field):
                f_keys += [(c, trig, dyn, True, s) for trig in (1, 2, 3) for dyn in DYN for s in (0, 1)]
    assert len(r_keys) > 1000000 and len(f_keys) > 100000
    seen = set()
    got = ask(["R %d %d %d %d %d %d %d %d" % (c.T, c.K, DYN[dyn], trig, c.scan_tc, c.prefix_rg, c.lds_from, field) for c, trig, dyn, field in r_keys])
    for (c, trig, dyn, field), g in zip(r_keys, got):
        grid, by, lds, lds_from, rows, listed, name = g.split(" ", 6)
        assert (name, int(grid), int(by), int(lds), int(lds_from), int(rows)) == mc.rollout_launch(c, trig, dyn, field) and listed == "1", (c, trig, dyn, field, g)
        seen.add(name)
    got = ask(["F %d %d %d %d %d %d %d %d" % (c.T, c.K, DYN[dyn], trig, s, c.fused_r, c.fused_S, rng) for c, trig, dyn, rng, s in f_keys])
    for (c, trig, dyn, rng, s), g in zip(f_keys, got):
        grid, block, lds, listed, name = g.split(" ", 4)
        assert (name, int(grid), int(block), int(lds)) == mc.fused_launch(c, trig, dyn, rng, s) and listed == "1", (c, trig, dyn, rng, s, g)
        seen.add(name)
    # every name of every list, and nothing outside them
    assert seen == FUSED | SCAN | COST | PREFIX | FIELD, (sorted(seen - (FUSED | SCAN | COST | PREFIX | FIELD)), sorted((FUSED | SCAN | COST | PREFIX | FIELD) - seen))
    assert [len(s) for s in (FUSED, SCAN, COST, PREFIX, FIELD)] == [42, 22, 4, 3, 3]
    # the predicates: in-kernel noise, noise ahead, a graph of ticks
    q_keys = sorted((fr, R, K, n) for fr, R, K in q_keys for n in (1, 2, 20))
    for (fr, R, K, n), g in zip(q_keys, ask(["Q %d %d %d %d" % k for k in q_keys])):
        in_kernel = fr and R in (8, 16)
        assert [int(x) for x in g.split()] == [in_kernel, fr and R == 8, in_kernel and R == 8 and K <= 1536 and n >= 2], ((fr, R, K, n), g)


# ---- the combine -------------------------------------------------------------------------------------------------------------------------
def test_plan_combine_is_the_restatement_over_the_sweep(ask):
    splits = set()
    for n in itertools.chain(range(1, 1101), range(2047, 2051)):
        splits |= {(1, n), (n, 1)} | {(g, n // g) for g in (2, 3, 32) if n % g == 0} | {(n // s, s) for s in (2, 5) if n % s == 0}
    keys = []
    for (G, S), T, direct, err, wide, ahead in itertools.product(sorted(splits), (1, 5, 64, 70, 128), (0, 1), (0, 1), (0, 1), (0, 1)):
        for K in ((17, 2049) if ahead else (17,)):          # (K only sizes the sampler blocks: the fused cases' 2R + 1)
            keys.append((T, K, G, S, direct, err, wide, ahead))
    got = ask(["M %d %d %d %d %d %d %d %d" % k for k in keys])
    seen = set()
    for k, g in zip(keys, got):
        log2, blocks, ahead_blocks, grid, block, listed, name = g.split(" ", 6)
        assert (name, int(log2), int(blocks), int(ahead_blocks), int(grid), int(block)) == mc.combine_plan(*k) and listed == "1", (k, g)
        seen.add(name)
    assert seen == COMBINE | {"mppi_combine_wide"} and len(COMBINE) == 9, seen
    # (the restatement agrees with the names the case table has used all along)
    assert all(mc.combine_plan(5, 17, 1, n, 0, 0, w, 0)[0] == mc.combine_name(n, bool(w)) for n in range(1, 1101) for w in (0, 1))


# ---- the lists, the names ------------------------------------------------------------------------------------------------------------------
def test_the_lists_of_forms_are_the_families_written_out(ask):
    names = ask(["L"])[0].split(";")
    assert len(names) == len(set(names)) == 42 + 22 + 3 + 4 + 3 + 9 + 1
    assert set(names) == FUSED | SCAN | COST | PREFIX | FIELD | COMBINE | {"mppi_combine_wide"}
    # in the order the instantiations have always been written (what keeps the code objects comparable byte for byte)
    fused = lambda tr, pairs: [f"mppi_rollout_fused<{tr}, {r}, {tl}, {rg}>" for r, rg in pairs for tl in (1, 2)]       # noqa: E731
    order = [n for tr in (2, 3, 4) for n in fused(tr, ((4, 0), (8, 0), (16, 0), (8, 1), (16, 1)))] + [n for tr in (2, 3, 4) for n in fused(tr, ((8, 2), (16, 2)))]
    order += [f"mppi_rollout_scan<{tr}, {tc}, {mw}>" for tr in (1, 3) for tc, mw in
              ((4, 16), (4, 12), (5, 12), (6, 12), (7, 16), (8, 16), (8, 12), (10, 12), (12, 12), (16, 12), (20, 12))]
    order += [f"mppi_rollout_prefix<{rg}>" for rg in (1, 2, 3)] + [f"mppi_rollout_cost<{tr}>" for tr in (1, 2, 3, 4)]
    order += [f"mppi_rollout_field<{tr}>" for tr in (1, 3, 4)] + [f"mppi_combine<{k}, {m}>" for m in (0, 1, 2) for k in (2, 4, 8)] + ["mppi_combine_wide"]
    assert names == order


def test_every_case_string_comes_out_of_form_name_for_the_case_options(ask):
    """Each case of tests/mppi_cases.py: its options applied to the restated choice at 256 CUs, the tick's launches asked of the
    C++ plan — the strings tbnav_mppi_last_kernel_names would format — against the case's own."""
    lines, want = [], []
    for c in mc.all_cases():
        ch, o = mc.default_choice(c.K, c.T, 256), dict(TRIG=1, SAMPLER=1, WIDE_COMBINE=1, NOISE_AHEAD=1)
        for name, v in c.opts:
            if name == "KERNEL":
                ok, tc, R, fS, fd, fr = (int(x) for x in ask(["O %d %d %d" % (c.T, c.K, v)])[0].split())
                assert ok == 1, c.id
                ch = ch._replace(scan_tc=tc, fused_r=R, fused_S=fS, fused_dev=bool(fd), fused_rng=bool(fr))
            elif name == "NO_LDS_STAGING":
                ch = ch._replace(lds_from=c.T, prefix_rg=0)
            else:
                o[name] = v
        rng = c.group == "fused_rng"          # (that group's `rollout` names the in-kernel-noise handle's kernel)
        in_kernel, ahead_wanted, _ = (int(x) for x in ask(["Q %d %d %d 1" % (ch.fused_rng, ch.fused_r, c.K)])[0].split())
        fused = (rng and in_kernel) or ch.fused_dev
        if fused:
            lines.append("F %d %d %d %d %d %d %d %d" % (c.T, c.K, DYN[c.dyn], o["TRIG"], o["SAMPLER"], ch.fused_r, ch.fused_S, rng and in_kernel))
        else:
            lines.append("R %d %d %d %d %d %d %d 0" % (c.T, c.K, DYN[c.dyn], o["TRIG"], ch.scan_tc, ch.prefix_rg, ch.lds_from))
        lines.append("M %d %d 1 %d 0 0 %d %d" % (c.T, c.K, ch.fused_S if fused else ch.S, o["WIDE_COMBINE"], rng and in_kernel and ahead_wanted and o["NOISE_AHEAD"]))
        want += [c.rollout, c.combine]
        assert mc.tick_names(mc.default_choice(c.K, c.T, 256), c.opts, c.dyn, device_noise=rng) == (c.rollout, c.combine), c.id
    got = [re.sub(r"^[\d ]+ (?=mppi_)", "", g) for g in ask(lines)]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]
