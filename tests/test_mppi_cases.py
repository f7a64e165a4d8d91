"""The MPPI case table (tests/mppi_cases.py) on the CPU: it names every instantiation the shipped listing holds, its references
are sound, and its overflow inputs do what they are meant to.  No device."""
import importlib.util
import os
import re

import numpy as np
import pytest

import mppi_cases as mc
import oracle_api as orc
import test_mppi_combine_gpu as tc       # the extended-precision combine reference and the record generator live with their GPU test
from cases import WAYPOINTS, mppi_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


# ---- the table is complete ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shipped_kernels():
    """Kernel names of csrc/mppi_rollout.hip and csrc/mppi_softmin.hip under the Makefile's flags (tools/isa_always_valu.py, as
    tests/test_mppi_dead_valu_isa.py compiles its listing); only the .amdhsa_kernel lines are read."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    spec = importlib.util.spec_from_file_location("isa_always_valu", os.path.join(ROOT, "tools", "isa_always_valu.py"))
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    return mc.demangled_kernel_names(isa.listing("mppi_rollout")) | mc.demangled_kernel_names(isa.listing("mppi_softmin"))


def test_every_shipped_instantiation_has_a_case_or_a_stated_exclusion(shipped_kernels):
    held = {k for k in shipped_kernels if any(re.match(f, k) for f in mc.HELD_FAMILIES)}
    # what the launchers of csrc/mppi.hip can name (the lists of forms of csrc/mppi_plan.hpp): 42 fused, 22 time-parallel, 4 sequential, 3 single-process combines
    assert [sum(1 for k in held if k.startswith(p)) for p in ("mppi_rollout_fused<", "mppi_rollout_scan<", "mppi_rollout_cost<", "mppi_combine<")] \
        == [42, 22, 4, 3], sorted(held)
    covered = mc.covered_kernels()
    assert not held - covered, f"instantiations without a case in tests/mppi_cases.py: {sorted(held - covered)}"
    rest = shipped_kernels - held
    unexplained = [k for k in rest if not any(re.fullmatch(p, k) for p in mc.OUT_OF_SCOPE)]
    assert not unexplained, f"kernels neither held nor excluded with a reason: {sorted(unexplained)}"
    assert not covered - shipped_kernels, f"cases that name kernels the library does not ship: {sorted(covered - shipped_kernels)}"


def test_the_table_is_what_it_says():
    fr, fg, sc, sq = mc.fused_resident_cases(), mc.fused_rng_cases(), mc.scan_cases(), mc.sequential_cases()
    assert len({c.rollout for c in fr}) == 18 and len({c.rollout for c in fg}) == 24
    assert len({c.rollout for c in sc if "scan" in c.rollout}) == 22 and len({c.rollout for c in sq}) == 4
    ids = [c.id for c in mc.all_cases()]
    assert len(ids) == len(set(ids))
    for c in fr + fg:     # K = 2R + 1 (or 1); TL from T
        R, TL = (int(x) for x in re.match(r"mppi_rollout_fused<\d, (\d+), (\d), \d>", c.rollout).groups())
        assert c.K in (2 * R + 1, 1) and TL == -(-c.T // 64) and c.T <= 128 and ("KERNEL", -R) in c.opts
    for c in mc.all_cases():      # the horizon gives the wanted T
        assert orc.mppi_steps(mppi_cfg(c.K, mc.horizon(c.T))) == c.T
    for T, value, _ in mc.REJECTIONS:
        assert orc.mppi_steps(mppi_cfg(70, mc.horizon(T))) == T
    # the chunk counts the time-parallel cases are there for: one chunk, 12 and 13 (MW 12 -> 16), 16, ragged and whole last chunks
    chunks = {(tc_, -(-T // tc_), T % tc_ != 0) for tc_, T in mc.SCAN_TC_T}
    assert {(4, 12, False), (4, 13, True), (4, 16, False), (8, 12, False), (8, 13, True), (8, 16, False), (7, 16, False), (5, 1, True),
            (7, 1, True), (5, 12, True), (20, 12, False)} <= chunks
    # combine: every edge of the record counts, both sides
    for K, Gs in mc.COMBINE_G.items():
        S = -(-K // 2048)
        counts = {G * S for G in Gs}
        for edge in (128, 256, 512):
            assert edge in counts and any(edge < c <= edge + 2 for c in counts), (K, edge)
    assert {64, 65, 1024, 1025} <= {G for G in mc.COMBINE_G[64]} | {1025} and mc.combine_name(128) == "mppi_combine<2, 0>"
    assert [mc.combine_name(n) for n in (129, 256, 257, 512, 513)] == ["mppi_combine<4, 0>"] * 2 + ["mppi_combine<8, 0>"] * 2 + ["mppi_combine<2, 0>"]
    assert {c.combine for c in mc.combine_tick_cases()} == {"mppi_combine<2, 0>", "mppi_combine<4, 0>", "mppi_combine<8, 0>", "mppi_combine_wide"}


# ---- the references are sound ------------------------------------------------------------------------------------------------------
def _oracle_combine(rec, u0, T):
    """oracle_api.mppi_combine on [G][T][S][8] (its own layout is [n_rec][T][8])."""
    G, _, S, _ = rec.shape
    flat = np.ascontiguousarray(rec.transpose(0, 2, 1, 3).reshape(G * S, T, 8))
    return orc.mppi_combine(mppi_cfg(64, mc.horizon(T)), u0, tc.UINIT, flat)


@pytest.mark.parametrize("G,S,T", [(1, 1, 1), (3, 1, 5), (65, 2, 5), (300, 1, 70)])
def test_extended_precision_combine_agrees_with_the_oracle_on_records_without_empties(G, S, T):
    seed = tc.seed_of(64 * S, G, T)
    rec, u0 = tc.draw_records(seed, G, T, S), tc.warm_start(seed, T)
    ref = tc.two_calls_reference(rec, u0)
    u1, out1 = _oracle_combine(rec, u0, T)
    assert np.allclose(u1, ref["nxt1"], rtol=1e-13, atol=1e-13) and np.allclose(out1, ref["out1"], rtol=1e-13, atol=1e-13)
    u2, out2 = _oracle_combine(rec, u1, T)
    assert np.allclose(u2, ref["nxt2"], rtol=1e-13, atol=1e-13) and np.allclose(out2, ref["out2"], rtol=1e-13, atol=1e-13)


def test_every_ordinary_synthetic_case_is_well_posed_and_unclamped():
    """At least three records of weight > 1e-3 per step (all of them where there are fewer), no control on the clamp — asserted
    again by the GPU test in front of its launch; here for every case without a device."""
    for K, Gs in mc.COMBINE_G.items():
        S = -(-K // 2048)
        for G in Gs:
            for T in mc.COMBINE_T:
                seed = tc.seed_of(K, G, T)
                rec = tc.draw_records(seed, G, T, S)
                assert rec.shape == (G, T, S, 8) and np.all(rec[..., 6] >= 1) and np.all(rec[..., 0] >= 50.0) and np.all(rec[..., 0] <= 500.02)
                ref = tc.two_calls_reference(rec, tc.warm_start(seed, T))
                assert tc.well_posed(rec) and not ref["clamped"].any(), (K, G, T)


def test_extended_precision_combine_agrees_with_the_oracle_tick_cut_into_records():
    """A whole 64 x 25 tick: records formed here from the oracle's J over 8 slices of 8 rollouts (include/tbnav_mppi.h, "Sharded
    soft-min"), combined by the reference, against oracle_api.mppi_new_controls."""
    d = mppi_cfg(64, 0.25)
    T, K, lam = 25, 64, d["lam"]
    noise = orc.normal_stream(42, K * T * 2, 0.0, np.sqrt(0.9)).reshape(K, T, 2)
    u0 = np.zeros((2, T))
    ref = orc.mppi_new_controls(d, u0, (0.0, 0.0), WAYPOINTS[1], (0.0, 0.0, 0.0), noise)
    rec = np.zeros((T, 8, 8))
    for s in range(8):
        J = ref["J"][:, 8 * s:8 * s + 8]
        dl, dr = noise[8 * s:8 * s + 8, :, 0].T, noise[8 * s:8 * s + 8, :, 1].T
        m = J.min(axis=1)
        e = np.exp(((J - m[:, None]) * -1.0) / lam)
        rec[:, s] = np.stack([m, e.sum(1), (e * dl).sum(1), (e * dr).sum(1), dl.sum(1), dr.sum(1), np.full(T, 8.0), np.zeros(T)], axis=1)
    upd, nxt, out, clamped = tc.combine_reference(rec, u0, (0.0, 0.0), lam, d["max_wheel_vel"])
    assert np.allclose(upd, ref["u_upd"], rtol=1e-12, atol=1e-13) and np.allclose(nxt, ref["u"], rtol=1e-12, atol=1e-13)
    assert np.allclose(out, ref["out"], rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("K,G,T", tc.SPECIAL_SHAPES)
def test_each_special_record_set_changes_the_answer_or_provably_must_not(K, G, T):
    S = -(-K // 2048)

    def answer(rec, seed):
        return tc.two_calls_reference(rec, tc.warm_start(seed, T))

    for kind in tc.SPECIAL_KINDS:
        seed = tc.seed_of(K, G, T, kind)
        plain, special = tc.draw_records(seed, G, T, S), tc.special_records(kind, seed, G, T, S)
        a, b = answer(plain, seed), answer(special, seed)
        assert np.all(np.isfinite(b["nxt2"])), kind
        assert not np.allclose(a["nxt2"], b["nxt2"], rtol=1e-6, atol=1e-9), kind     # a consumer that ignored the change would be caught
        if kind == "clamp":
            assert b["clamped"].any() and (b["upd1"] == mc.UMAX).any() and (b["upd1"] == -mc.UMAX).any()
        if kind.startswith("empty_groups"):
            # an empty record's fields must NOT change the answer: the live records alone give the same bits, whatever m says
            live_only = special[0::2]
            c = tc.combine_reference(tc.by_step(live_only), tc.warm_start(seed, T), tc.UINIT)
            assert np.array_equal(c[0], b["upd1"]), kind
            # ... and a reader that took its minimum over the empty records too (oracle_api.mppi_combine does) would differ
            if kind == "empty_groups_low_m":
                with np.errstate(all="ignore"):
                    u1, _ = _oracle_combine(special, tc.warm_start(seed, T), T)
                assert not np.allclose(u1, b["nxt1"], rtol=1e-6, atol=1e-9, equal_nan=False)
        if kind == "overflowed":
            # the record weighs nothing in the soft-min but counts in the 1e-8 floor: dropping it altogether moves the answer a
            # little, giving it weight moves it a lot
            dropped = special.copy(); dropped[np.isinf(special[..., 0])] = 0.0
            c = answer(dropped, seed)
            assert not np.array_equal(c["nxt1"], b["nxt1"]) and np.allclose(c["nxt1"], b["nxt1"], rtol=1e-3, atol=1e-3)


# ---- the overflow inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,T", [(4, 50), (8, 100), (16, 50)])
def test_overflow_inputs_give_infinite_cost_exactly_in_the_intended_rollouts(R, T):
    K = 2 * R + 1
    d = mppi_cfg(K, mc.horizon(T))
    noise = orc.normal_stream(K + T, K * T * 2, 0.0, np.sqrt(0.9)).reshape(K, T, 2)
    for which, rollouts in mc.overflow_sets(K, R).items():
        with np.errstate(all="ignore"):
            ref = orc.mppi_new_controls(d, np.zeros((2, T)), (0, 0), WAYPOINTS[2], (0.3, -0.2, 0.7), mc.overflow_noise(noise, rollouts))
        fine = np.setdiff1d(np.arange(K), rollouts)
        assert np.all(ref["J"][:, rollouts] == np.inf) and np.all(np.isfinite(ref["J"][:, fine])), which
        if which == "all":
            assert np.all(np.isnan(ref["u"][:, :-1])) and np.all(np.isnan(ref["out"]))
        else:
            assert np.all(np.isfinite(ref["u"])) and np.all(np.isfinite(ref["out"])), which
            assert np.all(ref["u"][:, T // 2:-1] == d["max_wheel_vel"])    # (the 1e-8 floor times 1e160: those steps sit on the clamp)
    K, T, _ = mc.OVERFLOW_DEFAULT
    assert K % 8 == 1
