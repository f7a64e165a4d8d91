"""The straight-line form of mppi_combine<KEEP, 0> (csrc/mppi_softmin.hip, combine_steps<KEEP, 0, true>: the K = 1024 and K = 2048
ticks) reduces its six wave sums side by side and without zeroed `old` operands (csrc/wave.hpp, wave_sums_dpp).  One wave handles
one time step and has its SIMD to itself, so every instruction it issues is paid for; six whole wave_sum_dpp one after the other
cost 84 `v_mov_b32 vN, 0` and 27 `s_nop` more.  The listing is the one the library ships: csrc/Makefile's flags for the
file (tools/makefile_flags.py), hipcc cross-compiles without a GPU.  Looked at: the block between the `sched_barrier` that closes
the entry loads and the first store of the controls, in mppi_combine<2, 0> and mppi_combine<4, 0>.

  * The six sums advance stage by stage: the `row_shr:1` moves of all six come before the first `row_bcast:31` move of any of
    them.  (The sums are the DPP moves behind the last weight's `v_ldexp_f64`; the minimum's lie in front of the weights.)
  * Every stage of the sums is a full-mask `bound_ctrl` move: from their first `row_shr:1` to their last `row_bcast:31` there is no
    `v_mov_b32 vN, 0` at all, and nowhere in the block does one feed a DPP move whose row and bank masks are full.
  * No scratch, at most 128 VGPRs (__launch_bounds__(256)).

Against the parent of the commit that added this file the first two fail in both instantiations (no `bound_ctrl` move at all: six
whole reductions in a row, 36 zero moves in front of full-mask DPP moves and 48 in front of masked ones); the third passes.

What this file does not hold, because it was built, measured and taken out again (docs/lab_notebook.md, Round 23): the minimum
interleaved with the three sums that need no weight, and the two weights side by side without exec-mask branches."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

COMBINE = {2: "mppi_combineILi2ELi0E", 4: "mppi_combineILi4ELi0E"}


@pytest.fixture(scope="module")
def isa():
    spec = importlib.util.spec_from_file_location("isa_always_valu", os.path.join(ROOT, "tools", "isa_always_valu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def softmin_asm(isa):
    return isa.listing("mppi_softmin")


def _function(lines, pattern):
    """The raw lines of the one kernel whose mangled name contains `pattern`, and the lines of its descriptor."""
    names = [m.group(1) for l in lines for m in [re.match(r"^(_Z\S+):", l)] if m and pattern in m.group(1)]
    assert len(names) == 1, (pattern, names)
    start = next(i for i, l in enumerate(lines) if l.startswith(names[0] + ":"))
    end = next(i for i in range(start, len(lines)) if ".Lfunc_end" in lines[i])
    desc = lines.index(next(l for l in lines if l.strip() == ".amdhsa_kernel " + names[0]))
    return lines[start + 1:end], lines[desc:next(i for i in range(desc, len(lines)) if ".end_amdhsa_kernel" in lines[i])]


def _block(lines, pattern):
    """Instructions and labels from the entry's sched_barrier to the first store of the controls, comments stripped."""
    body, _ = _function(lines, pattern)
    first = next(i for i, l in enumerate(body) if "sched_barrier" in l)
    out = []
    for l in body[first + 1:]:
        l = l.split(";")[0].strip()
        if l.startswith("global_store"):
            return out
        if l and (not l.startswith(".") or re.match(r"^\.LBB\d+_\d+:", l)):
            out.append(l)
    raise AssertionError("no store behind the entry")


def _where(block, what):
    return [i for i, l in enumerate(block) if re.search(what, l)]


def _sums(block, keep):
    """(indices of the sums' row_shr:1 moves, of their row_bcast:31 moves): the DPP moves behind the last weight."""
    ldexp = _where(block, r"^v_ldexp_f64")
    assert len(ldexp) == keep, ldexp
    shr1 = [i for i in _where(block, r"^v_mov_b32_dpp .*row_shr:1 ") if i > ldexp[-1]]
    bc31 = [i for i in _where(block, r"^v_mov_b32_dpp .*row_bcast:31 ") if i > ldexp[-1]]
    assert len(shr1) == 12 and len(bc31) == 12, ([block[i] for i in shr1], [block[i] for i in bc31])   # six sums, two halves each
    return shr1, bc31


@pytest.mark.parametrize("keep", sorted(COMBINE))
def test_the_six_wave_sums_advance_stage_by_stage(softmin_asm, keep):
    block = _block(softmin_asm, COMBINE[keep])
    shr1, bc31 = _sums(block, keep)
    assert max(shr1) < min(bc31), (shr1, bc31)


@pytest.mark.parametrize("keep", sorted(COMBINE))
def test_no_zeroed_old_operand_in_the_wave_sums(isa, softmin_asm, keep):
    block = _block(softmin_asm, COMBINE[keep])
    shr1, bc31 = _sums(block, keep)
    moves = [i for i in range(min(shr1), max(bc31) + 1) if block[i].startswith("v_mov_b32_dpp")]
    assert len(moves) == 6 * 7 * 2, len(moves)               # seven stages of six sums, two halves each
    assert all("row_mask:0xf bank_mask:0xf bound_ctrl:1" in block[i] for i in moves), [block[i] for i in moves if "bound_ctrl:1" not in block[i]]
    zero = [i for i in range(min(shr1), max(bc31) + 1) if re.match(r"^v_mov_b32_e32\s+v\d+,\s*0$", block[i])]
    assert not zero, [block[i - 1:i + 3] for i in zero[:4]]
    dead = isa.dead_zero_moves(block)
    assert not dead, [block[i:i + 3] for i in dead[:4]]


@pytest.mark.parametrize("keep", sorted(COMBINE))
def test_no_scratch_and_the_launch_bounds_register_budget(softmin_asm, keep):
    body, desc = _function(softmin_asm, COMBINE[keep])
    assert not [l for l in body if re.match(r"\s*scratch_", l)], "scratch instructions"
    field = {m.group(1): int(m.group(2)) for l in desc for m in [re.match(r"\s*\.amdhsa_(\w+)\s+(\d+)\s*$", l)] if m}
    assert field["private_segment_fixed_size"] == 0, field
    assert 0 < field["next_free_vgpr"] <= 128, field["next_free_vgpr"]
