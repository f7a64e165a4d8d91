"""mppi_rollout_fused issues no vector instruction whose result nothing can read (csrc/mppi_rollout.hip, csrc/wave.hpp), in the
listing the library ships (csrc/Makefile's flags for the file, tools/makefile_flags.py; hipcc cross-compiles without a GPU):

  * small_sincos's full-range evaluation stays behind its wave-uniform branch: between the kernel's entry and s_barrier, outside
    every region a forward conditional branch can skip, a lane's step rounds to the quadrant twice (v_rndne_f64) — the ONE
    fast_sincos of the step's heading.  Turned into selects, the fallback's Cody-Waite reduction adds two more per step.
  * no `v_mov_b32 vN, 0` feeds the `old` operand of a DPP move whose row and bank masks are full: every lane either has a source
    (the butterfly partners of group_reduce_dpp) or gets bound_ctrl's zero (row_shr / row_shl 1..3 of the scans).

Against the parent of the commit that added this file both fail on each instantiation: 4 v_rndne_f64 per step, and 66 such moves
(24 in front of the barrier, 42 in the record loop).  The analysis is tools/isa_always_valu.py's; no instruction total is pinned."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

# one step per lane (TL = 1): the fp32 and the fp64 sampler drawn in the kernel, and resident noise
FUSED = {"<2, 8, 1, 1>": "mppi_rollout_fusedILi2ELi8ELi1ELi1E", "<2, 8, 1, 2>": "mppi_rollout_fusedILi2ELi8ELi1ELi2E",
         "<2, 8, 1, 0>": "mppi_rollout_fusedILi2ELi8ELi1ELi0E"}
STEPS_PER_LANE = 1


@pytest.fixture(scope="module")
def isa():
    spec = importlib.util.spec_from_file_location("isa_always_valu", os.path.join(ROOT, "tools", "isa_always_valu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def rollout_asm(isa):
    return isa.listing("mppi_rollout")


@pytest.mark.parametrize("inst", sorted(FUSED))
def test_one_full_range_sincos_per_step_in_front_of_the_barrier(isa, rollout_asm, inst):
    body = isa.kernel_body(rollout_asm, FUSED[inst])
    assert any(l.startswith("s_barrier") for l in body)
    c = isa.count(body, "v_rndne_f64")
    always = c["entry"][1] + c["to barrier"][1]
    assert 0 < always <= 2 * STEPS_PER_LANE, c


@pytest.mark.parametrize("inst", sorted(FUSED))
def test_no_zeroed_old_operand_in_front_of_a_full_mask_dpp_move(isa, rollout_asm, inst):
    body = isa.kernel_body(rollout_asm, FUSED[inst])
    assert sum(1 for l in body if l.startswith("v_mov_b32_dpp")) >= 40, "the scans and the group reductions are DPP moves"
    dead = isa.dead_zero_moves(body)
    assert not dead, [body[i:i + 3] for i in dead[:4]]
