"""The case table of the device noise source, shared by test_noise_restatement.py (CPU: counter spaces, the mutation proof) and
test_noise_gpu.py (every stored draw against noise_restatement.py).

MPPI rows: (K, T, seed, tick, ul_var, ur_var, sampler, shard); shard = None or (first_rollout, rollouts_global).
  shapes  (1, 1); (3, 5); (257, 7): K a multiple of neither the wave nor the block; (64, 50); (1024, 50): the headline tick's;
          (16384, 129): T*K = 2 113 536 > 8192 * 256, the smallest shape at which mppi_sample_noise's grid cap binds and threads
          take a second trip (one row per sampler there)
  ticks   0, 1 and 2^32 + 3 (the counter's high word); seeds 0, 77 and 2^63 + 5 (the key's high word)
  ul_var = 0.9, ur_var = 0.4: exchanged sigmas show
  shards  first_rollout 0 and 2K + 1 of rollouts_global = 5K
RBPF rows: (id, N, k, icp_ok per scan, seed, shard, reseed); seed None = the handle's default 0x5EED without a tbnav_rbpf_set_seed
  call; shard = None or (first_particle, particles_global); reseed = None or (scan, seed): tbnav_rbpf_set_seed before that scan,
  which starts the scan count again.  Three scans each: scan << 40 is in the counter.
"""
from collections import namedtuple

MppiRow = namedtuple("MppiRow", "K T seed tick ul_var ur_var sampler shard")
RbpfRow = namedtuple("RbpfRow", "id N k icp seed shard reseed")

UL_VAR, UR_VAR = 0.9, 0.4
HIGH_TICK, HIGH_SEED = 2 ** 32 + 3, 2 ** 63 + 5
MPPI_SHAPES = [(1, 1), (3, 5), (257, 7), (64, 50), (1024, 50)]
MPPI_LARGE = (16384, 129)
MPPI_DT = 0.01
RBPF_DEFAULT_SEED = 0x5EED


def _mppi_rows():
    rows = []
    for K, T in MPPI_SHAPES:
        none, low, high = None, (0, 5 * K), (2 * K + 1, 5 * K)
        # every tick, seed and shard setting, each with both samplers; the high tick and the high seed once alone and once together,
        # both with and without a shard in front of them
        for seed, tick, shard in [(0, 0, none), (77, 1, low), (77, HIGH_TICK, none), (HIGH_SEED, 0, low), (HIGH_SEED, HIGH_TICK, high),
                                  (0, 1, high), (77, 0, high)]:
            for sampler in ("wide", "narrow"):
                rows.append(MppiRow(K, T, seed, tick, UL_VAR, UR_VAR, sampler, shard))
    K, T = MPPI_LARGE
    rows.append(MppiRow(K, T, 77, 1, UL_VAR, UR_VAR, "wide", None))
    rows.append(MppiRow(K, T, HIGH_SEED, HIGH_TICK, UL_VAR, UR_VAR, "narrow", (2 * K + 1, 5 * K)))
    return rows


MPPI_ROWS = _mppi_rows()


def mppi_horizon(T):
    """A horizon that tbnav_mppi_create turns into T steps of MPPI_DT (it truncates horizon / dt: half a step above T is safe)."""
    return (T + 0.5) * MPPI_DT


OK3 = (True, True, True)
RBPF_ROWS = [
    RbpfRow("one-particle-7-normals", 1, 1, OK3, None, None, None),                 # 7 normals: the last pair is used by half
    RbpfRow("two-particles", 2, 1, OK3, 77, None, None),
    RbpfRow("high-seed", 5, 2, OK3, HIGH_SEED, None, None),
    RbpfRow("icp-alternating", 33, 7, (True, False, True), 4242, None, None),       # 3 normals per particle on the failed scan
    RbpfRow("icp-failed-first", 33, 7, (False, True, False), 4242, None, None),
    RbpfRow("reseed-mid-run", 5, 2, OK3, 9, None, (2, 10)),                          # the third scan is scan 0 of seed 10
    RbpfRow("reseed-same-seed", 5, 2, OK3, 9, None, (1, 9)),                         # the second scan repeats the first one's stream
    # stride 9: first_particle 1 -> base 9 (odd: the first element is the odd half of a pair), 2 -> base 18 (even);
    # the offset is element particles_global * 9: 63 (odd) and 72 (even), and 81 with the even base
    RbpfRow("shard-odd-base-odd-offset", 5, 2, OK3, 77, (1, 7), None),
    RbpfRow("shard-even-base-even-offset", 5, 2, OK3, 77, (2, 8), None),
    RbpfRow("shard-even-base-odd-offset", 5, 2, OK3, HIGH_SEED, (2, 9), None),
    RbpfRow("shard-odd-base-even-offset", 5, 2, OK3, 77, (1, 6), None),
]


def rbpf_stride(row, scan):
    return 3 * row.k + 3 if row.icp[scan] else 3


def rbpf_schedule(row):
    """(seed, scan count) of each of the row's SLAM calls."""
    seed = RBPF_DEFAULT_SEED if row.seed is None else row.seed
    out, count = [], 0
    for s in range(len(row.icp)):
        if row.reseed is not None and row.reseed[0] == s:
            seed, count = row.reseed[1], 0
        out.append((seed, count))
        count += 1
    return out
