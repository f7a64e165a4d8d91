"""The case table of everything an RBPF scan does after the proposal: the weights' normalise / Neff / low-variance selection
(csrc/rbpf_normalize.hpp: normalize_body, in its two homes — the kernel rbpf_normalize and workgroup 0 of rbpf_raycast_box), the
run-length count children[], the resampling copies (rbpf_resample_apply = resample_tables_body + gather_body), rbpf_gather_weights
and rbpf_argmax / rbpf_export_map.  Plain data and the rules restated; all of it is integer or order-exact arithmetic whose
specification is the host's sequential tbnav_rbpf_resample_global (rtn_amd.rbpf.resample_global), so every comparison is `==`.
tests/test_resample_cases.py proves the table on the CPU (each case reaches what it names); tests/test_rbpf_resample_gpu.py runs it
on the device.

A normalise run: every particle of the filter is the same particle (one pose, one map) and is handed the SAME normals, so the scan
multiplies every prior weight by one and the same eta: weight_raw = fl(prior * eta) keeps the prior's shape to an ulp, which is what
lets a shape such as `every-once` (margins of 1 / N^2) survive the scan.  The check itself reads the device's own weight_raw.

No library is imported at module level (numpy alone)."""
import numpy as np

K_NORM_CHUNK = 2048               # rbpf_plan.hpp: kNormChunk
K_RESAMPLE_THREADS = 1024         # kResampleThreads
K_RESAMPLE_BLOCKS = 8192          # resample_on_device: the table loop's workgroups, at most
K_TS = 32                         # kTS: 32 x 32-cell tiles
ARGMAX_THREADS = 256

# the register blocks of 16 and 32 (seq_sum, the prefix loop), the 256-thread stride, the chunk of 2048 either side, two chunks + 1
SIZES = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 255, 256, 257, 2047, 2048, 2049, 4096, 4097)
Z_VALUES = (-2.5, 0.3, 2.5)       # -2.5: the first slots all choose parent 0; +2.5: the last slots run past cs[N - 1] and are clamped
FORMS = ("ride-512", "ride-1024", "own-ordered", "own-timing")
SHAPES = ("uniform", "dominant-0", "dominant-third", "dominant-last", "two-heavy", "lognormal", "half-zero", "last", "every-once", "dyadic")
EVERY_ONCE_MIN_N = 16             # `every-once` exists at even N from here on (see prior)


# ---- the rules, restated --------------------------------------------------------------------------------------------------------------
def decision(sq_sum, N):
    """normalize_body / tbnav_rbpf_resample_global: neff = (int)(1.0 / sq); resampled = neff < N / 2 with integer division."""
    neff = int(1.0 / sq_sum)
    return neff, int(neff < N // 2)


def can_resample(N):
    """sq <= 1 for normalised non-negative weights, so neff >= 1: N / 2 must be at least 2."""
    return N // 2 >= 2


def chunks(N):
    return (N + K_NORM_CHUNK - 1) // K_NORM_CHUNK


def normalise_home(form):
    """Where normalize_body runs for a handle set up as `form` (csrc/rbpf.hip: scan_enqueue's `overlap`, launch_raycast; csrc/rbpf_plan.hpp: plan_raycast): riding as
    workgroup 0 of rbpf_raycast_box when overlap holds and the box kernel runs; else rbpf_normalize, a launch of its own.
    Returns (home, the raycast kernel's name — whole for the beam-ordered kernel, up to the thread count for the box —, raycast workgroups minus N)."""
    timing = form == "own-timing"
    ordered = form == "own-ordered"
    overlap = not timing                       # (never local-only here)
    if ordered:
        return "rbpf_normalize", "rbpf_raycast", 0
    nt = 1024 if form == "ride-1024" else 512
    return ("rbpf_raycast_box" if overlap else "rbpf_normalize"), f"rbpf_raycast_box<{nt}, ", (1 if overlap else 0)


def setup(pf, capi, form):
    """Makes the handle take `form`."""
    if form == "own-ordered":
        pf.setOption(capi.RBPF_OPT_RAYCAST_ORDERED, 1)
    else:
        pf.setOption(capi.RBPF_OPT_RAYCAST_THREADS, 1024 if form == "ride-1024" else 512)
    if form == "own-timing":
        pf.setTiming(True)


def table_trips(N, TT):
    """Trips of resample_tables_body's loop for the workgroup that makes most."""
    n = N * TT
    blocks = min((n + K_RESAMPLE_THREADS - 1) // K_RESAMPLE_THREADS, K_RESAMPLE_BLOCKS)
    per_trip = blocks * K_RESAMPLE_THREADS
    return (n + per_trip - 1) // per_trip


def smallest_n_with_two_trips(TT):
    return K_RESAMPLE_BLOCKS * K_RESAMPLE_THREADS // TT + 1


def argmax_restated(w):
    """particle_filter.cpp:260-267: strict '>', starting from 0.0 — the lowest index among the maxima, 0 if no weight is positive."""
    best, bi = 0.0, 0
    for i, v in enumerate(np.asarray(w, dtype=np.float64).tolist()):
        if v > best:
            best, bi = v, i
    return bi


def tiles_nonzero(log_odds, cells):
    """Number of 32 x 32 tiles of a map that hold a non-zero cell (tests/test_rbpf_tiles_gpu.py's count)."""
    pad = (-cells) % K_TS
    side = (cells + pad) // K_TS
    nz = np.pad(np.asarray(log_odds).reshape(cells, cells) != 0.0, ((0, pad), (0, pad)))
    return int(nz.reshape(side, K_TS, side, K_TS).any(axis=(1, 3)).sum())


# ---- prior weights --------------------------------------------------------------------------------------------------------------------
def prior(shape, N):
    """What setParticles(w=...) installs before the scan (None: the shape does not exist at this N)."""
    rng = np.random.default_rng(1000 + N)
    idx = np.arange(N)
    if shape == "uniform":
        return np.full(N, 1.0 / N)
    if shape.startswith("dominant-"):
        at = {"0": 0, "third": N // 3, "last": N - 1}[shape[9:]]
        return np.where(idx == at, 1.0, rng.random(N) * 1e-9)
    if shape == "two-heavy":
        if N < 3:
            return None
        w = np.full(N, 1e-3 / N); w[N // 4] = 0.7; w[(2 * N) // 3] = 0.2
        return w
    if shape == "lognormal":          # 20 orders of magnitude between -3 and +3 sigma
        return np.exp(rng.normal(0.0, 8.0, N))
    if shape == "half-zero":
        w = np.where(rng.random(N) < 0.5, 0.0, rng.random(N))
        if N >= 2:
            w[N // 2] = 0.0
        w[0] = max(w[0], 0.25)
        return w
    if shape == "last":               # the selection's walk reaches the end for every slot but those with U <= 0: clamped at N - 1
        w = np.zeros(N); w[N - 1] = 1.0
        return w
    if shape == "every-once":
        # z = 0: U_m = m t with t = 1 / (N - 1).  The running sums sit at  m t + d  (m even) and  (m + 1) t - d  (m odd), the last at 1:
        # cs[m - 1] < U_m <= cs[m] for every m, so every parent is chosen exactly once — and with d = t / (64 N) the weights alternate
        # between ~0 and ~2 t, so Neff ~ N / 2 - 1 / 4 and the filter DOES resample (uniform weights never would).  Even N only: the sum
        # of squares of such a vector is below 2 / (N - 1), so at odd N Neff >= (N - 1) / 2 = N / 2 and nothing is resampled.
        if N < EVERY_ONCE_MIN_N or N % 2:
            return None
        t = 1.0 / (N - 1)
        d = t / (64.0 * N)
        cs = np.where(idx % 2 == 0, idx * t + d, (idx + 1) * t - d)
        cs[N - 1] = 1.0
        return np.diff(cs, prepend=0.0)
    if shape == "dyadic":             # every add a tie candidate
        return np.ldexp(rng.integers(1, 1 << 12, N).astype(np.float64), -int(np.ceil(np.log2(max(N, 2))) + 20))
    raise KeyError(shape)


def z_values(shape):
    return (0.0,) if shape == "every-once" else Z_VALUES


def normalise_runs(N):
    """(shape, prior, z) of every run at N."""
    out = []
    for shape in SHAPES:
        w = prior(shape, N)
        if w is not None:
            out += [(shape, w, z) for z in z_values(shape)]
    return out


# ---- parent lists for tbnav_rbpf_gather_local (any list, sorted or not; the host counts the children) -------------------------------------
def parent_lists(N):
    assert N >= 6
    idx = np.arange(N, dtype=np.int32)
    counts = np.array([2] * (N - 3) + [0, 0] + [1], dtype=np.int32)      # children: [2] = N - 3, [0] = 2, [1] = 1, the others 0
    keep = idx.copy(); keep[::2] = -1; keep[1] = 0; keep[3] = 2         # slots 0, 2, 4, ... keep their content; 1 <- 0, 3 <- 2
    return {"identity": idx.copy(), "all-to-0": np.zeros(N, dtype=np.int32), "all-to-last": np.full(N, N - 1, dtype=np.int32),
            "reversal": idx[::-1].copy(), "counts": counts, "keep": keep}


def resolve(parents):
    """What tbnav_rbpf_gather_local makes of a list: -1 -> the slot itself; and the children it counts."""
    p = np.asarray(parents, dtype=np.int64).copy()
    p[p < 0] = np.flatnonzero(p < 0)
    return p, np.bincount(p, minlength=p.size)


# ---- arg-max cases -------------------------------------------------------------------------------------------------------------------
ARGMAX_SIZES = (1, 2, 255, 256, 257, 1000, 2049)


def argmax_cases(N):
    """name -> weights.  rbpf_argmax: thread i % 256 scans index i; an LDS tree then folds thread t + off into thread t.
    `cross`: two maxima, the lower index in the HIGHER thread (6 and 261 -> threads 6 and 5) — only the index tie-break gets it right;
    `stride`: two maxima in one thread's stride (5 and 261 -> thread 5): the strict '>' of the scan keeps the first."""
    out = {}
    rng = np.random.default_rng(77 + N)
    base = rng.random(N) * 0.5

    def maxima(*at):
        w = base.copy(); w[list(at)] = 0.75
        return w
    if N >= 262:
        out["cross"] = maxima(6, 261)
        out["stride"] = maxima(5, 261)
        out["cross-3"] = maxima(200, 261, 300 if N > 300 else 262)
    elif N == 257:
        out["cross"] = maxima(1, 256)
        out["stride"] = maxima(0, 256)
    if N >= 3:
        out["pair"] = maxima(N // 3, N - 1)
        out["tree"] = maxima(min(N, 256) - 1, min(N, 256) // 2)      # both in the tree's upper half at its first step
    if N >= 2:
        out["all-equal"] = np.full(N, 0.125)
    out["only-last"] = maxima(N - 1)
    out["zeros"] = np.zeros(N)
    w = np.zeros(N); w[N // 2] = 5e-324
    out["denormal"] = w
    return out
