"""Everything an RBPF scan does after the proposal, on the device, against the host's sequential loops — every comparison `==`
(tests/resample_cases.py is the table, tests/test_resample_cases.py shows on the CPU what each case reaches):
  a. normalize_body in its two homes and four code paths (riding in rbpf_raycast_box<512 | 1024, ...> as workgroup 0: PAR = false, one
     chunk or many; rbpf_normalize behind the beam-ordered kernel or with event timing on: PAR = true), sums, Neff, decision, parents,
     children[] and the gathered weights against rtn_amd.rbpf.resample_global of the device's own weight_raw;
  c. resample_tables_body's three count paths through tbnav_rbpf_gather_local: tiles in use after every list equal the tiles of the
     maps that survive, every slot holds its parent's content;
  d. gather_body's copy of the stored distance field (chunks > 1);
  e. rbpf_argmax's tie rule and rbpf_export_map of a shared table."""
import numpy as np
import pytest

import oracle_api as orc
import rbpf_cases as rc
import resample_cases as rsc

pytestmark = pytest.mark.gpu

K = 4
INC = (0.002, 0.003, 0.002)
ROOM_CORNER = (-0.5, 0.45, -0.45, 0.6)      # a room that straddles the tile border at x = -0.4 m of the 80-cell map from some poses only


def _dev(gpu_pkg, pool_bytes=0, df_mode=None, **kw):
    from rtn_amd.rbpf import ParticleFilter, default_params
    return ParticleFilter(default_params(**kw), pool_bytes=pool_bytes, df_mode=df_mode)


_RUN = {}


def _trajectory(n):
    """n scans of a robot creeping through ROOM_SMALL (the filters start at -INC: the particles' frame is the world's)."""
    if n not in _RUN:
        steps, poses = rc.trajectory(n, inc=INC)
        rng = np.random.default_rng(11)
        _RUN[n] = (steps, [orc.room_scan(poses[s], walls=rc.ROOM_SMALL, rng=rng) for s in range(n)])
    return _RUN[n]


# ---- a. normalise and selection in every home -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", rsc.SIZES)
@pytest.mark.parametrize("form", rsc.FORMS)
def test_normalise_selection_children_and_weights_equal_the_host_loops_bit_for_bit(gpu_pkg, form, N):
    from rtn_amd import capi
    from rtn_amd.rbpf import resample_global
    runs = rsc.normalise_runs(N)
    steps, scans = _trajectory(32)
    assert len(runs) <= len(steps)
    pf = _dev(gpu_pkg, N=N, k=K, pose0=tuple(-v for v in INC))
    rsc.setup(pf, capi, form)
    home, raycast_name, extra = rsc.normalise_home(form)
    block = orc.normal_stream(31, 3 * K + 3, 0.0, 1.0)      # the same normals for every particle: one eta for all (see resample_cases)
    decisions, kids_seen = set(), set()
    for s, (shape, w, z) in enumerate(runs):
        prev, cur, t_icp, u = steps[s]
        normals = np.concatenate([np.tile(block, N), [z]])
        assert normals.size == pf.numNormals(True)
        pf.setParticles(w=w)
        st = pf.SLAM(scans[s], u, cur, prev, True, t_icp, normals)
        assert st.status == 0
        _, raycast, groups = pf.lastKernelNames()
        # (the beam-ordered kernel's name is a prefix of the box kernel's: equality for it, the instantiation's prefix for the box)
        assert (raycast == raycast_name if form == "own-ordered" else raycast.startswith(raycast_name)) and groups == N + extra, (form, N, raycast, groups)
        assert (home == "rbpf_raycast_box") == (groups == N + 1)
        if form == "own-timing":      # the launch of rbpf_normalize itself: its interval between the handle's events
            assert pf.kernelMs()["normalize"] > 0.0
        tr = pf.trace()
        raw = tr["weight_raw"]
        parents, wn, st_h = resample_global(raw, z)
        tag = (form, N, shape, z)
        assert (st.sum_w, st.sq_sum, st.neff, st.resampled) == (st_h.sum_w, st_h.sq_sum, st_h.neff, st_h.resampled), (tag, st.sum_w - st_h.sum_w, st.sq_sum - st_h.sq_sum)
        w_after = pf.particles()[2]
        assert np.array_equal(tr["resample_idx"], parents), tag       # (identity when nothing was resampled)
        if st.resampled:
            kids = pf.children()
            assert np.array_equal(kids, np.bincount(parents, minlength=N)), tag
            kids_seen |= set(np.minimum(kids, 2).tolist())
        assert np.array_equal(w_after, wn[parents]), tag              # the parents' normalised weights: not reset (particle_filter.cpp:495)
        decisions.add(int(st.resampled))
        # the shapes survive the scan's common factor: what the CPU test shows of the priors holds of the device's weights
        if shape == "every-once":
            assert st.resampled == 1 and np.array_equal(parents, np.arange(N)), tag
        if shape == "last":
            assert (raw[:-1] == 0.0).all() and raw[-1] > 0.0
        if shape.startswith("dominant") and rsc.can_resample(N):
            assert st.resampled == 1, tag
    assert decisions == ({0, 1} if rsc.can_resample(N) else {0})
    assert not rsc.can_resample(N) or kids_seen == {0, 1, 2}
    pf.close()


def test_gather_weights_hands_every_slot_its_global_parent_s_normalised_weight(gpu_pkg):
    """rbpf_gather_weights behind the stand-alone kernel (the sharded filter's order of calls): 300 slots (two workgroups of the
    kernel), parents anywhere in a global vector of 5000."""
    import ctypes as C
    import torch
    from rtn_amd import capi
    from rtn_amd.rbpf import resample_global
    N, n = 300, 5000
    pf = _dev(gpu_pkg, N=N, k=2)
    w = rsc.prior("lognormal", n)
    parents_h, wn_h, st_h = resample_global(w, 0.3)
    assert st_h.resampled
    dw = torch.from_numpy(w).cuda()
    parents_d, st = np.empty(n, dtype=np.int32), capi.RbpfStats()
    capi.check(pf._L.tbnav_rbpf_resample_global_dev(pf._h, dw.data_ptr(), n, 1000, C.c_double(0.3), parents_d.ctypes.data, C.byref(st)), "resample_global_dev")
    assert np.array_equal(parents_d, parents_h)
    assert np.array_equal(pf.particles()[2], wn_h[1000:1000 + N])       # this shard's slice of the normalised vector
    gp = np.ascontiguousarray(np.concatenate([parents_h[1000:1000 + N - 3], [0, n - 1, 2048]]), dtype=np.int32)
    capi.check(pf._L.tbnav_rbpf_set_weights_from_global_dev(pf._h, gp.ctypes.data), "set_weights_from_global_dev")
    assert np.array_equal(pf.particles()[2], wn_h[gp])
    pf.close()


# ---- c. tables and reference counts ----------------------------------------------------------------------------------------------------
def _snapshot(pf, slots):
    pose, prev, w = pf.particles()
    nocc = pf.occupiedCount()
    return {m: (pf.logOdds(m), int(nocc[m]), pose[m].copy(), prev[m].copy(), float(w[m])) for m in slots}


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4]


class _Pool:
    """The model the counts are held to.  Every slot holds one map `ident`; a list makes slot m hold its parent's; a scan that writes
    every tile its map had (the same scan from the same pose) leaves every slot with a private map of its own, while the tiles of a
    map that two or more slots shared stay named by the shed notes until the next list settles them."""

    def __init__(self, pf):
        self.pf, self.N, self.cells = pf, pf.N, pf.xsize
        self.cap = pf.poolStats()[0]
        self.ident = list(range(self.N))
        self.next_id = self.N
        self.T = {}
        self.held = 0

    def used(self):
        return self.cap - self.pf.poolStats()[1]

    def measure(self):
        for m, i in enumerate(self.ident):
            if i not in self.T:
                self.T[i] = rsc.tiles_nonzero(self.pf.logOdds(m), self.cells)

    def expect(self):
        return sum(self.T[i] for i in set(self.ident)) + self.held

    def scan(self, scan):
        shared = {i for i in set(self.ident) if self.ident.count(i) > 1}
        self.held = sum(self.T[i] for i in shared)
        self.pf.integrateScanMany(scan, self.pf.particles()[0])
        self.ident = list(range(self.next_id, self.next_id + self.N))
        self.next_id += self.N
        self.measure()

    def apply(self, parents, tag):
        before = _snapshot(self.pf, range(self.N))
        self.pf.gatherLocal(parents)
        p, kids = rsc.resolve(parents)
        assert np.array_equal(self.pf.children(), kids), tag
        after = _snapshot(self.pf, range(self.N))
        for m in range(self.N):
            assert _same(after[m], before[int(p[m])]), (tag, m)
        self.ident = [self.ident[int(q)] for q in p]
        self.held = 0
        assert self.used() == self.expect(), (tag, self.used(), self.expect())


@pytest.mark.parametrize("lists", ["one-free-list", "sixteen-free-lists"])
def test_tiles_in_use_after_every_list_are_the_tiles_of_the_maps_that_survive(gpu_pkg, monkeypatch, lists):
    """resample_tables_body through tbnav_rbpf_gather_local: children == 1 (nothing to count), the plain store on a private tile (new
    count, or back to the pool), the one atomic add on a shared tile (a slot that dies while its siblings live on frees nothing), and the
    shed notes of a scan.  The pool holds 144 tiles: one free list, or sixteen of 9 with the TBNAV_POOL_SHARD_MIN hook."""
    import ctypes as C
    if lists == "sixteen-free-lists":
        monkeypatch.setenv("TBNAV_POOL_SHARD_MIN", "32")
    N = 8
    pf = _dev(gpu_pkg, N=N, k=K)
    L = rsc.parent_lists(N)
    pool = _Pool(pf)
    assert pool.cap == 2 * N * 9 and pool.used() == 0
    # how many lists a pool of this size is put on (create and the self-test ask the same pool_lists_for): one caller popping four
    # tiles from a fresh pool gets neighbours from one list, and ids sixteen apart from list 0 of sixteen
    ids, f_pop, f_push = np.zeros(4, dtype=np.uint32), C.c_uint64(0), C.c_uint64(0)
    assert pf._L.tbnav_rbpf_pool_selftest(pool.cap + 1, 1, 1, 4, 1, ids.ctypes.data, C.addressof(f_pop), C.addressof(f_push)) == 0
    assert np.diff(ids.astype(np.int64)).tolist() == [16 if lists == "sixteen-free-lists" else 1] * 3, ids
    scan = orc.room_scan((0.0, 0.0, 0.0), walls=ROOM_CORNER, rng=np.random.default_rng(2))
    shift = np.array([(0.0, -0.05 + 0.05 * (m % 4), -0.1 + 0.05 * (m // 2)) for m in range(N)])
    rng = np.random.default_rng(4)
    w = rng.random(N); w /= w.sum()
    pf.setParticles(prev=rng.random((N, 3)), w=w)
    pf.integrateScanMany(scan, shift)
    pool.measure()
    assert len(set(pool.T.values())) >= 2 and pool.used() == sum(pool.T.values())         # every tile private, the maps of different sizes
    pool.apply(L["identity"], "identity")                                                     # children == 1 everywhere: the skipped branch
    pool.apply(L["reversal"], "reversal")
    pool.apply(L["counts"], "counts")                                                         # 0, 1, 2 and N - 3 children
    assert len(set(pool.ident)) == 3
    pool.apply([1, 1, 1, N - 3, N - 3, N - 1, N - 1, N - 1], "siblings-live-on")             # slots die, every map lives on: nothing is freed
    assert len(set(pool.ident)) == 3
    before = pool.used()
    pool.scan(scan)                                                                           # every slot clones every tile it shares
    assert pool.held == before and pool.used() == pool.expect() == before + sum(pool.T[i] for i in pool.ident)
    pool.apply(L["keep"], "keep")                                                             # the shed notes are settled; slots 1 and 3 die
    assert len(set(pool.ident)) == N - 2
    pool.scan(scan)
    pool.apply(L["counts"], "counts-after-scan")
    pool.apply(L["all-to-0"], "all-to-0")
    pool.scan(scan)
    pool.apply(L["all-to-last"], "all-to-last")
    assert pool.used() == rsc.tiles_nonzero(pf.logOdds(N - 1), pf.xsize) > 0
    pf.close()


def _tile_numbers(log_odds, cells):
    """The table indices t = row * TW + column of the 32 x 32 tiles of a map that hold a non-zero cell."""
    pad = (-cells) % rsc.K_TS
    side = (cells + pad) // rsc.K_TS
    nz = np.pad(np.asarray(log_odds).reshape(cells, cells) != 0.0, ((0, pad), (0, pad)))
    return np.flatnonzero(nz.reshape(side, rsc.K_TS, side, rsc.K_TS).any(axis=(1, 3)))


def test_the_table_loop_s_second_trip_copies_counts_and_frees_like_the_first(gpu_pkg):
    """N * TT > 8192 workgroups x 1024 threads: on a 400 x 400 map (TT = 169) the smallest such N is 49 637, and the second trip is
    the last slot's table from t = 124 on.  Slots N - 1 and N - 2 stand 6.5 m out along both axes, so every tile of their maps is
    t = 126 or beyond: all that slot N - 1 owns is second-trip work.  List 1 lets slot N - 1 die and take N - 2's map (the trip copies
    non-zero ids and frees a dead slot's private tiles); a scan then clones what the two share; list 2 makes everybody a copy of
    N - 1 (the trip stores the new count of private tiles and settles shed notes).  The tiles in use are exact after each."""
    TT = 169
    N = rsc.smallest_n_with_two_trips(TT)
    assert N == 49637 and rsc.table_trips(N, TT) == 2 and rsc.table_trips(N - 1, TT) == 1
    first_t = rsc.K_RESAMPLE_BLOCKS * rsc.K_RESAMPLE_THREADS - (N - 1) * TT
    assert first_t == 124
    pf = _dev(gpu_pkg, pool_bytes=3 << 30, N=N, k=2, map_min=-10.0, map_max=10.0)
    assert pf.xsize == 400
    cap = pf.poolStats()[0]
    used = lambda: cap - pf.poolStats()[1]
    scan = orc.room_scan((0.0, 0.0, 0.0), walls=ROOM_CORNER, rng=np.random.default_rng(2))
    # the tile border at cell 192 is x = -0.4 m here too; five classes of pose, on and off that border; the last two slots far out
    cls = np.arange(N) % 5
    poses = np.stack([np.zeros(N), np.array([-0.05, 0.15, 0.0, 0.15, 0.05])[cls], np.array([-0.1, 0.1, 0.1, -0.1, 0.0])[cls]], 1)
    poses[N - 1] = (0.0, 6.5, 6.5)
    poses[N - 2] = (0.0, 6.45, 6.6)
    pf.integrateScanMany(scan, poses)
    T_old = np.array([rsc.tiles_nonzero(pf.logOdds(c), 400) for c in range(5)])[cls]      # tiles of every slot's map
    lo_a, lo_b = pf.logOdds(N - 1), pf.logOdds(N - 2)
    for lo, m in ((lo_a, N - 1), (lo_b, N - 2)):
        t = _tile_numbers(lo, 400)
        assert t.size >= 2 and t.min() >= first_t + 2, (m, t)
        T_old[m] = t.size
    assert not np.array_equal(lo_a, lo_b) and len(set(T_old[:5].tolist())) >= 2 and used() == int(T_old.sum())
    # ---- list 1
    idx = np.arange(N)
    parents = ((idx * 7919) % (N // 3)).astype(np.int32)      # unsorted; two thirds of the particles die
    parents[N - 1] = N - 2                                    # the last slot dies (nobody names it) and takes its neighbour's map ...
    parents[N - 2] = N - 2                                    # ... which that neighbour keeps
    kids = np.bincount(parents, minlength=N)
    assert kids[N - 1] == 0 and kids[N - 2] == 2
    watch = [0, 1, 2, N // 3, N - 2, N - 1]
    before = _snapshot(pf, sorted({int(parents[m]) for m in watch}))
    pf.gatherLocal(parents)
    assert np.array_equal(pf.children(), kids)
    after = _snapshot(pf, watch)
    for m in watch:
        assert _same(after[m], before[int(parents[m])]), m
    assert np.array_equal(after[N - 1][0], lo_b) and _tile_numbers(after[N - 1][0], 400).min() >= first_t      # non-zero ids came through the second trip
    assert used() == int(T_old[kids > 0].sum())               # ... and slot N - 1's own tiles went back to the pool in it
    # ---- a scan from the same poses: every slot that shares a map clones all of it; the shared tiles stay named by the shed notes
    pf.integrateScanMany(scan, pf.particles()[0])
    assert used() == int(T_old[parents].sum() + T_old[kids > 1].sum())
    want = pf.logOdds(N - 1)
    assert not np.array_equal(want, lo_b) and np.array_equal(_tile_numbers(want, 400), _tile_numbers(lo_b, 400))
    # ---- list 2
    pf.gatherLocal(np.full(N, N - 1, dtype=np.int32))
    assert used() == _tile_numbers(want, 400).size == T_old[N - 2]
    for m in (0, N // 2, N - 2, N - 1):
        assert np.array_equal(pf.logOdds(m), want), m
    pf.close()


# ---- d. the gather's copy of the stored field -------------------------------------------------------------------------------------------
def _spread_filter(gpu_pkg, df_mode, N=6):
    """One scan of six particles at poses of their own on a 140 x 140 map (G / 4 / 2048 = 2 chunks of the code copy)."""
    pf = _dev(gpu_pkg, df_mode=df_mode, N=N, k=K, map_min=-3.5, map_max=3.5, pose0=(-0.04, -0.03, -0.02))
    assert pf.G == 140 * 140 and pf.G // 4 // 2048 == 2
    steps, poses = rc.trajectory(1, inc=(0.04, 0.03, 0.02))
    prev, cur, t_icp, u = steps[0]
    pose = np.array([(-0.04 + 0.01 * m, -0.03 + 0.1 * m, -0.02 - 0.08 * m) for m in range(N)])
    pf.setParticles(pose=pose)
    scan = orc.room_scan(poses[0], walls=rc.ROOM_SMALL, rng=np.random.default_rng(6))
    st = pf.SLAM(scan, u, cur, prev, True, t_icp, orc.normal_stream(8, pf.numNormals(True), 0.0, 1.0))
    assert st.status == 0 and st.resampled == 0
    return pf


@pytest.mark.parametrize("mode", ["full", "window"])
def test_a_stored_field_travels_with_its_particle_in_the_stored_field_modes(gpu_pkg, mode):
    pf = _spread_filter(gpu_pkg, mode)
    N = pf.N
    codes = [pf.distCode(m).copy() for m in range(N)]
    assert all(not np.array_equal(codes[0], c) for c in codes[1:])
    for parents in ([3, 3, 0, 5, 1, 1], [5, 4, 3, 2, 1, 0]):
        pf.gatherLocal(parents)
        now = [pf.distCode(m).copy() for m in range(N)]
        for m in range(N):
            assert np.array_equal(now[m], codes[parents[m]]), (mode, parents, m)
        codes = now
    pf.close()


def test_the_reference_field_travels_with_its_particle_across_a_resample_on_a_map_of_two_chunks(gpu_pkg):
    """The reference-field mode keeps state in the stored codes (the brushfire's order-dependent result) and copies them for every
    slot, whatever its field state.  140 x 140 cells (two chunks a slot), 40 particles, a forced resample at scan 3 of 6: every slot's
    field and map are the oracle filter's afterwards, bit for bit."""
    from test_rbpf_field_gpu import _free_run
    N = 40
    pf_o, pf_d, rows = _free_run(gpu_pkg, "reference", N=N, k=K, map_half=3.5, walls=rc.ROOM_SMALL, n_scans=6, inc=(0.04, 0.03, 0.02),
                                 seed=3, force_resample_at=3)
    assert pf_d.G // 4 // 2048 == 2 and rows[3]["resampled"] == (1, 1) and rows[3]["parents_equal"]
    fields = []
    for p in range(N):
        g = pf_o.grid(p).dump()
        assert np.array_equal(pf_d.occDist(p), g["occ_dist"]), p
        assert np.array_equal(pf_d.logOdds(p), g["log_odds"]), p
        fields.append(g["occ_dist"])
    assert any(not np.array_equal(fields[0], f) for f in fields[1:])
    pf_d.close(); pf_o.close()


def test_an_injected_field_travels_and_a_plain_slot_stays_plain_in_query_mode(gpu_pkg):
    """Query mode copies a slot's codes only where they are authoritative (field state 2).  Slots 0-2 get a made-up field injected,
    slots 3-5 stay plain; the list maps injected -> plain and plain -> injected.  A slot that took an injected parent reads that very
    field back; a slot that took a plain parent is plain — its field, worked out on demand, is its NEW map's (a twin filter's)."""
    pf, twin = _spread_filter(gpu_pkg, None), _spread_filter(gpu_pkg, None)
    N, G = pf.N, pf.G
    rng = np.random.default_rng(9)
    fake = [np.sqrt(rng.integers(0, 400, G).astype(np.float64)) * 0.05 for _ in range(3)]
    for m in range(3):
        pf.setOccDist(m, fake[m])
    parents = [4, 5, 1, 0, 2, 3]
    pf.gatherLocal(parents)
    for m in range(N):
        q = parents[m]
        if q < 3:
            assert np.array_equal(pf.occDist(m), fake[q]), m
        else:
            assert np.array_equal(pf.distCode(m), twin.distCode(q)), m
            assert np.array_equal(pf.logOdds(m), twin.logOdds(q))
    pf.close(); twin.close()


# ---- e. rbpf_argmax and rbpf_export_map ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", rsc.ARGMAX_SIZES)
def test_arg_max_is_the_lowest_index_among_the_maxima_and_0_without_a_positive_weight(gpu_pkg, N):
    pf = _dev(gpu_pkg, N=N, k=2)
    pf_o = orc.PfAPI(orc.pf_params(N=N, k=2, map_min=-0.5, map_max=0.5))
    pose = np.random.default_rng(N).random((N, 3))
    pf.setParticles(pose=pose)
    for name, w in rsc.argmax_cases(N).items():
        pf.setParticles(w=w)
        pf_o.set_particles(w=w)
        got_pose, got = pf.getRobotState()
        assert got == pf_o.best() == rsc.argmax_restated(w), (N, name, got)
        assert np.array_equal(got_pose, pose[got])
    pf.close(); pf_o.close()


@pytest.mark.parametrize("N", [40, 300, 2049])
def test_arg_max_after_a_real_resample_picks_the_first_child_of_the_best_parent(gpu_pkg, N):
    """Weights are not reset at a resample: all children of the best parent tie, the lowest slot wins."""
    pf = _dev(gpu_pkg, N=N, k=K, pose0=tuple(-v for v in INC))
    steps, scans = _trajectory(32)
    prev, cur, t_icp, u = steps[0]
    pf.setParticles(w=rsc.prior("two-heavy", N))
    normals = np.concatenate([np.tile(orc.normal_stream(31, 3 * K + 3, 0.0, 1.0), N), [-2.5]])     # (z = -2.5: slot 0 stays on parent 0)
    st = pf.SLAM(scans[0], u, cur, prev, True, t_icp, normals)
    assert st.status == 0 and st.resampled == 1
    parents, w = pf.trace()["resample_idx"], pf.particles()[2]
    kids = np.bincount(parents, minlength=N)
    best_parent = N // 4
    assert kids[best_parent] >= 3 and (w == w.max()).sum() == kids[best_parent]
    first = int(np.flatnonzero(parents == best_parent)[0])
    assert first > 0 and pf.getRobotState()[1] == first == rsc.argmax_restated(w)
    pf_o = orc.PfAPI(orc.pf_params(N=N, k=2, map_min=-0.5, map_max=0.5))
    pf_o.set_particles(w=w)
    assert pf_o.best() == first
    pf_o.close(); pf.close()


def test_new_map_of_a_best_slot_whose_table_is_a_shared_copy_is_the_oracle_s_grid_map(gpu_pkg):
    N = 6
    pf = _dev(gpu_pkg, N=N, k=K)
    scan = orc.room_scan((0.0, 0.0, 0.0), walls=rc.ROOM_SMALL, rng=np.random.default_rng(3))
    poses = np.array([(0.0, 0.02 * m, -0.03 * m) for m in range(N)])
    pf.integrateScanMany(scan, poses)
    parents = [0, 4, 4, 4, 1, 2]                 # slots 1, 2, 3 share particle 4's table
    pf.gatherLocal(parents)
    w = np.array([0.1, 0.05, 0.3, 0.3, 0.2, 0.05])    # slots 2 and 3 tie: 2 is the best
    pf.setParticles(w=w)
    (pose, idx) = pf.getRobotState()
    assert idx == 2 and np.array_equal(pose, poses[4])
    g = orc.GridAPI("orc", grid=(0.05, -2.0, 2.0, -2.0, 2.0))
    g.integrate_scan(scan, poses[4], esdf=False)
    assert np.array_equal(pf.newMap(), g.grid_map())
    other = orc.GridAPI("orc", grid=(0.05, -2.0, 2.0, -2.0, 2.0))
    other.integrate_scan(scan, poses[0], esdf=False)
    assert not np.array_equal(g.grid_map(), other.grid_map())       # (the maps can tell the slots apart)
    g.close(); other.close()
    pf.close()
