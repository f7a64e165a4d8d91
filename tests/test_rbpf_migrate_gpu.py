"""A particle moving between handles, byte for byte: tbnav_rbpf_export_* / tbnav_rbpf_import_* (single and batched) and
tbnav_rbpf_copy_particle against the host restatement of tests/migrate_cases.py — rbpf_pack_tiles, rbpf_count_tiles, rbpf_pack_batch
(second compaction trip, waves all named / all empty, codes section), rbpf_blob_headers, rbpf_release_slots (table and shed notes),
rbpf_unpack_batch (full runs, a short last run, scattered runs, the exhausted path, codes section), rbpf_dense_to_tiles and
rbpf_tiles_to_dense (every map goes in through the one and comes out through the other).  Everything is integer or bit-copy work:
`==` throughout."""
import ctypes as C
import os

import numpy as np
import pytest

import migrate_cases as mc
import oracle_api as orc

pytestmark = pytest.mark.gpu

PER_TILE = 8192 + 128 + 4 + 4            # what create budgets per pool tile: log-odds, occupancy bits, count, free-list entry
SMALL_LISTS = 1000                       # pool tiles for the free-list tests: sixteen lists of 62 or 63, none can supply a run of 64


def _pf(grid, N, tiles=0, df_mode=None):
    """A handle on `grid` (pool of `tiles` tiles, 0 = the roomy default), its geometry checked against the case module."""
    from rtn_amd.rbpf import ParticleFilter, default_params
    pf = ParticleFilter(default_params(N=N, k=2, map_min=grid.map_min, map_max=grid.map_max), pool_bytes=tiles * PER_TILE, df_mode=df_mode)
    TW = (pf.xsize + mc.TS - 1) // mc.TS
    assert (pf.xsize, pf.ysize, TW, TW * TW) == (grid.xsize, grid.xsize, grid.TW, grid.TT)
    if grid.id == "B":
        assert TW * TW > 256 and pf.xsize % 32 != 0          # a second compaction trip, partial edge tiles
    if tiles:
        assert pf.poolStats()[0] == tiles - 1                 # (tile 0 is the shared zero tile)
    return pf


def _set_states(pf, salt=0):
    st = [mc.state_of(p, salt) for p in range(pf.N)]
    pf.setParticles(np.array([s[0] for s in st]), np.array([s[1] for s in st]), np.array([s[2] for s in st]))
    return st


def _used(pf):
    cap, free, _ = pf.poolStats()
    assert free <= cap, "a tile was freed twice"
    return cap - free


# ---- the raw calls, through pf._L ----------------------------------------------------------------------------------------------
def _upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _export_size(pf, slot):
    n = C.c_uint64()
    assert pf._L.tbnav_rbpf_export_size(pf._h, int(slot), C.byref(n)) == 0
    return int(n.value)


def _export_one(pf, slot):
    import torch
    n, got = _export_size(pf, slot), C.c_uint64()
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    assert pf._L.tbnav_rbpf_export_particle_dev(pf._h, int(slot), buf.data_ptr(), n, C.byref(got)) == 0 and got.value == n
    return buf.cpu().numpy()


def _export_batch(pf, slots):
    import torch
    slots = np.ascontiguousarray(slots, dtype=np.int32)
    sizes = np.zeros(slots.size, dtype=np.uint64)
    assert pf._L.tbnav_rbpf_export_batch_sizes(pf._h, slots.size, slots.ctypes.data, sizes.ctypes.data) == 0
    buf = torch.zeros(int(sizes.sum()), dtype=torch.uint8, device="cuda")
    offs = np.zeros(slots.size + 1, dtype=np.uint64)
    assert pf._L.tbnav_rbpf_export_batch_dev(pf._h, slots.size, slots.ctypes.data, buf.data_ptr(), buf.numel(), offs.ctypes.data) == 0
    return buf.cpu().numpy(), offs, sizes


def _import_one(pf, slot, blob, nbytes=None):
    dev = _upload(blob)
    return pf._L.tbnav_rbpf_import_particle_dev(pf._h, int(slot), dev.data_ptr(), dev.numel() if nbytes is None else nbytes)


def _import_batch(pf, slots, blobs, offsets=None, nbytes=None):
    """Slot slots[i] takes blobs[i] (the buffer is the blobs back to back), or the blob at offsets[i] of the one buffer `blobs`."""
    slots = np.ascontiguousarray(slots, dtype=np.int32)
    if offsets is None:
        offsets = np.cumsum([0] + [b.size for b in blobs[:-1]])
        blobs = np.concatenate(blobs)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    dev = _upload(blobs)
    return pf._L.tbnav_rbpf_import_batch_dev(pf._h, slots.size, slots.ctypes.data, dev.data_ptr(), dev.numel() if nbytes is None else nbytes,
                                             offsets.ctypes.data)


def _import(pf, slots, blobs, batched):
    """The same import by either call; returns the list of status codes (one for a batch)."""
    if batched:
        return [_import_batch(pf, slots, blobs)]
    return [_import_one(pf, s, b) for s, b in zip(slots, blobs)]


def _snap(pf):
    return dict(maps=[pf.logOdds(p) for p in range(pf.N)], st=pf.particles(), nocc=pf.occupiedCount(), pool=pf.poolStats(),
                blobs=[_export_one(pf, p) for p in range(pf.N)])


def _assert_same(pf, before, slots=None, where=""):
    now = _snap(pf)
    for p in range(pf.N) if slots is None else slots:
        assert np.array_equal(now["maps"][p], before["maps"][p]), (where, p)
        assert all(np.array_equal(a[p], b[p]) for a, b in zip(now["st"], before["st"])), (where, p)
        assert now["nocc"][p] == before["nocc"][p] and np.array_equal(now["blobs"][p], before["blobs"][p]), (where, p)
    if slots is None:
        assert now["pool"] == before["pool"], where


def _assert_holds(pf, slot, blob, grid, where=""):
    """Slot `slot` is exactly the particle of `blob`: map, state, counts, and the bytes it exports again (tile order, tile-row counts,
    header — no hook needed)."""
    want = mc.parse_blob(blob, grid.TW, grid.xsize ** 2)
    assert np.array_equal(pf.logOdds(slot), want["dense"]), (where, slot)
    pose, prev, w = pf.particles()
    assert np.array_equal(pose[slot], want["pose"]) and np.array_equal(prev[slot], want["prev"]) and w[slot] == want["weight"], (where, slot)
    assert pf.occupiedCount()[slot] == want["nocc"], (where, slot)
    assert np.array_equal(_export_one(pf, slot), blob), (where, slot)


def _assert_empty(pf, slot, grid, where=""):
    """Slot `slot` holds the empty map: no tile, no occupied cell, no stored field, every distance unreached."""
    assert not pf.logOdds(slot).any(), (where, slot)
    assert pf.occupiedCount()[slot] == 0, (where, slot, pf.occupiedCount())
    pose, prev, w = pf.particles()
    again = _export_one(pf, slot)
    assert np.array_equal(again, mc.expected_blob(np.zeros(grid.xsize ** 2), grid.xsize, mc.L_OCC, pose[slot], prev[slot], w[slot])), (where, slot)
    p = mc.parse_blob(again, grid.TW, grid.xsize ** 2)
    assert p["n_tiles"] == 0 and not p["trow"].any() and p["has_codes"] == 0 and p["fstate"] == 0
    assert np.all(pf.distCode(slot) == mc.UNREACHED), (where, slot)


# ---- the sources: one handle per grid, one case per slot, everything read from it once ----------------------------------------------
class _Source:
    def __init__(self, grid):
        self.grid = grid
        self.names = list(mc.cases(grid))
        self.pf = pf = _pf(grid, len(self.names))
        assert 4 <= pf.N <= 16
        self.states = _set_states(pf)
        self.dense = [mc.fill(grid, mc.cases(grid)[n], salt=i) for i, n in enumerate(self.names)]
        for i, d in enumerate(self.dense):
            pf.setLogOdds(i, d)
        self.n_tiles = [int(mc.cases(grid)[n].sum()) for n in self.names]
        self.want = [mc.expected_blob(d, grid.xsize, mc.L_OCC, *self.states[i]) for i, d in enumerate(self.dense)]
        # what the exports say, read BEFORE any distance field is asked for (distCode makes a slot's stored field authoritative)
        self.sizes = [_export_size(pf, i) for i in range(pf.N)]
        self.single = [_export_one(pf, i) for i in range(pf.N)]
        ix = self.names.index
        self.order = [ix("all"), ix("empty"), ix("n129")] + [i for i, n in enumerate(self.names) if n not in ("all", "empty", "n129")] + [ix("all")]
        self.batch, self.offs, self.batch_sizes = _export_batch(pf, self.order)
        self.used, self.nocc = _used(pf), pf.occupiedCount()
        self.codes = {n: pf.distCode(ix(n)) for n in ("empty", "one_first", "one_last", "n129")}

    def blob(self, name):
        return self.single[self.names.index(name)]


@pytest.fixture(scope="module")
def sources(gpu_pkg):
    held = {}

    def get(gid):
        if gid not in held:
            held[gid] = _Source(mc.GRIDS[gid])
        return held[gid]
    yield get
    for s in held.values():
        s.pf.close()


# ---- a. export bytes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", ["A", "B"])
def test_exports_are_the_restated_bytes_singly_and_in_one_batch(sources, gid):
    """rbpf_dense_to_tiles named exactly the non-zero tiles; export_size / export_batch_sizes are blob_layout's total; the single export
    (rbpf_pack_tiles) and the batched one (rbpf_count_tiles + rbpf_pack_batch: on grid B the compaction's second trip, the carried
    base, waves whose 64 entries are all named or all empty) write expected_blob byte for byte, the batch back to back with a slot
    listed twice and the empty particle between two large ones."""
    s = sources(gid)
    g = s.grid
    G = g.xsize ** 2
    assert s.used == sum(s.n_tiles)
    for i, name in enumerate(s.names):
        total = mc.blob_layout(g.TW, G, s.n_tiles[i], False).total
        assert s.sizes[i] == total == s.want[i].size, name
        assert s.nocc[i] == mc.occupied_count(s.dense[i]), name
        if not np.array_equal(s.single[i], s.want[i]):
            bad = np.flatnonzero(s.single[i] != s.want[i])
            raise AssertionError(f"{gid}/{name}: the single export differs in {bad.size} bytes, first at {bad[:4].tolist()} "
                                 f"(sections {mc.blob_layout(g.TW, G, s.n_tiles[i], False)})")
    assert s.batch_sizes.tolist() == [s.sizes[i] for i in s.order]
    assert s.offs.tolist() == np.concatenate([[0], np.cumsum(s.batch_sizes)]).tolist()
    for q, i in enumerate(s.order):
        got = s.batch[int(s.offs[q]):int(s.offs[q + 1])]
        if not np.array_equal(got, s.want[i]):
            bad = np.flatnonzero(got != s.want[i])
            raise AssertionError(f"{gid}/{s.names[i]} (item {q} of the batch): {bad.size} bytes differ, first at {bad[:4].tolist()} "
                                 f"(sections {mc.blob_layout(g.TW, G, s.n_tiles[i], False)})")
    assert s.batch.size == int(s.offs[-1])


# ---- b. round trip into a handle that already holds other maps ----------------------------------------------------------------------------------
def _round_trip(s, tiles):
    g = s.grid
    dst = _pf(g, 8, tiles)
    _set_states(dst, salt=1)
    held = {}
    for p in range(8):
        d = mc.fill(g, mc.cases(g)["n65" if p % 2 == 0 else "one_first"], salt=20 + p)
        dst.setLogOdds(p, d)
        held[p] = mc.expected_blob(d, g.xsize, mc.L_OCC, *mc.state_of(p, 1))
    tiles_of = lambda blob: mc.parse_blob(blob, g.TW, g.xsize ** 2)["n_tiles"]  # noqa: E731
    assert _used(dst) == sum(tiles_of(b) for b in held.values())
    # the single call: every case in turn into slot 1 (the largest first, the small ones last)
    for name in sorted(s.names, key=lambda n: -s.n_tiles[s.names.index(n)]):
        assert _import_one(dst, 1, s.blob(name)) == 0, name
        held[1] = s.blob(name)
        _assert_holds(dst, 1, held[1], g, name)
        assert _used(dst) == sum(tiles_of(b) for b in held.values()), name    # before - what slot 1 alone held + the incoming tiles
        for p in (0, 2):
            assert np.array_equal(_export_one(dst, p), held[p]), (name, p)
    # the batch call: one blob into two slots; more than 64 tiles beside 0 and 1 tiles
    into, names = [2, 3, 4, 5, 6], ["n129", "n129", "empty", "one_first", "all"]
    at = {n: int(s.offs[s.order.index(s.names.index(n))]) for n in names}
    assert _import_batch(dst, into, s.batch, offsets=[at[n] for n in names]) == 0
    for p, n in zip(into, names):
        held[p] = s.blob(n)
    for p in range(8):
        _assert_holds(dst, p, held[p], g, "batch")
    assert _used(dst) == sum(tiles_of(b) for b in held.values())
    for p, n in ((2, "n129"), (4, "empty"), (5, "one_first")):
        assert np.array_equal(dst.distCode(p), s.codes[n]), n       # materialised from the imported bits and tile-row counts
    dst.close()


@pytest.mark.parametrize("gid", ["A", "B"])
def test_imports_rebuild_the_particle_and_settle_the_pool(sources, gid):
    """Into slots that hold maps of their own: map, state, counts and the re-exported bytes equal the blob's, tiles in use follow
    exactly, unlisted slots keep theirs.  rbpf_unpack_batch with one run, full runs and a short last run (n63 .. all)."""
    _round_trip(sources(gid), 0)


# ---- c. stored field ------------------------------------------------------------------------------------------------------------------
def test_a_stored_field_travels_with_the_particle_and_lands_in_a_handle_without_one(gpu_pkg):
    g = mc.GRID_A
    G = g.xsize ** 2
    src = _pf(g, 4)
    states = _set_states(src)
    dense = [mc.fill(g, mc.scattered(g, n), salt=40 + i) for i, n in enumerate((5, 66, 7, 0))]
    fields = [mc.stored_field(g, salt=i) for i in range(2)]
    for i in range(4):
        src.setLogOdds(i, dense[i])
    for i in range(2):
        src.setOccDist(i, fields[i][1])          # after the map: a field that is nobody's distance transform, and authoritative
    want = [mc.expected_blob(dense[i], g.xsize, mc.L_OCC, *states[i], fstate=2 if i < 2 else 0, codes=fields[i][0] if i < 2 else None) for i in range(4)]
    blobs = [_export_one(src, i) for i in range(4)]
    batch, offs, sizes = _export_batch(src, [0, 2, 1, 3])
    for i in range(4):
        p = mc.parse_blob(blobs[i], g.TW, G)
        assert (p["has_codes"], p["fstate"]) == ((1, 2) if i < 2 else (0, 0))
        assert i >= 2 or np.array_equal(p["codes"], fields[i][0])
        assert np.array_equal(blobs[i], want[i]), i
    for q, i in enumerate([0, 2, 1, 3]):
        assert np.array_equal(batch[int(offs[q]):int(offs[q + 1])], want[i]), (q, i)      # rbpf_pack_batch's codes section, mixed
    # the single call into a handle on which nothing has touched a distance field: the codes are allocated by the import
    d1 = _pf(g, 4)
    assert _import_one(d1, 3, blobs[1]) == 0
    _assert_holds(d1, 3, blobs[1], g, "single, codes")
    assert np.array_equal(d1.distCode(3), fields[1][0])            # the injected field, not the map's transform
    assert np.array_equal(_export_one(d1, 3), blobs[1])
    d1.close()
    # a batch that mixes both kinds, again into a fresh handle
    d2 = _pf(g, 4)
    assert _import_batch(d2, [2, 0, 1, 3], batch, offsets=offs[:4]) == 0            # slot 2 <- 0 (codes), 0 <- 2, 1 <- 1 (codes), 3 <- 3 (empty)
    for slot, i in ((2, 0), (0, 2), (1, 1), (3, 3)):
        _assert_holds(d2, slot, blobs[i], g, "batch, mixed")
    assert np.array_equal(d2.distCode(2), fields[0][0]) and np.array_equal(d2.distCode(1), fields[1][0])
    occ = (dense[2] >= mc.L_OCC).reshape(g.xsize, g.xsize)
    exact = orc.exact_edt_codes(occ, 200, np.full((g.xsize, g.xsize), mc.UNREACHED, np.uint16))
    assert np.array_equal(d2.distCode(0).reshape(g.xsize, g.xsize), exact)             # no codes came: the true transform of the imported bits
    assert np.all(d2.distCode(3) == mc.UNREACHED)
    # a blob without codes over a slot whose field was authoritative: the slot's field is the new map's again
    assert _import_one(d2, 2, blobs[3]) == 0
    _assert_holds(d2, 2, blobs[3], g, "no codes over codes")
    src.close(); d2.close()


# ---- d. shared tiles and shed notes ----------------------------------------------------------------------------------------------------
def _shared_tiles(s, tiles, batched):
    g = s.grid
    N = 8
    dst = _pf(g, N, tiles)
    cap = dst.poolStats()[0]
    states = _set_states(dst, salt=1)
    d65 = mc.fill(g, mc.cases(g)["n65"], salt=7)
    dst.setLogOdds(0, d65)
    dst.gatherLocal([0] * N)
    assert _used(dst) == 65
    shared = mc.expected_blob(d65, g.xsize, mc.L_OCC, *states[0])
    dst.setLogOdds(2, mc.fill(g, mc.cases(g)["n63"], salt=9))                       # clones every tile it names: 65 shed notes
    assert _used(dst) == 130
    scan = orc.room_scan((0.0, 0.0, 0.0), walls=(-1.6, 1.5, -1.3, 1.7), rng=np.random.default_rng(2))
    dst.integrateScan(3, scan, (0.0, 0.0, 0.0))                                      # clones the shared tiles it writes, takes fresh ones beside
    assert _used(dst) > 130
    names = ["n63", "n64", "one_last"]
    rcs = _import(dst, [1, 2, 3], [s.blob(n) for n in names], batched)
    assert set(rcs) == {0}
    for p, n in zip((1, 2, 3), names):
        _assert_holds(dst, p, s.blob(n), g, n)
    for p in (0, 4, 5, 6, 7):                                                       # the sharers keep n65 exactly ...
        assert np.array_equal(dst.logOdds(p), d65) and dst.occupiedCount()[p] == mc.occupied_count(d65), p
    assert np.array_equal(_export_one(dst, 0), shared)
    assert _used(dst) == 65 + 63 + 64 + 1                                           # ... and no tile of theirs returned, every clone did
    # now every sharer writes: the 65 tiles are named by five shed notes and nothing else; when the slots give everything up, the
    # last note to go must hand each of them back
    for p in (0, 4, 5, 6, 7):
        dst.setLogOdds(p, mc.fill(g, mc.cases(g)["n65"], salt=30 + p))
    assert _used(dst) == 65 + 5 * 65 + 128
    empty = s.blob("empty")
    assert set(_import(dst, list(range(N)), [empty] * N, batched)) == {0}
    assert dst.poolStats()[1] == cap, "a tile leaked (free below cap) or came back twice (above)"
    for p in (0, 3, 7):
        assert not dst.logOdds(p).any()
    dst.close()


@pytest.mark.parametrize("batched", [True, False], ids=["batch", "single"])
def test_shared_tiles_stay_with_their_sharers_and_shed_notes_are_settled(sources, batched):
    _shared_tiles(sources("A"), 0, batched)


# ---- e. the same on sixteen short free lists ----------------------------------------------------------------------------------------------
def test_on_sixteen_short_lists_every_run_is_gathered_tile_by_tile(gpu_pkg, sources, monkeypatch):
    """TBNAV_POOL_SHARD_MIN (a test hook) puts a pool of 1000 tiles on sixteen lists of 62 or 63: no list can supply a run of 64, so
    every full run of rbpf_unpack_batch takes the scattered path (ids parked in the table, read back through nth); the assertions are
    those of the tests above.  Then one import that takes 95 % or more of the free tiles: a request that fits never sees exhaustion."""
    monkeypatch.setenv("TBNAV_POOL_SHARD_MIN", "32")
    # the hook is in force: on sixteen lists caller c pops from list c, whose ids are all c (mod 16); one list hands out 1, 2, 3 ...
    ids, f_pop, f_push = np.zeros(4 * 8, dtype=np.uint32), C.c_uint64(), C.c_uint64()
    assert gpu_pkg.capi.lib().tbnav_rbpf_pool_selftest(SMALL_LISTS, 1, 4, 8, 0, ids.ctypes.data, C.addressof(f_pop), C.addressof(f_push)) == 0
    assert [sorted(set((row % 16).tolist())) for row in ids.reshape(4, 8)] == [[0], [1], [2], [3]], ids
    sa, sb = sources("A"), sources("B")
    _round_trip(sa, SMALL_LISTS)
    _round_trip(sb, SMALL_LISTS)
    _shared_tiles(sa, SMALL_LISTS, True)
    _shared_tiles(sa, SMALL_LISTS, False)
    g = sa.grid
    names = ["all", "n129", "n65"]
    incoming = sum(sa.n_tiles[sa.names.index(n)] for n in names)
    dst = _pf(g, 4, incoming + 8)                      # 363 incoming tiles of 370 free, sixteen lists of 23
    cap, free, _ = dst.poolStats()
    assert free == cap and 0.95 * free <= incoming <= free
    assert _import_batch(dst, [3, 0, 1], [sa.blob(n) for n in names]) == 0
    for p, n in zip((3, 0, 1), names):
        _assert_holds(dst, p, sa.blob(n), g, n)
    assert dst.poolStats()[1] == cap - incoming
    dst.close()


# ---- f. exhaustion ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crowd(gpu_pkg):
    """Blobs for a pool that is too small: four particles of 110 tiles, four of 50 (grid A), their maps beside them."""
    g = mc.GRID_A
    src = _pf(g, 8)
    _set_states(src, salt=3)
    dense = [mc.fill(g, mc.scattered(g, 110 if i < 4 else 50), salt=50 + i) for i in range(8)]
    for i, d in enumerate(dense):
        src.setLogOdds(i, d)
    blobs = [_export_one(src, i) for i in range(8)]
    src.close()
    assert [mc.parse_blob(b, g.TW, g.xsize ** 2)["n_tiles"] for b in blobs] == [110] * 4 + [50] * 4
    return blobs[:4], blobs[4:]


def _tight_handle():
    """N = 8 on a pool of 199 tiles; slot 0 holds 60 tiles and an authoritative stored field, and every slot shares both."""
    g = mc.GRID_A
    dst = _pf(g, 8, 200)
    dst.setLogOdds(0, mc.fill(g, mc.scattered(g, 60), salt=60))
    dst.distCode(0)                               # the whole field, stored and authoritative from here on: it travels with a resample's copies
    dst.gatherLocal([0] * 8)
    _set_states(dst, salt=2)
    cap, free, _ = dst.poolStats()
    assert (cap, free) == (199, 139)
    return dst, cap, free


def _installed_or_empty(dst, slot, blob, where):
    """1 if the slot is exactly the blob's particle, 0 if it holds the empty map; anything else fails."""
    g = mc.GRID_A
    if dst.logOdds(slot).any():
        _assert_holds(dst, slot, blob, g, where)
        return 1
    _assert_empty(dst, slot, g, where)
    return 0


def _one_list():
    return not os.environ.get("TBNAV_POOL_SHARD_MIN")     # (199 tiles keep ONE free list unless the whole suite runs under the hook)


def test_a_batch_beyond_the_bound_is_refused_with_nothing_touched(gpu_pkg, crowd):
    from rtn_amd import capi
    dst, cap, free = _tight_handle()
    before = _snap(dst)
    assert 4 * 110 > free + 4 * 60                          # incoming > free + every tile the four slots name
    assert _import_batch(dst, [1, 2, 3, 4], crowd[0]) == capi.ERR_POOL_EXHAUSTED
    _assert_same(dst, before, where="refused before the release")
    dst.close()


def test_a_batch_that_runs_dry_leaves_each_slot_whole_or_empty(gpu_pkg, crowd):
    """Inside the bound (200 <= 139 + 240), but releasing slots 1-4 frees nothing: slots 0 and 5-7 still share the tiles.
    Before the fix a slot left with "the empty map" kept trow, nocc and fstate of the map it gave up (this test failed on the stale
    occupied count); now the failure branch of rbpf_unpack_batch writes the empty map's."""
    from rtn_amd import capi
    dst, cap, free = _tight_handle()
    before = _snap(dst)
    assert 4 * 50 <= free + 4 * 60
    assert _import_batch(dst, [1, 2, 3, 4], crowd[1]) == capi.ERR_POOL_EXHAUSTED
    _assert_same(dst, before, slots=(0, 5, 6, 7), where="the sharers")
    installed = sum(_installed_or_empty(dst, p, crowd[1][p - 1], "ran dry") for p in (1, 2, 3, 4))
    assert installed <= free // 50 and (installed == free // 50 or not _one_list()), installed
    assert _import_batch(dst, list(range(8)), [mc.expected_blob(np.zeros(160000), 400, mc.L_OCC, (0, 0, 0), (0, 0, 0), 0.5)] * 8) == 0
    assert dst.poolStats()[1] == cap
    dst.close()


def test_the_single_import_that_runs_dry_leaves_the_slot_whole_or_empty(gpu_pkg, crowd):
    """The same situation through tbnav_rbpf_import_particle_dev, slot by slot.  Before the fix the call installed whichever tiles it
    had popped and then copied state, trow and nocc of the whole particle (half a map under the counts of a whole one); now it is
    the batch path with n = 1."""
    from rtn_amd import capi
    dst, cap, free = _tight_handle()
    before = _snap(dst)
    rcs = [_import_one(dst, p, crowd[1][p - 1]) for p in (1, 2, 3, 4)]
    assert set(rcs) <= {0, capi.ERR_POOL_EXHAUSTED} and capi.ERR_POOL_EXHAUSTED in rcs, rcs
    _assert_same(dst, before, slots=(0, 5, 6, 7), where="the sharers")
    installed = 0
    for p, rc_ in zip((1, 2, 3, 4), rcs):
        got = _installed_or_empty(dst, p, crowd[1][p - 1], f"single, rc {rc_}")
        assert got == (1 if rc_ == 0 else 0), (p, rc_, got)
        installed += got
    assert installed <= free // 50 and (installed == free // 50 or not _one_list()), installed
    empty = mc.expected_blob(np.zeros(160000), 400, mc.L_OCC, (0, 0, 0), (0, 0, 0), 0.5)
    assert [_import_one(dst, p, empty) for p in range(8)] == [0] * 8
    assert dst.poolStats()[1] == cap
    dst.close()


# ---- g. refusals ----------------------------------------------------------------------------------------------------------------------
def test_a_bad_blob_or_a_bad_slot_is_refused_and_nothing_is_touched(gpu_pkg, sources):
    sa, sb = sources("A"), sources("B")
    g = sa.grid
    N = 4
    dst = _pf(g, N)
    _set_states(dst, salt=1)
    for p in range(N):
        dst.setLogOdds(p, mc.fill(g, mc.cases(g)["n65" if p % 2 == 0 else "one_first"], salt=20 + p))
    before = _snap(dst)
    good, other = sa.blob("n64"), sa.blob("one_last")

    def patched(field, value):
        b = good.copy()
        b[:mc.HEADER.itemsize].view(mc.HEADER)[field] = value
        return b

    both = np.concatenate([good, other])
    tries = {
        "flipped magic, single": lambda: _import_one(dst, 1, patched("magic", mc.MAGIC ^ 1)),
        "flipped magic, batch": lambda: _import_batch(dst, [0, 1], [other, patched("magic", mc.MAGIC ^ (1 << 63))]),
        "another grid, single": lambda: _import_one(dst, 1, sb.blob("one_first")),
        "another grid, batch": lambda: _import_batch(dst, [0, 1], [other, sb.blob("n63")]),
        "n_tiles = TT + 1, single": lambda: _import_one(dst, 1, patched("n_tiles", g.TT + 1)),
        "n_tiles = TT + 1, batch": lambda: _import_batch(dst, [0, 1], [other, patched("n_tiles", g.TT + 1)]),
        "8 bytes short, single": lambda: _import_one(dst, 1, good, nbytes=good.size - 8),
        "8 bytes short, last of a batch": lambda: _import_batch(dst, [0, 1], both, offsets=[0, good.size], nbytes=both.size - 8),
        "offset off an 8-byte boundary": lambda: _import_batch(dst, [0, 1], both, offsets=[0, 4]),
        "slot -1, single": lambda: _import_one(dst, -1, good),
        "slot N, single": lambda: _import_one(dst, N, good),
        "slot -1, batch": lambda: _import_batch(dst, [0, -1], [other, good]),
        "slot N, batch": lambda: _import_batch(dst, [0, N], [other, good]),
        "a slot listed twice": lambda: _import_batch(dst, [2, 2], [other, good]),
    }
    for what, call in tries.items():
        assert call() != 0, what
        _assert_same(dst, before, where=what)
    assert dst._L.tbnav_rbpf_import_batch_dev(dst._h, 0, None, None, 0, None) == 0        # n = 0: OK, and nothing happens
    assert dst._L.tbnav_rbpf_export_batch_sizes(dst._h, 0, None, None) == 0
    _assert_same(dst, before, where="n = 0")
    assert _import_batch(dst, [0, 1], both, offsets=[0, good.size]) == 0                 # (the same buffer, whole, is taken)
    _assert_holds(dst, 0, good, g)
    _assert_holds(dst, 1, other, g)
    dst.close()


# ---- h. tbnav_rbpf_copy_particle ----------------------------------------------------------------------------------------------------------
def test_copy_particle_across_handles_and_within_one(gpu_pkg, sources):
    g = mc.GRID_A
    a, b = _pf(g, 4), _pf(g, 4)
    _set_states(a, salt=1)
    _set_states(b, salt=2)
    d = mc.fill(g, mc.cases(g)["n65"], salt=3)
    a.setLogOdds(1, d)
    b.setLogOdds(2, mc.fill(g, mc.cases(g)["one_last"], salt=4))           # (what the copy replaces)
    blob = _export_one(a, 1)
    assert np.array_equal(blob, mc.expected_blob(d, g.xsize, mc.L_OCC, *mc.state_of(1, 1)))
    b.copyParticle(2, a, 1)
    _assert_holds(b, 2, blob, g, "across")
    a.copyParticle(3, a, 1)
    _assert_holds(a, 3, blob, g, "within")
    _assert_holds(a, 1, blob, g, "the source")
    assert _used(a) == 130 and _used(b) == 65                              # a deep copy: tiles of its own
    codes, metres = mc.stored_field(g)
    a.setOccDist(1, metres)
    b.copyParticle(0, a, 1)
    assert np.array_equal(b.distCode(0), codes) and np.array_equal(b.logOdds(0), d)
    # refusals: another grid, another field mode, a slot out of range — nothing moves
    before = _snap(b)
    other_grid = sources("B").pf
    ref_mode = _pf(g, 4, df_mode="reference")
    assert b.copyParticle(1, other_grid, 0, check=False) != 0
    assert b.copyParticle(1, ref_mode, 0, check=False) != 0 and ref_mode.copyParticle(1, b, 2, check=False) != 0
    assert b.copyParticle(4, a, 1, check=False) != 0 and b.copyParticle(1, a, -1, check=False) != 0
    _assert_same(b, before, where="refused copies")
    a.close(); b.close(); ref_mode.close()


def test_copy_particle_in_reference_mode_carries_the_occupied_sets_history(gpu_pkg):
    """Two scans into the source slot, the copy, a third scan into both at the same pose: both fields equal the oracle's GridMapper
    fed the three scans with its brushfire — whose result depends on the order the occupied cells were inserted in, so the history
    travelled (RefField::copy_slot)."""
    g = mc._grid("S", -3.0, 3.0)
    a, b = _pf(g, 4, df_mode="reference"), _pf(g, 4, df_mode="reference")
    poses = [(0.0, 0.0, 0.0), (0.05, 0.1, 0.05), (0.1, 0.15, 0.1)]
    rng = np.random.default_rng(6)
    rooms = [(-1.0, 1.0, -0.8, 0.9), (-1.0, 1.0, -0.8, 0.9), (-2.4, 2.5, -2.2, 2.3)]
    scans = [orc.room_scan(po, walls=w, rng=rng) for po, w in zip(poses, rooms)]
    ref = orc.GridAPI("orc", grid=(mc.RESOLUTION, g.map_min, g.map_max, g.map_min, g.map_max))
    for s in range(2):
        a.integrateScan(1, scans[s], poses[s])
        ref.integrate_scan(scans[s], poses[s], esdf=True)
    b.copyParticle(2, a, 1)
    a.integrateScan(1, scans[2], poses[2])
    b.integrateScan(2, scans[2], poses[2])
    ref.integrate_scan(scans[2], poses[2], esdf=True)
    want = ref.dump()
    ref.close()
    fa, fb = a.occDist(1), b.occDist(2)
    assert np.array_equal(fa, fb) and np.array_equal(fb, want["occ_dist"])
    assert np.array_equal(a.logOdds(1), want["log_odds"]) and np.array_equal(b.logOdds(2), want["log_odds"])
    assert (want["occ_dist"] == 0.0).sum() > 50 and a.occupiedCount()[1] == b.occupiedCount()[2] == (want["occ_dist"] == 0.0).sum()
    a.close(); b.close()
