"""A migrating particle restated on the host, and the maps the migration tests move (tests/test_migrate_cases.py on the CPU,
tests/test_rbpf_migrate_gpu.py on the device).  Plain numpy, no device.

The blob (csrc/rbpf_device.hpp: BlobHeader, blob_layout_hd; written by csrc/rbpf_migrate.hip and csrc/rbpf_io.hip):

    BlobHeader    magic u64, n_tiles u32, has_codes u32, nocc i32, fstate i32, xsize u32, TT u32   (32 bytes, no padding)
    state         7 doubles: pose (theta, x, y), prev_pose, weight
    tile indices  n_tiles u32, ascending table index ti * TW + tj, padded to 8 bytes
    payloads      n_tiles * 1024 doubles, in-tile order (i & 31) * 32 + (j & 31)
    bits          n_tiles * 32 u32: word i & 31, bit j & 31 set where the cell is occupied (>= the cut), padded to 8
    tile rows     TW i32: occupied cells per tile row, padded to 8
    codes         G u16, padded to 8 — only where the stored field is authoritative (fstate == 2)

Every section but the payloads can end off an 8-byte boundary; the export never writes the pad bytes, so a test that compares bytes
hands it a zeroed buffer and expected_blob leaves them zero.

The maps are written once, with setLogOdds, into a fresh slot: rbpf_dense_to_tiles then names exactly the tiles that hold a non-zero
cell.  Their values stay away from the occupancy cut, so nothing here has to reproduce the bisection that finds it (find_occ_cut,
csrc/rbpf.hip, which lands within an ulp or so of L_OCC): occupied cells are L_OCC times 1, 2 or 3, free cells L_FREE times 1, 2 or
3 — fill() asserts that no value lies strictly between 0.5 * L_OCC and L_OCC, so `cut_occ` may be taken as L_OCC."""
from collections import namedtuple

import numpy as np

TS = 32                                   # kTS: cells per tile side
TILE_CELLS = TS * TS
RUN = 64                                  # 1 << rsh, rsh = 6: tiles one thread of rbpf_unpack_batch pops at once
TRIP = 256                                # table entries one trip of rbpf_pack_batch's compaction covers (four waves of 64)
WAVE = 64
MAGIC = 0x54424E4156504631                # kBlobMagic, "TBNAVPF1"
HEADER = np.dtype([("magic", "<u8"), ("n_tiles", "<u4"), ("has_codes", "<u4"), ("nocc", "<i4"), ("fstate", "<i4"),
                   ("xsize", "<u4"), ("TT", "<u4")])
UNREACHED = 0xFFFF
RESOLUTION = 0.05
MAX_OCC_DIST = 10.0
L_OCC = float(np.log(0.9 / (1 - 0.9)))
L_FREE = float(np.log(0.35 / (1 - 0.35)))

Layout = namedtuple("Layout", "state tidx tiles tile_bm trow codes total")
Grid = namedtuple("Grid", "id map_min map_max xsize TW TT")


def _grid(gid, map_min, map_max):
    xsize = int(np.ceil((map_max - map_min) / RESOLUTION))       # mapSize, as create computes it
    TW = (xsize + TS - 1) // TS
    return Grid(gid, map_min, map_max, xsize, TW, TW * TW)


# Grid A: the default survey map, 400 = 12 * 32 + 16 cells a side: tile row 12 and tile column 12 are half tiles, one trip of the
# compaction.  Grid B: more than 256 tiles (a second trip) and again a side that is no multiple of 32.  The GPU tests assert both
# conditions on the handle and take xsize, TW and TT from it.
GRID_A = _grid("A", -10.0, 10.0)
GRID_B = _grid("B", -13.0, 13.0)
GRIDS = {g.id: g for g in (GRID_A, GRID_B)}
assert GRID_A.TT <= TRIP and GRID_A.xsize % TS != 0
assert GRID_B.TT > TRIP and GRID_B.xsize % TS != 0 and GRID_B.xsize % 2 == 0


def up8(v):
    return (v + 7) & ~7


def blob_layout(TW, G, n_tiles, has_codes):
    """blob_layout_hd, line by line."""
    o = HEADER.itemsize
    state = o; o += 8 * 7
    tidx = o; o = up8(o + 4 * n_tiles)
    tiles = o; o += 8 * TILE_CELLS * n_tiles
    tile_bm = o; o = up8(o + 4 * TS * n_tiles)
    trow = o; o = up8(o + 4 * TW)
    codes = o
    if has_codes:
        o = up8(o + 2 * G)
    return Layout(state, tidx, tiles, tile_bm, trow, codes, o)


def _tiles_of(dense, xsize):
    """[TT][32][32]: the map cut into tiles, 0.0 for the cells of the edge tiles beyond xsize."""
    TW = (xsize + TS - 1) // TS
    pad = TW * TS - xsize
    m = np.pad(np.asarray(dense, dtype=np.float64).reshape(xsize, xsize), ((0, pad), (0, pad)))
    return m.reshape(TW, TS, TW, TS).transpose(0, 2, 1, 3).reshape(TW * TW, TS, TS)


def named_tiles(dense, xsize):
    """Ascending table indices ti * TW + tj of the tiles that hold a non-zero cell."""
    return np.flatnonzero((_tiles_of(dense, xsize) != 0.0).any(axis=(1, 2))).astype(np.uint32)


def occupied_count(dense, cut_occ=L_OCC):
    return int((np.asarray(dense) >= cut_occ).sum())


def expected_blob(dense_log_odds, xsize, cut_occ, pose, prev, weight, fstate=0, codes=None):
    """The bytes an export writes for a particle whose map was set once, with setLogOdds, in a fresh slot."""
    TW = (xsize + TS - 1) // TS
    G = xsize * xsize
    tiles = _tiles_of(dense_log_odds, xsize)
    tidx = np.flatnonzero((tiles != 0.0).any(axis=(1, 2))).astype(np.uint32)
    occ = tiles >= cut_occ
    words = (occ.astype(np.uint64) << np.arange(TS, dtype=np.uint64)).sum(axis=2).astype(np.uint32)      # [TT][row]: bit j & 31
    trow = occ.reshape(TW, TW, TS, TS).sum(axis=(1, 2, 3)).astype(np.int32)
    L = blob_layout(TW, G, tidx.size, codes is not None)
    out = np.zeros(L.total, dtype=np.uint8)
    hd = np.zeros(1, dtype=HEADER)
    hd["magic"], hd["n_tiles"], hd["has_codes"], hd["nocc"] = MAGIC, tidx.size, 0 if codes is None else 1, int(trow.sum())
    hd["fstate"], hd["xsize"], hd["TT"] = fstate, xsize, TW * TW

    def put(at, a):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        out[at:at + raw.size] = raw

    put(0, hd)
    put(L.state, np.concatenate([np.asarray(pose, dtype=np.float64), np.asarray(prev, dtype=np.float64), [float(weight)]]))
    put(L.tidx, tidx)
    put(L.tiles, tiles[tidx])
    put(L.tile_bm, words[tidx])
    put(L.trow, trow)
    if codes is not None:
        put(L.codes, np.asarray(codes, dtype=np.uint16).reshape(G))
    return out


def parse_blob(blob, TW, G):
    """A blob back into its parts: the header's fields, pose / prev / weight, tidx, the dense map (G values), the dense occupancy
    the bits describe, trow, codes (None without a codes section), total (the bytes it occupies)."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    hd = blob[:HEADER.itemsize].view(HEADER)[0]
    n, has_codes = int(hd["n_tiles"]), int(hd["has_codes"]) != 0
    L = blob_layout(TW, G, n, has_codes)
    assert blob.size >= L.total
    xsize = int(round(np.sqrt(G)))
    take = lambda at, dt, count: blob[at:at + np.dtype(dt).itemsize * count].view(dt)  # noqa: E731
    state = take(L.state, "<f8", 7)
    tidx = take(L.tidx, "<u4", n)
    tiles = np.zeros((TW * TW, TS, TS))
    tiles[tidx] = take(L.tiles, "<f8", n * TILE_CELLS).reshape(n, TS, TS)
    words = np.zeros((TW * TW, TS), dtype=np.uint32)
    words[tidx] = take(L.tile_bm, "<u4", n * TS).reshape(n, TS)
    bits = ((words[:, :, None] >> np.arange(TS, dtype=np.uint32)) & 1).astype(bool)
    undo = lambda t: t.reshape(TW, TW, TS, TS).transpose(0, 2, 1, 3).reshape(TW * TS, TW * TS)  # noqa: E731
    full, full_occ = undo(tiles), undo(bits)
    assert not full[xsize:].any() and not full[:, xsize:].any() and not full_occ[xsize:].any() and not full_occ[:, xsize:].any()
    return dict(magic=int(hd["magic"]), n_tiles=n, has_codes=int(hd["has_codes"]), nocc=int(hd["nocc"]), fstate=int(hd["fstate"]),
                xsize=int(hd["xsize"]), TT=int(hd["TT"]), pose=state[0:3].copy(), prev=state[3:6].copy(), weight=float(state[6]),
                tidx=tidx.copy(), dense=full[:xsize, :xsize].reshape(-1).copy(), occ=full_occ[:xsize, :xsize].reshape(-1).copy(),
                trow=take(L.trow, "<i4", TW).copy(), codes=take(L.codes, "<u2", G).copy() if has_codes else None, total=L.total)


# ---- the tile sets ---------------------------------------------------------------------------------------------------------------
def scattered(grid, n):
    """n tiles spread over the table by a fixed permutation (37 is coprime to 13 * 13 and to 17 * 17)."""
    assert 0 <= n <= grid.TT and np.gcd(37, grid.TT) == 1
    m = np.zeros(grid.TT, dtype=bool)
    m[(np.arange(n) * 37 + 11) % grid.TT] = True
    return m


def _ranges(grid, *spans):
    m = np.zeros(grid.TT, dtype=bool)
    for a, b in spans:
        m[a:b] = True
    return m


def _edge_ring(grid):
    m = np.zeros((grid.TW, grid.TW), dtype=bool)
    m[-1, :] = True
    m[:, -1] = True
    return m.reshape(-1)


def cases(grid):
    """name -> boolean mask over the grid's TT table entries, in a fixed order."""
    TT = grid.TT
    c = {"empty": _ranges(grid), "one_first": _ranges(grid, (0, 1)), "one_last": _ranges(grid, (TT - 1, TT)), "edge_ring": _edge_ring(grid)}
    for n in (63, 64, 65, 128, 129):
        c[f"n{n}"] = scattered(grid, n)
    c["all"] = _ranges(grid, (0, TT))
    if TT > TRIP:
        c["straddle_255_256"] = _ranges(grid, (250, 263))                        # the base carries into the second trip
        c["wave_full_then_empty"] = _ranges(grid, (0, 64), (128, 192), (256, TT))  # waves all named / all empty, then a second trip
        c["only_second_trip"] = _ranges(grid, (256, TT))                          # the first trip adds nothing to the base
    return c


def fill(grid, mask, salt=0):
    """The dense map (G values) of a tile set: in every chosen tile the four corner cells of the part of the tile that lies in the
    grid, valued so that swapping rows and columns, or the bit order of a word, changes the blob, and two more cells whose
    position moves with the tile's index and `salt`.  Every third tile holds free cells only: a payload, but no occupancy bit."""
    xs, TW = grid.xsize, grid.TW
    m = np.zeros((xs, xs))
    for t in np.flatnonzero(np.asarray(mask).reshape(-1)):
        ti, tj = divmod(int(t), TW)
        h, w = min(TS, xs - TS * ti), min(TS, xs - TS * tj)
        r0, c0 = TS * ti, TS * tj
        free_only = (t + salt) % 3 == 0
        a = (lambda q: L_FREE * q) if free_only else (lambda q: L_OCC * q)
        m[r0, c0] = a(1)
        m[r0, c0 + w - 1] = a(2)
        m[r0 + h - 1, c0] = L_FREE * 3
        m[r0 + h - 1, c0 + w - 1] = a(3)
        m[r0 + (7 * t + 3 + salt) % h, c0 + (11 * t + 5 + 2 * salt) % w] = a(1 + (t + salt) % 3)
        m[r0 + (13 * t + 1 + 3 * salt) % h, c0 + (5 * t + 2 + salt) % w] = L_FREE * (1 + t % 3)
    m = m.reshape(-1)
    assert not ((m > 0.5 * L_OCC) & (m < L_OCC)).any() and not ((m != 0.0) & (np.abs(m) < 0.4)).any()
    return m


def state_of(slot, salt=0):
    """Distinct pose, prev_pose and weight per slot (theta, x, y), all exactly representable sums of small binary fractions."""
    s = slot + 16 * salt
    return (np.array([0.125 * s - 1.0, 0.25 * s - 3.0, 2.0 - 0.375 * s]), np.array([0.0625 * s, -0.5 * s + 1.0, 0.75 * s - 2.0]),
            (s + 1) / 1024.0)


def stored_field(grid, salt=0):
    """(codes u16 [G] as the handle holds them, metres f64 [G] as tbnav_rbpf_set_occ_dist takes them) of a stored field that is NOT
    any map's distance transform: a few hand-placed squared cell distances, max_occ_dist elsewhere (which the handle holds as 200
    cells' squared distance: edt_cases.as_injected)."""
    import edt_cases as ec
    G = grid.xsize * grid.xsize
    codes = np.full(G, UNREACHED, dtype=np.uint16)
    at = (np.array([0, 1, grid.xsize - 1, grid.xsize, G // 2 + 7, G - grid.xsize, G - 2, G - 1]) + 3 * salt) % G
    codes[at] = np.array([0, 1, 2, 5, 13, 400, 9, 25], dtype=np.uint16) + salt
    return ec.as_injected(codes, RESOLUTION, MAX_OCC_DIST), ec.metres(codes, RESOLUTION, MAX_OCC_DIST)
