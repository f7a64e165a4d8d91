"""The case table of the stored distance field (csrc/rbpf_field.hip: rbpf_edt<64>, rbpf_edt<32>, rbpf_edt_compact<144>,
rbpf_edt_compact<288>; csrc/rbpf_propose.hip: rbpf_field_by_query).  Plain data: map sizes, occupancy patterns with fixed seeds, and the
kernel each pattern must run.  tests/test_edt_cases.py proves the table on the CPU, tests/test_edt_gpu.py runs it.

Sizes are the smallest at which each kernel and each edge of create's rules exists:
  * the LDS limit: the last size with 64-column tiles (434), the first and the last with 32-column tiles (436, 660), the first with
    no LDS transform at all (662);
  * a ragged last tile under both widths (464 = 7 * 64 + 16 = 14 * 32 + 16);
  * the largest radius create accepts (254), also at the last LDS size;
  * radii below 128 / 64 / 8, where the compact kernels' neighbour-word loops make one or no trip (80, 20, 4);
  * the shipped 400-cell map;
  * radii of exactly one and two words (64, 128), where the bound of those loops, (words between) * 64 < radius, is an equality.
"""
import zlib
from collections import namedtuple

import numpy as np

Size = namedtuple("Size", "id half res xsize cols radius")
SIZES = (
    Size("lds64-last", 10.85, 0.05, 434, 64, 200),
    Size("lds32-first", 10.9, 0.05, 436, 32, 200),
    Size("lds32-last", 16.5, 0.05, 660, 32, 200),
    Size("query-first", 16.55, 0.05, 662, 0, 200),
    Size("ragged16", 14.5, 0.0625, 464, 32, 160),
    Size("rmax", 10.0, 0.0394, 508, 32, 254),
    Size("rmax-last", 13.0, 0.0394, 660, 32, 254),
    Size("r80", 8.0, 0.125, 128, 64, 80),
    Size("r20", 6.0, 0.5, 24, 64, 20),
    Size("r4", 10.0, 2.5, 8, 64, 4),
    Size("shipped", 10.0, 0.05, 400, 64, 200),
    Size("r64", 10.0, 0.15625, 128, 64, 64),
    Size("r128", 10.0, 0.078125, 256, 64, 128),
)
SIZE = {s.id: s for s in SIZES}
# a resolution create must refuse (radius 255) and its neighbour it must accept (radius 254), on the same 458-cell map
RADIUS_255 = dict(half=9.0, refused_res=0.03936, accepted_res=0.03938, xsize=458)

COMPACT_A, COMPACT_B, BY_QUERY = "rbpf_edt_compact<144>", "rbpf_edt_compact<288>", "rbpf_field_by_query"
ROWS_A, ROWS_B = 144, 288
BUDGET = 5 * 10 ** 8          # occupied cells x cells of one pattern: the brute-force reference stays around a second
UNREACHED = 0xFFFF

# name, group, builder, arguments, the previous field (None: all unreached; "pattern": previous_codes() is injected first)
Pattern = namedtuple("Pattern", "id group build args prev")


def kernel_for_rows(size, rows):
    """The kernel a particle with `rows` non-empty map rows must take on a map of this size."""
    if size.cols == 0:
        return BY_QUERY
    return COMPACT_A if rows <= ROWS_A else COMPACT_B if rows <= ROWS_B else f"rbpf_edt<{size.cols}>"


# ---- builders: (size, rng, *args) -> occupancy [xsize][xsize] u8 --------------------------------------------------------------------
def _cells(size, rng, cells):
    occ = np.zeros((size.xsize, size.xsize), dtype=np.uint8)
    for i, j in cells:
        occ[i, j] = 1
    return occ


def _rows_drawn(size, rng, rows_used, most):
    """tests/test_rbpf_gpu.py::test_distance_field_tiers_random_occupancy's generator: rows_used distinct rows, 1..most cells each at
    drawn columns."""
    xs = size.xsize
    occ = np.zeros((xs, xs), dtype=np.uint8)
    for r in rng.choice(xs, size=rows_used, replace=False):
        occ[r, rng.choice(xs, size=int(rng.integers(1, most + 1)), replace=False)] = 1
    return occ


def _column_run(size, rng, col, rows):
    """Rows 0 .. rows - 1 all hold one cell, in column col: the row pass of every other column meets distance |j - col|."""
    occ = np.zeros((size.xsize, size.xsize), dtype=np.uint8)
    occ[:rows, col] = 1
    return occ


def _with_fillers(size, rng, cells, rows):
    """`cells` (all within columns 0..7) and one filler cell in as many further rows as make `rows` non-empty ones, in columns more
    than the radius away from column 8: the columns 0..8 see the cells alone, and the particle takes the tier of `rows`."""
    xs = size.xsize
    occ = _cells(size, rng, cells)
    lo = 8 + size.radius + 1
    assert lo < xs
    need = rows - len({i for i, _ in cells})
    for r in [r for r in range(xs) if not occ[r].any()][:need]:
        occ[r, lo + (7 * r) % (xs - lo)] = 1
    return occ


def _full_row(size, rng):
    occ = np.zeros((size.xsize, size.xsize), dtype=np.uint8)
    occ[size.xsize // 2, :] = 1
    return occ


def _full_column(size, rng):
    occ = np.zeros((size.xsize, size.xsize), dtype=np.uint8)
    occ[:, 5] = 1
    return occ


def _full_map(size, rng):
    return np.ones((size.xsize, size.xsize), dtype=np.uint8)


def _checkerboard(size, rng):
    i, j = np.indices((size.xsize, size.xsize))
    return ((i + j) & 1).astype(np.uint8)


def _uniform(size, rng, percent):
    return (rng.random((size.xsize, size.xsize)) < percent / 100.0).astype(np.uint8)


def _empty(size, rng):
    return np.zeros((size.xsize, size.xsize), dtype=np.uint8)


BUILDERS = dict(cells=_cells, rows_drawn=_rows_drawn, column_run=_column_run, with_fillers=_with_fillers, full_row=_full_row,
                full_column=_full_column, full_map=_full_map, checkerboard=_checkerboard, uniform=_uniform, empty=_empty)

# Ties in the lower envelope, seen from column 0 (f = the cell's column): the intersection of the parabolas of rows q1 < q2 is
# num / den = (f2^2 + q2^2 - f1^2 - q1^2) / (2 (q2 - q1)).  All cells lie within 8 x 8, so that every map holds them.
TIES = {
    "integer-odd-gap":  ((1, 0), (4, 3)),          # 24 / 6 = 4
    "integer-even-gap": ((1, 0), (3, 0)),          # 8 / 4 = 2: rows 1 and 3 tie on row 2
    "half-odd-gap":     ((1, 0), (2, 2)),          # 7 / 2 = 3.5
    "half-even-gap":    ((1, 0), (5, 2)),          # 28 / 8 = 3.5 (a gap of 2 cannot give a half: f2^2 - f1^2 is never 2 mod 4)
    "negative-quarter": ((0, 3), (2, 2)),          # -1 / 4: floor -1, truncation 0 — row 0 belongs to the second cell
    "negative-half":    ((0, 4), (3, 2)),          # -3 / 6
    "pop-on-equal-odd":  ((0, 0), (1, 1), (2, 0)),  # 2 / 2 = 1 and 2 / 2 = 1: the middle parabola's start equals the newcomer's
    "pop-on-equal-even": ((0, 0), (2, 2), (4, 0)),  # 8 / 4 = 2 and 8 / 4 = 2
    "three-kept":        ((0, 0), (3, 1), (6, 0)),  # 10 / 6 and 26 / 6: all three stay on the envelope
}
TIES_UNDER_OTHER_KERNELS = ("half-odd-gap", "negative-quarter", "pop-on-equal-even")


def seam_columns(size):
    """Columns at the word and tile seams: 0, 31 | 32, 63 | 64, 127, the last one, and the first column of the ragged last tile under
    64- and under 32-column tiles."""
    xs = size.xsize
    cols = {0, 31, 32, 63, 64, 127, xs - 1, (xs - 1) // 64 * 64, (xs - 1) // 32 * 32}
    return sorted(c for c in cols if 0 <= c < xs)


def patterns(size):
    """Every pattern of one map size, in the order of the particles that carry them."""
    xs = size.xsize
    out = [Pattern("empty", "tiers", "empty", (), None)]
    for n in (1, ROWS_A, ROWS_A + 1, ROWS_B, ROWS_B + 1, xs):
        if n <= xs:
            out.append(Pattern(f"rows-{n}", "tiers", "rows_drawn", (n, 3 if n <= 400 else 2), None))   # (budget: 1..2 cells on the largest)
    mid = xs // 2
    for name, cell in (("centre", (mid, mid)), ("corner-00", (0, 0)), ("corner-0n", (0, xs - 1)), ("corner-n0", (xs - 1, 0)),
                       ("corner-nn", (xs - 1, xs - 1))):
        out.append(Pattern(f"cut-{name}", "cut", "cells", ((cell,),), "pattern"))
    for rname, row in (("mid", mid), ("first", 0), ("last", xs - 1)):
        for c in seam_columns(size):
            out.append(Pattern(f"seam-{rname}-{c}", "seams", "cells", (((row, c),),), None))
    if xs <= 128:
        for name, cells in TIES.items():
            out.append(Pattern(f"tie-{name}", "ties", "cells", (cells,), None))
        for name in ("full_row", "full_column", "full_map", "checkerboard"):
            out.append(Pattern(name.replace("_", "-"), "ties", name, (), None))
        for pc in (1, 10, 30):
            out.append(Pattern(f"uniform-{pc}", "ties", "uniform", (pc,), None))
    if xs > ROWS_B:
        # the general kernel's (and the by-query kernel's) own row pass and envelope at the seams and ties: every pattern has 289 non-empty rows
        for c in (0, 64, xs - 1):
            out.append(Pattern(f"column-289-{c}", "general", "column_run", (c, ROWS_B + 1), None))
    if size.id in ("shipped", "lds32-first"):
        for name in TIES_UNDER_OTHER_KERNELS:
            for rows in (ROWS_B, ROWS_B + 1):
                out.append(Pattern(f"tie-{name}-{rows}", "general", "with_fillers", (TIES[name], rows), None))
    if size.id in ("lds64-last", "lds32-first", "lds32-last", "ragged16", "rmax"):
        for n in (140, 280, 400):
            out.append(Pattern(f"room-{n}", "rooms", "rows_drawn", (n, 3), None))
    return out


def groups(size):
    seen = []
    for p in patterns(size):
        if p.group not in seen:
            seen.append(p.group)
    return seen


def occupancy(size, pattern):
    """The pattern's occupancy on this size; the seed is fixed by the two names."""
    rng = np.random.default_rng(zlib.crc32(f"{size.id}/{pattern.id}".encode()))
    return BUILDERS[pattern.build](size, rng, *pattern.args)


def kernel(size, pattern, occ=None):
    """The kernel the pattern must run (an empty map reports the first compact kernel, which wrote nothing)."""
    occ = occupancy(size, pattern) if occ is None else occ
    return kernel_for_rows(size, int(occ.any(axis=1).sum()))


def previous_codes(size):
    """A previous field that is a pattern, not all "unreached": squared distances 1 .. 60000 and a sprinkle of unreached cells, every
    value one that tbnav_rbpf_set_occ_dist accepts."""
    i, j = np.indices((size.xsize, size.xsize))
    codes = (1 + (7 * i + 13 * j + 3 * i * j) % 60000).astype(np.uint16)
    codes[(i + 2 * j) % 11 == 0] = UNREACHED
    return codes


def metres(codes, res, max_occ_dist=10.0):
    """What tbnav_rbpf_get_occ_dist decodes codes to, and what set_occ_dist takes back: sqrt(code) * resolution."""
    return np.where(codes == UNREACHED, max_occ_dist, np.sqrt(codes.astype(np.float64)) * res)


def as_injected(codes, res, max_occ_dist=10.0):
    """The codes the handle holds after set_occ_dist(metres(codes)): the same, except that "unreached" is max_occ_dist metres, and where
    that is a whole number of cells (10 m at 0.05 m: 200 cells) the value reads as that distance — the reference's occ_dist cannot tell
    the two apart either."""
    v = metres(codes, res, max_occ_dist)
    cells = v / res
    d2 = np.rint(cells * cells)
    fits = (d2 >= 0) & (d2 < 65535) & (np.sqrt(d2) * res == v)
    assert np.all(fits | (v == max_occ_dist))
    return np.where(fits, d2, UNREACHED).astype(np.uint16)
