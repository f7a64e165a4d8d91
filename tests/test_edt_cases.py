"""The distance-field case table (tests/edt_cases.py) on the CPU: its sizes are what create's rules give, its patterns take the tiers
they name, the brute-force reference agrees with an independent restatement, and the edge cases would catch the mistakes they are
there for.  No device."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest

import edt_cases as ec
import oracle_api as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
MAX_LDS = 160 * 1024


# ---- create's rules, restated (csrc/rbpf.hip: create_impl; csrc/rbpf_plan.hpp: edt_lds_bytes, edt_cols_for) --------------------------------------------------------------------------
def lds_bytes(xsize, cols):
    """Bitmap rows as u64 words, and per row and column of the tile a u16 stack row, an i16 stack start and a u8 row distance."""
    return xsize * ((xsize + 63) // 64) * 8 + xsize * cols * 5


def create_rules(half, res):
    xsize = int(math.ceil((half - -half) / res))
    radius = int(math.ceil((10.0 - 0.0) / res))
    cols = 64 if lds_bytes(xsize, 64) <= MAX_LDS else 32 if lds_bytes(xsize, 32) <= MAX_LDS else 0
    return xsize, radius, cols


def test_every_size_is_what_the_create_rules_give():
    for s in ec.SIZES:
        assert create_rules(s.half, s.res) == (s.xsize, s.radius, s.cols), s.id
        assert s.xsize % 2 == 0 and 4 <= s.xsize and s.radius <= 254
    by = ec.SIZE
    # the LDS limit from both sides, for both tile widths
    assert lds_bytes(434, 64) == 163184 <= MAX_LDS < lds_bytes(436, 64)
    assert lds_bytes(660, 32) == 163680 <= MAX_LDS < lds_bytes(662, 32)
    assert (by["lds64-last"].xsize, by["lds32-first"].xsize, by["lds32-last"].xsize, by["query-first"].xsize) == (434, 436, 660, 662)
    assert by["ragged16"].xsize == 7 * 64 + 16 == 14 * 32 + 16
    assert {s.radius for s in ec.SIZES} == {200, 160, 254, 80, 20, 4, 64, 128}
    # the compact kernels' neighbour-word loops run while (words between) * 64 < radius: no, one, two, three and four trips
    assert {-(-s.radius // 64) for s in ec.SIZES} == {1, 2, 3, 4}
    r = ec.RADIUS_255
    assert create_rules(r["half"], r["refused_res"]) == (r["xsize"], 255, 32)
    assert create_rules(r["half"], r["accepted_res"]) == (r["xsize"], 254, 32)


def test_patterns_take_the_tier_they_name_and_stay_within_the_budget():
    names_seen = set()
    for s in ec.SIZES:
        pats = ec.patterns(s)
        assert len({p.id for p in pats}) == len(pats)
        for p in pats:
            occ = ec.occupancy(s, p)
            assert occ.shape == (s.xsize, s.xsize) and occ.dtype == np.uint8
            assert np.array_equal(occ, ec.occupancy(s, p))            # a fixed seed
            rows = int(occ.any(axis=1).sum())
            name = ec.kernel(s, p, occ)
            names_seen.add(name)
            assert int(occ.sum()) * s.xsize * s.xsize <= ec.BUDGET, (s.id, p.id, int(occ.sum()))
            m = re.fullmatch(r"rows-(\d+)", p.id)
            if m:       # the tier edges: exactly that many non-empty rows, 1..3 cells each
                assert rows == int(m.group(1)) and set(occ.sum(axis=1).tolist()) <= {0, 1, 2, 3}
            if s.cols:
                want = ec.COMPACT_A if rows <= 144 else ec.COMPACT_B if rows <= 288 else f"rbpf_edt<{s.cols}>"
                assert name == want
                if p.group in ("cut", "seams", "ties") or p.id == "empty":
                    assert name == ec.COMPACT_A
                if p.group == "general":
                    assert rows in (288, 289) and name == (ec.COMPACT_B if rows == 288 else f"rbpf_edt<{s.cols}>")
            else:
                assert name == ec.BY_QUERY
        if s.xsize > 289:
            edge = {p.id: ec.kernel(s, p) for p in pats if p.id.startswith("rows-")}
            g = ec.kernel_for_rows(s, s.xsize)
            assert list(edge.values()) == ([ec.COMPACT_A] * 2 + [ec.COMPACT_B] * 2 + [g] * 2 if s.cols else [ec.BY_QUERY] * 6), s.id
    assert names_seen == {"rbpf_edt<64>", "rbpf_edt<32>", ec.COMPACT_A, ec.COMPACT_B, ec.BY_QUERY}
    # seams: every size has its word seams and the first column of its ragged last tile
    assert ec.seam_columns(ec.SIZE["ragged16"]) == [0, 31, 32, 63, 64, 127, 448, 463]
    assert ec.seam_columns(ec.SIZE["lds64-last"]) == [0, 31, 32, 63, 64, 127, 384, 416, 433]
    assert ec.seam_columns(ec.SIZE["r4"]) == [0, 7]
    # with-fillers patterns: columns 0..8 see the tie cells alone
    for sid in ("shipped", "lds32-first"):
        s = ec.SIZE[sid]
        for p in ec.patterns(s):
            if p.build == "with_fillers":
                occ = ec.occupancy(s, p)
                cells = np.zeros_like(occ)
                for i, j in p.args[0]:
                    cells[i, j] = 1
                rest = occ - cells
                assert rest[:, :8 + s.radius + 1].sum() == 0 and rest.sum() == p.args[1] - len({i for i, _ in p.args[0]})


# ---- the reference is sound: brute force against a separable restatement ------------------------------------------------------------
def separable_codes(occ, radius, prev):
    """Row distance first, then the minimum over rows of di^2 + f^2; numpy, integers."""
    xs = occ.shape[0]
    none = 1 << 40
    j = np.arange(xs, dtype=np.int64)
    f2 = np.full((xs, xs), none, dtype=np.int64)
    for i in range(xs):
        cols = np.flatnonzero(occ[i])
        if cols.size:
            f2[i] = np.abs(j[:, None] - cols[None, :]).min(axis=1) ** 2
    di2 = (j[:, None] - j[None, :]) ** 2
    d2 = (di2[:, :, None] + f2[None, :, :]).min(axis=1)
    return np.where(d2 <= radius * radius, d2, prev).astype(np.uint16)


def _prev(size, pattern):
    return ec.as_injected(ec.previous_codes(size), size.res) if pattern.prev == "pattern" else np.full((size.xsize, size.xsize), ec.UNREACHED, dtype=np.uint16)


SMALL = [s for s in ec.SIZES if s.xsize <= 128]


@pytest.fixture(scope="module")
def small_references():
    """orc.exact_edt_codes of every pattern on the maps of at most 128 cells, computed once."""
    return {(s.id, p.id): orc.exact_edt_codes(ec.occupancy(s, p), s.radius, _prev(s, p)) for s in SMALL for p in ec.patterns(s)}


def test_brute_force_reference_agrees_with_a_separable_restatement(small_references):
    for s in SMALL:
        for p in ec.patterns(s):
            assert np.array_equal(small_references[s.id, p.id], separable_codes(ec.occupancy(s, p), s.radius, _prev(s, p))), (s.id, p.id)


def test_previous_codes_are_a_pattern_and_survive_the_round_trip_through_metres():
    for s in ec.SIZES:
        codes = ec.previous_codes(s)
        assert (codes == ec.UNREACHED).any() and len(np.unique(codes)) > min(1000, s.xsize * s.xsize // 4)
        held = ec.as_injected(codes, s.res)         # (asserts that set_occ_dist accepts every value)
        ok = codes != ec.UNREACHED
        assert np.array_equal(held[ok], codes[ok])
        # "unreached" is 10 m: where that is a whole number of cells it comes back as that distance, elsewhere as itself
        whole = s.radius * s.res == 10.0
        assert np.all(held[~ok] == (s.radius ** 2 if whole else ec.UNREACHED)), s.id
    assert {s.id for s in ec.SIZES if s.radius * s.res != 10.0} == {"rmax", "rmax-last"}


# ---- the edge cases bite ----------------------------------------------------------------------------------------------------------------
def test_radius_cut_cases_depend_on_the_radius_and_hold_cells_exactly_on_it():
    """Single cells, so the field is (i - i0)^2 + (j - j0)^2 directly — for every size, without the brute force."""
    for s in ec.SIZES:
        n_cut = 0
        for p in (p for p in ec.patterns(s) if p.group == "cut"):
            (i0, j0), = p.args[0]
            i, j = np.indices((s.xsize, s.xsize))
            d2 = (i - i0) ** 2 + (j - j0) ** 2
            prev = _prev(s, p)
            field = lambda r: np.where(d2 <= r * r, d2, prev)
            disc_is_cut = (d2 > s.radius ** 2).any()
            if disc_is_cut:
                assert not np.array_equal(field(s.radius), field(s.radius - 1)), (s.id, p.id)
                on = d2 == s.radius ** 2
                assert on.any() and (prev[on] != d2[on]).any(), (s.id, p.id)          # cells exactly on the radius exist and are rewritten
                out = d2 > s.radius ** 2
                assert len(np.unique(prev[out])) > min(100, out.sum() // 2)   # what is kept is a pattern
                n_cut += 1
        assert n_cut >= 4, s.id       # every size: the four corner discs are cut off by the radius (the centre's too where the map is wide)


def envelope_codes(occ, radius, prev, floor="floor", pop="le", stats=None):
    """The kernels' algorithm, column by column: row distance (none beyond the radius), lower envelope of the parabolas
    (i - q)^2 + f(q)^2 with integer starts z = floor(num / den), pop while s <= z[top], walk.  floor="trunc" and pop="lt" are the two
    mistakes the tie cases are there for."""
    xs = occ.shape[0]
    out = prev.copy()
    cols_of = [np.flatnonzero(occ[i]) for i in range(xs)]
    for j in range(xs):
        f = [int(np.abs(c - j).min()) if c.size else None for c in cols_of]
        v, z = [], []
        for q in range(xs):
            if f[q] is None or f[q] > radius:
                continue
            hq = f[q] * f[q] + q * q
            s = None
            while v:
                num, den = hq - (f[v[-1]] ** 2 + v[-1] ** 2), 2 * (q - v[-1])
                s = num // den if floor == "floor" or num >= 0 else -((-num) // den)
                if stats is not None and z[-1] is not None and s == z[-1]:
                    stats["equal"] = stats.get("equal", 0) + 1
                gone = z[-1] is not None and (s <= z[-1] if pop == "le" else s < z[-1])
                if not gone:
                    break
                v.pop(); z.pop()
            z.append(s if v else None)     # (the first entry starts at minus infinity)
            v.append(q)
        if not v:
            continue
        kk = 0
        for i in range(xs):
            while kk + 1 < len(v) and z[kk + 1] < i:
                kk += 1
            d2 = (i - v[kk]) ** 2 + f[v[kk]] ** 2
            if d2 <= radius * radius:
                out[i, j] = d2
    return out


TIE_CASES = [(s, p) for s in SMALL for p in ec.patterns(s) if p.group == "ties" and (s.xsize <= 24 or p.id.startswith("tie-"))]


def test_envelope_restatement_is_the_reference_on_every_tie_case(small_references):
    for s, p in TIE_CASES:
        assert np.array_equal(envelope_codes(ec.occupancy(s, p), s.radius, _prev(s, p)), small_references[s.id, p.id]), (s.id, p.id)


def test_truncation_toward_zero_is_caught_by_a_tie_case(small_references):
    caught = [(s.id, p.id) for s, p in TIE_CASES
              if not np.array_equal(envelope_codes(ec.occupancy(s, p), s.radius, _prev(s, p), floor="trunc"), small_references[s.id, p.id])]
    for s in SMALL:
        assert (s.id, "tie-negative-quarter") in caught and (s.id, "tie-negative-half") in caught, caught
        # ... where the case says: the intersection lies in (-1, 0), its truncation gives row 0 of column 0 to the wrong parabola
        for name, d2 in (("negative-quarter", 8), ("negative-half", 13)):
            p = next(p for p in ec.patterns(s) if p.id == "tie-" + name)
            wrong = envelope_codes(ec.occupancy(s, p), s.radius, _prev(s, p), floor="trunc")
            assert small_references[s.id, p.id][0, 0] == d2 and wrong[0, 0] > d2, (s.id, name)


def test_the_pop_rule_meets_equality_on_the_tie_cases_and_a_strict_rule_keeps_what_it_should_pop(small_references):
    """`<` for `<=` in the pop rule: the tie cases drive the rule to s == z[top] (counted), where the strict rule keeps an entry the
    rule pops.  That kept entry starts where its successor starts, so the walk never stops on it: with integer starts the strict rule
    writes the SAME field (shown here on every tie case, and by the argument in docs/lab_notebook.md, Round 16) — a kernel with
    either rule is correct, and no output test can tell them apart.  What a test can hold is that equality is reached, which is
    where a rule that is wrong in another way (`<= z - 1`, a comparison against the wrong entry) shows."""
    reached = {}
    for s, p in TIE_CASES:
        st = {}
        occ, prev = ec.occupancy(s, p), _prev(s, p)
        strict = envelope_codes(occ, s.radius, prev, pop="lt", stats=st)
        reached[s.id, p.id] = st.get("equal", 0)
        assert np.array_equal(strict, small_references[s.id, p.id]), (s.id, p.id)
    for sid in (s.id for s in SMALL):
        assert reached[sid, "tie-pop-on-equal-odd"] > 0 and reached[sid, "tie-pop-on-equal-even"] > 0


def test_the_tie_cases_hold_the_intersections_they_name():
    """From column 0: exact integers at odd and even gaps, exact halves, negatives within (-1, 0)."""
    from fractions import Fraction

    def cut(a, b, col=0):
        (q1, j1), (q2, j2) = a, b
        f1, f2 = abs(j1 - col), abs(j2 - col)
        return Fraction(f2 * f2 + q2 * q2 - f1 * f1 - q1 * q1, 2 * (q2 - q1))
    t = ec.TIES
    assert cut(*t["integer-odd-gap"]) == 4 and cut(*t["integer-even-gap"]) == 2
    assert cut(*t["half-odd-gap"]) == Fraction(7, 2) and cut(*t["half-even-gap"]) == Fraction(7, 2)
    assert cut(*t["negative-quarter"]) == Fraction(-1, 4) and cut(*t["negative-half"]) == Fraction(-1, 2)
    for k in ("pop-on-equal-odd", "pop-on-equal-even"):
        a, b, c = t[k]
        assert cut(a, b) == cut(b, c) and cut(a, b).denominator == 1
    a, b, c = t["three-kept"]
    assert math.floor(cut(a, b)) < math.floor(cut(b, c))
    assert all(0 <= i < 8 and 0 <= j < 8 for cells in t.values() for i, j in cells)
    assert set(ec.TIES_UNDER_OTHER_KERNELS) <= set(t)


# ---- the table names every transform instantiation the library ships ---------------------------------------------------------------
def test_shipped_listing_holds_exactly_the_four_transform_instantiations_and_the_table_names_each():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    spec = importlib.util.spec_from_file_location("isa_always_valu", os.path.join(ROOT, "tools", "isa_always_valu.py"))
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    shipped = set()
    for l in isa.listing("rbpf_field"):
        m = re.match(r"\s*\.amdhsa_kernel\s+_ZN8tbnav_rk\d+(rbpf_edt(?:_compact)?)ILi(\d+)EE", l)
        if m:
            shipped.add(f"{m.group(1)}<{m.group(2)}>")
    assert shipped == {"rbpf_edt<64>", "rbpf_edt<32>", "rbpf_edt_compact<144>", "rbpf_edt_compact<288>"}
    named = {ec.kernel(s, p) for s in ec.SIZES for p in ec.patterns(s)}
    assert shipped <= named and named - shipped == {ec.BY_QUERY}
