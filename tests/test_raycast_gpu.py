"""The map update on the device against the oracle's GridMapper, case by case and form by form (tests/raycast_cases.py; proved on
the CPU by tests/test_raycast_cases.py): every step through tbnav_rbpf_integrate_scan_many, the kernel of every launch asserted by
name and its LDS array by size against the restated selector, and at the marked steps EVERY particle's log-odds, occupied count,
occupancy bits (through the query-mode distance field) and exported map compared with `==`."""
import numpy as np
import pytest

import raycast_cases as rcs

pytestmark = pytest.mark.gpu

PARAMS = [(c.id, f) for c in rcs.cases() for f in c.forms]


def _filter(c, form):
    from rtn_amd import capi
    from rtn_amd.rbpf import ParticleFilter, default_params
    warm = rcs.FORMS[form]["warm"]
    pf = ParticleFilter(default_params(**rcs.device_params(c, c.N * (2 if warm else 1))))
    assert (pf.xsize, pf.ysize) == (rcs.cells_of(c),) * 2
    for k, v in rcs.form_opts(c, form).items():
        pf.setOption(getattr(capi, "RBPF_OPT_RAYCAST_" + k), v)
    return pf, warm


def _compare(pf, c, maps, where):
    nocc = pf.occupiedCount()
    for p in range(c.N):
        lo, occ, gm = maps[p]
        got = pf.logOdds(p)
        if not np.array_equal(got, lo):
            bad = np.flatnonzero(got != lo)
            cells = rcs.cells_of(c)
            raise AssertionError(f"{where} particle {p}: {bad.size} cells differ, first (cell, got, want): "
                                 f"{[(divmod(int(q), cells), float(got[q]), float(lo[q])) for q in bad[:4]]}")
        assert int(nocc[p]) == occ.size, (where, p, int(nocc[p]), occ.size)
        assert np.array_equal(np.flatnonzero(pf.occDist(p) == 0.0), occ), (where, p)      # the bits and the tile-row counts the query walks
        assert np.array_equal(pf.particleMap(p), gm), (where, p)


def _run(c, form, last_one_by_one=False):
    ref, pl = rcs.reference(c.id), rcs.plans(c.id)[form]
    pf, warm = _filter(c, form)
    try:
        first = next(st for st in c.steps if st.scan is not None)
        for _ in range(warm):           # the boxes' need reaches the host two launches on: spare particles take the same launch twice
            pf.integrateScanMany(first.scan, first.poses, first=c.N)
        for s, st in enumerate(c.steps):
            if st.scan is None:
                pf.gatherLocal(list(st.gather) + [-1] * (pf.N - c.N))
            elif last_one_by_one and s == len(c.steps) - 1:
                for p in range(c.N):
                    pf.integrateScan(p, st.scan, st.poses[p])
            else:
                pf.integrateScanMany(st.scan, st.poses)
                name, cap, need = pl[s]
                assert pf.lastKernelNames()[1:] == (name, c.N), (c.id, form, s, pf.lastKernelNames())
                if cap is not None:
                    assert pf.raycastBoxCells() == (need, cap), (c.id, form, s, pf.raycastBoxCells(), (need, cap))
            if st.mark:
                _compare(pf, c, ref["steps"][s]["maps"], f"{c.id} / {form} / step {s}:")
    finally:
        pf.close()


@pytest.mark.parametrize("cid,form", PARAMS, ids=[f"{a}-{b}" for a, b in PARAMS])
def test_the_map_update_leaves_the_oracle_s_maps(gpu_pkg, cid, form):
    _run(rcs.case(cid), form)


@pytest.mark.parametrize("cid", ["align", "sensor_offset", "events_9", "overflow_65", "hot_80", "cow_across_bands", "toggle_each_writer"])
def test_one_particle_at_a_time_leaves_the_same_maps(gpu_pkg, cid):
    """The case's final step through tbnav_rbpf_integrate_scan, particle by particle (what bmapping::GridMapper calls): one workgroup a
    launch, the same maps."""
    _run(rcs.case(cid), "box1024", last_one_by_one=True)


def test_integrate_scan_many_rejects_what_it_cannot_do(gpu_pkg):
    from rtn_amd import capi
    from rtn_amd.rbpf import ParticleFilter, default_params
    c = rcs.case("align")
    st = c.steps[0]
    pf = ParticleFilter(default_params(**rcs.device_params(c, c.N)))
    assert pf.integrateScanMany(st.scan, st.poses[:4], first=c.N - 3, check=False) == capi.ERR_INVALID_ARG     # runs past the last particle
    assert pf.integrateScanMany(st.scan, st.poses[:4], first=-1, check=False) == capi.ERR_INVALID_ARG
    far = st.poses.copy(); far[5, 1] = 7.0                                                                    # one particle out of the world
    assert pf.integrateScanMany(st.scan, far, check=False) == capi.ERR_OUT_OF_WORLD
    pf.close()
    import ctypes as C
    odd, h = default_params(**dict(rcs.device_params(c, c.N), map_max=2.05)), C.c_void_p()                      # 81 cells a side
    assert pf._L.tbnav_rbpf_create(C.byref(odd), C.byref(h)) == capi.ERR_UNSUPPORTED and not h.value             # no odd-sided map exists
    pf = ParticleFilter(default_params(**rcs.device_params(c, c.N)), df_mode="window")
    assert pf.integrateScanMany(st.scan, st.poses, check=False) == capi.ERR_UNSUPPORTED                          # stored fields: one particle at a time
    assert not pf.logOdds(0).any()
    pf.close()


def test_create_admits_the_cell_sizes_the_header_states(gpu_pkg):
    """include/tbnav_rbpf.h on `resolution`: radius ceil(10 / res) <= 254 (0.0394 m is admitted, 0.0393 m is not), an even square side,
    res > 0 — and *out stays NULL where create refuses."""
    import ctypes as C
    from rtn_amd import capi
    from rtn_amd.rbpf import default_params
    L = capi.lib()
    for kw, want in ((dict(resolution=0.0394), 0), (dict(resolution=0.5), 0), (dict(resolution=0.0393), capi.ERR_UNSUPPORTED),
                     (dict(resolution=0.01), capi.ERR_UNSUPPORTED), (dict(resolution=0.0), capi.ERR_INVALID_ARG), (dict(resolution=-0.05), capi.ERR_INVALID_ARG),
                     (dict(resolution=0.3, map_max=2.2), capi.ERR_UNSUPPORTED),          # fl(4.2 / 0.3) is just above 14: 15 cells, odd
                     (dict(resolution=0.5, map_max=0.4), capi.ERR_UNSUPPORTED)):         # 4.8 -> 5 cells, odd
        p, h = default_params(N=2, k=4, **kw), C.c_void_p()
        side = int(np.ceil((p.xmax - p.xmin) / p.resolution)) if p.resolution > 0 else None
        if want == capi.ERR_UNSUPPORTED and kw["resolution"] >= 0.0394:
            assert side % 2 == 1, (kw, side)                                             # refused for its odd side, nothing else
        rc = L.tbnav_rbpf_create(C.byref(p), C.byref(h))
        assert rc == want and bool(h.value) == (want == 0), (kw, rc, h.value)
        if h.value:
            L.tbnav_rbpf_destroy(h)
