"""CPU proofs about the hypotheses' case table (tests/icp_hyp_cases.py) on the restatement (tests/icp_hyp_restatement.py): every case
reaches what it names; the restatement's sliding maximum agrees with H4 applied pair by pair; the device's method (bins, every listed
candidate knocks the winners of the bins round it) agrees with it on drawn volumes, and winners against winners does not; each planted
error changes at least one case, and every case the table names for it; the refusals of H1 and H6; and the restated chain's verdicts on
the rectangle and the room."""
import numpy as np
import pytest

import icp_global_restatement as G
import icp_hyp_cases as hc
import icp_hyp_restatement as H


def _digest(r: H.Result):
    return (r.status, [(y.ia, y.tx, y.ty, y.score, y.accepted) for y in r.hyps], r.info, r.index.tolist(), r.score.tolist(), r.peak.tolist())


@pytest.mark.parametrize("name", [c.name for c in hc.CASES])
def test_the_case_reaches_what_it_names(name):
    c = hc.CASE[name]
    r, g = hc.expected(name), hc.volumes(name)
    assert c.check(c, r, g), (name, c.reaches, r.info, r.hyps)
    # H4 / H5 on what came out: in key order, hypothesis 0 is the global search's answer, no two peaks in each other's window
    if r.hyps:
        y = r.hyps[0]
        assert (y.ia, y.tx, y.ty, y.score) == (g.info.ia, g.info.tx, g.info.ty, g.info.score)
        keys = [(y.score << 32) | (~((y.ia * c.geom.side + y.tx) * c.geom.side + y.ty) & 0xffffffff) for y in r.hyps]
        assert keys == sorted(keys, reverse=True) and len(set(keys)) == len(keys)
    assert r.info["n"] == min(c.hp.max_hyp, r.info["n_peaks"]) and int(r.peak.sum()) == r.info["n_peaks"] and len(r.index) == r.info["candidates"]
    assert np.all(np.diff(r.index.astype(np.int64)) > 0)


def _pairwise_peaks(scores, side, tx0, ty0, t, hp):
    """H4 as it is written: a candidate at the floor is a peak when no candidate of its window has a greater key"""
    idx = np.argwhere(scores >= max(t, 1))
    sc = scores[scores >= max(t, 1)].astype(np.int64)
    lin = (idx[:, 0] * side + tx0 + idx[:, 1]) * side + ty0 + idx[:, 2]
    na = scores.shape[0]
    peak = np.zeros(len(idx), dtype=np.uint8)
    for n in range(len(idx)):
        inside = ((np.abs(idx[:, 1] - idx[n, 1]) <= hp.sep_cells) & (np.abs(idx[:, 2] - idx[n, 2]) <= hp.sep_cells)
                  & (H.heading_distance(idx[:, 0], idx[n, 0], na, hp) <= hp.sep_steps))
        greater = (sc > sc[n]) | ((sc == sc[n]) & (lin < lin[n]))
        peak[n] = not (inside & greater).any()
    return peak


def _device_peaks(scores, side, tx0, ty0, t, hp, winners_only=False):
    """the kernels' method in numpy: bins of (sep_steps + 1) x (sep_cells + 1)^2, each bin's winner; every candidate at the floor (or,
    planted, every winner) knocks the winners with a lesser key inside its window; the alive winners are the peaks"""
    idx = np.argwhere(scores >= max(t, 1))
    sc = scores[scores >= max(t, 1)].astype(np.int64)
    lin = (idx[:, 0] * side + tx0 + idx[:, 1]) * side + ty0 + idx[:, 2]
    key = (sc << 32) | (~lin & 0xffffffff)
    na = scores.shape[0]
    ba, b = hp.sep_steps + 1, hp.sep_cells + 1
    win = {}
    for n, (ia, x, y) in enumerate(idx):
        k = (ia // ba, x // b, y // b)
        if k not in win or key[n] > key[win[k]]:
            win[k] = n
    alive = {k: True for k in win}
    for n in (sorted(win.values()) if winners_only else range(len(idx))):
        ia, x, y = idx[n]
        heads = {(ia + d) % na for d in range(-hp.sep_steps, hp.sep_steps + 1)} if hp.wrap else {ia + d for d in range(-hp.sep_steps, hp.sep_steps + 1) if 0 <= ia + d < na}
        for ka in {h // ba for h in heads}:
            for kx in (x // b - 1, x // b, x // b + 1):
                for ky in (y // b - 1, y // b, y // b + 1):
                    w = win.get((ka, kx, ky))
                    if w is None or key[w] >= key[n]:
                        continue
                    if (abs(idx[w, 1] - x) <= hp.sep_cells and abs(idx[w, 2] - y) <= hp.sep_cells
                            and H.heading_distance(idx[w, 0], ia, na, hp) <= hp.sep_steps):
                        alive[(ka, kx, ky)] = False
    peak = np.zeros(len(idx), dtype=np.uint8)
    for k, n in win.items():
        peak[n] = alive[k]
    return peak


def _fake(scores, side):
    info = G.Info(1, 0, (0.0, 0.0, 0.0), 0, 0, 0, int(scores.max()), 1, 1, 0.0, 0)
    s = 8
    return G.Result(None, None, 1, G.block_maxima(scores, s), scores, info, 0)


@pytest.mark.parametrize("name", [c.name for c in hc.CASES if c.name not in ("rectangle", "room")] + ["rectangle", "room"])
def test_the_sliding_maximum_and_the_bins_agree_with_h4_pair_by_pair(name):
    c, r, g = hc.CASE[name], hc.expected(name), hc.volumes(name)
    if r.info["candidates"] == 0:
        return
    tx0, ty0, _, _ = G.region(c.gp, c.geom.side)
    t = r.info["floor_score"]
    assert np.array_equal(_pairwise_peaks(g.scores, c.geom.side, tx0, ty0, t, c.hp), r.peak), name
    assert np.array_equal(_device_peaks(g.scores, c.geom.side, tx0, ty0, t, c.hp), r.peak), name


def test_drawn_volumes_the_bins_are_exact_and_winners_against_winners_are_not():
    rng = np.random.default_rng(5)
    differs = 0
    for trial in range(60):
        na, w, h = int(rng.integers(1, 14)), int(rng.integers(1, 20)), int(rng.integers(1, 20))
        scores = rng.integers(0, int(rng.integers(2, 7)), size=(na, w, h)).astype(np.uint32)      # few distinct values: ties everywhere
        if scores.max() == 0:
            continue
        hp = H.HypParams(max_hyp=64, floor_q10=int(rng.integers(1, 1025)), sep_cells=int(rng.integers(0, 6)), sep_steps=int(rng.integers(0, 8)),
                         wrap=int(rng.integers(0, 2)))
        side = max(w, h)
        gp = G.Params(ang_count=na, region=(0, 0, w - 1, h - 1))
        r = H.hypotheses(_fake(scores, side), G.Geom(0.0, 0.0, 1.0, side), gp, hp)
        t = r.info["floor_score"]
        assert np.array_equal(_pairwise_peaks(scores, side, 0, 0, t, hp), r.peak), trial
        assert np.array_equal(_device_peaks(scores, side, 0, 0, t, hp), r.peak), trial
        differs += not np.array_equal(_device_peaks(scores, side, 0, 0, t, hp, winners_only=True), r.peak)
    assert differs > 0


# ---- the plants ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", H.PLANTS)
def test_each_planted_error_changes_a_case_and_every_case_named_for_it(plant):
    named = [c for c in hc.CASES if plant in c.plants]
    assert named, plant
    for c in named:
        assert _digest(H.hypotheses(hc.volumes(c.name), c.geom, c.gp, c.hp, plant)) != _digest(hc.expected(c.name)), (plant, c.name)


# ---- the refusals ---------------------------------------------------------------------------------------------------------------------------
def test_bad_parameters_bins_and_the_two_limits_are_refused():
    for kw in hc.BAD_PARAMS:
        assert not H.valid(H.HypParams().with_(**kw)), kw
    assert H.valid(H.HypParams()) and H.valid(H.HypParams(max_hyp=64, floor_q10=1, sep_cells=64, sep_steps=720, wrap=0))
    assert H.bins(hc.BINS_GP, 200, hc.BINS_HP) == 720 * 200 * 200 > H.MAX_BINS
    assert max(H.bins(c.gp, c.geom.side, c.hp) for c in hc.CASES) <= H.MAX_BINS
    cloud = hc.CASE["floor_equal"].cloud
    assert len(cloud) == 1
    for name, gp, hp in hc.REFUSED:
        vol = G.localize(hc.FULL_200(), hc.G200, cloud, hc.gc.SP5, gp)
        t = H.floor_of(int(vol.scores.max()), hp.floor_q10)
        blocks, cands = int((vol.bounds >= t).sum()), int((vol.scores >= t).sum())
        assert (blocks > H.MAX_REFINE) == (name == "floor_blocks") and (cands > H.MAX_CANDIDATES), (name, blocks, cands)
        assert H.hypotheses(vol, hc.G200, gp, hp).status == "unsupported"
    assert H.floor_of(255, 900) == 225 and H.floor_of(255, 904) == 226 and H.floor_of(255, 904, "floor_down") == 225 and H.floor_of(7, 1) == 1


# ---- behaviour: the restated chain ---------------------------------------------------------------------------------------------------------
def test_the_rectangle_ends_with_both_hypotheses_verified_and_ambiguous():
    _, _, _, ch = hc.behaviour("rectangle")
    assert [o["verified"] for o in ch["hypotheses"]] == [True, True] and ch["verified_count"] == 2 and ch["ambiguous"] and ch["best"] == 0
    assert all(o["fine"].ok and (o["check"]["walked"], o["check"]["hit"], o["check"]["through"], o["check"]["missing"]) == (360, 360, 0, 0)
               for o in ch["hypotheses"])
    assert ch["T"] == ch["hypotheses"][0]["T"]


def test_the_room_ends_with_four_accepted_by_quality_one_verified_and_not_ambiguous():
    _, _, _, ch = hc.behaviour("room")
    assert [o["found"].accepted for o in ch["hypotheses"]] == [1, 1, 1, 1]
    assert [o["verified"] for o in ch["hypotheses"]] == [True, False, False, False] and ch["best"] == 0 and not ch["ambiguous"]
    print([(o["check"]["hit"], o["check"]["through"], o["check"]["missing"]) for o in ch["hypotheses"]])
    # the wrong rotations are refused for beams through walls and beams that end in known free space, not by a hair
    assert all(o["check"]["through"] + o["check"]["missing"] > 60 for o in ch["hypotheses"][1:])
