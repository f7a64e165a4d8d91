"""Digests of a few cases of tests/raycast_cases.py and tests/propose_cases.py as the tables give them: the scans, the poses, the
oracle's maps at every marked step and the restated plans, hashed.  tests/golden/case_digests.json was written by this script BEFORE
the tables took a cell size; tests/test_raycast_cases.py and tests/test_propose_cases.py recompute the digests and compare, so the
0.05 m cases are byte for byte what they were.  Run from the repository root: python tests/golden/make_case_digests.py"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

RAYCAST_IDS = ("align", "map_edge_last_pair", "corner", "sensor_offset", "bv_513", "events_9", "overflow_65", "hot_80", "bands_natural_4p2m",
               "cow_across_bands", "toggle_each_writer")
PROPOSE_IDS = ("k-4", "valid-65", "split-default", "segments", "look7-limit", "lut-tiers", "edge", "trs")

PROPOSE_FIELDS = ("id group half cells room range_max trs start inc N k beams sources noises n_scans seed valid var clamps icp u_at resample_at "
                  "shard window walls_at reset_at threads expect").split()


def _h(parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes() if isinstance(p, np.ndarray) else repr(p).encode())
    return h.hexdigest()


def raycast_digest(cid):
    import raycast_cases as rcs
    c, ref = rcs.case(cid), rcs.reference(cid)
    parts = [c.map_min, c.map_max, c.range_max, c.n_beams, c.trs, c.N, c.forms, sorted(c.opts.items()), rcs.cells_of(c), rcs.grid_of(c)]
    for st, r in zip(c.steps, ref["steps"]):
        parts += [st.mark, st.gather] + ([st.scan, st.poses] if st.scan is not None else [])
        parts += [r["rc"], r["boxes"], r["robots"]] + (list(r["ends"]) if r["ends"] is not None else [])
        if r["maps"] is not None:
            for lo, occ, gm in r["maps"]:
                parts += [lo, occ, gm]
    parts.append(sorted(rcs.plans(cid).items()))
    return _h(parts)


def propose_digest(cid):
    import propose_cases as pc
    c = pc.CASE[cid]
    parts = [[getattr(c, f) for f in PROPOSE_FIELDS], pc.runs_of(c), [(pc.occ_half(c, s), pc.slice_bytes(c, s)) for s in c.sources], 
             sorted(((k, v) for k, v in pc.common_params(c).items() if k != "resolution"), key=str)]   # (the key the cell size added)
    for sc in pc.scans(c):
        parts += [sc.s, sc.scan, sc.u, np.asarray(sc.cur), np.asarray(sc.prev), sc.guess, sc.normals, sc.icp_ok, pc.n_valid(c, sc.scan)]
        parts += [x for x in (sc.weights, sc.reset_pose) if x is not None]
    return _h(parts)


def digests():
    return dict(raycast={i: raycast_digest(i) for i in RAYCAST_IDS}, propose={i: propose_digest(i) for i in PROPOSE_IDS})


if __name__ == "__main__":
    with open(os.path.join(HERE, "case_digests.json"), "w") as f:
        json.dump(digests(), f, indent=1, sort_keys=True)
        f.write("\n")
