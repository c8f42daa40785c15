"""What the tests of the ordered hits along parallel rays (test_ordered_along_host.py, test_gpu_ordered_along.py) share: the starts,
the oracle's expectation on the rays written out (ordered_helpers.peel / from_table on mirt.make_rays(starts, d)), and the calls
through 0xAA-prefilled buffers with guard records and guard counts behind them (ordered_helpers.guarded_call).  Test plumbing only."""
import numpy as np

import mirt
import ordered_helpers as O
from along_helpers import OBLIQUE, plant_odd_starts
from query_helpers import make_batch

GUARD, REC, prefix, same, last_records = O.GUARD, O.REC, O.prefix, O.same, O.last_records
SCENES = ("cornell", "soup2000", "soup65x2", "one")
HITS = (1, 2, 3, 4, 5, 8)
# the floors of the issue's table, on the reference alone: (subset, scene) -> (share with >= 1 hit, share with >= 2 hits or None)
FLOORS = {("back", "soup2000"): (0.5, 0.4), ("drawn", "soup2000"): (0.2, 0.1), ("back", "cornell"): (0.9, 0.3), ("back", "soup65x2"): (0.3, None)}
NAMES = ("mirt_intersect_ordered_along", "mirt_intersect_ordered_along_device", "mirt_intersect_ordered_alongs", "mirt_intersect_ordered_alongs_device")
_cache = {}


def extent_of(tris):
    return float(np.abs(np.asarray(tris).reshape(-1, 15)[:, :9]).max())


def starts_of(tris, d, n, seed=7):
    """(starts, planted, back): with B = make_batch(n, 1.5, 1.0)["start"], even rays are plant_odd_starts(B, extent) as drawn --
    starts inside the scene, the hits behind them excluded by t >= 0 --, odd rays are B / 1.5 - 3 * dhat, in front of the scene.
    planted: the even rays that carry one of plant_odd_starts' kinds; back: the odd rays."""
    B = make_batch(n, 1.5, 1.0, seed=seed)["start"]
    d64 = np.asarray(d, np.float64)
    with np.errstate(all="ignore"):
        norm = np.linalg.norm(d64)
        dhat = d64 / norm if np.isfinite(norm) and norm > 0 else np.zeros(3)
    starts, planted = plant_odd_starts(B, extent_of(tris))
    back = np.arange(n) % 2 == 1
    starts[back] = (B[back].astype(np.float64) / 1.5 - 3.0 * dhat).astype(np.float32)
    planted &= ~back
    return starts, planted, back


def case(oracle, name, d=OBLIQUE, n=257, cap=8, seed=7):
    """(tris, starts, planted, back, (hits[n, cap], counts[n])) for scene `name` along d, the oracle's enumeration computed once and
    left unchanged."""
    d = np.ascontiguousarray(d, np.float32)
    key = (name, d.tobytes(), n, cap, seed)
    if key not in _cache:
        tris = O.scene(name)
        starts, planted, back = starts_of(tris, d, n, seed)
        hits, counts = O.peel(oracle, tris, mirt.make_rays(starts, d), cap)
        for x in (starts, planted, back, hits, counts):
            x.setflags(write=False)
        _cache[key] = tris, starts, planted, back, (hits, counts)
    return _cache[key]


def floors_hold(name, want, back, what):
    """The conditions of the issue's table on the oracle's answer `want` for the rays in use."""
    counts = want[1]
    for subset, rows in (("back", back[:len(counts)]), ("drawn", ~back[:len(counts)])):
        if (subset, name) not in FLOORS or not rows.any():
            continue
        one, two = FLOORS[subset, name]
        if name == "soup65x2":
            h = want[0][rows]
            tie = (h["index"][:, 0] >= 0) & (h["index"][:, 1] >= 0) & (h["distance"][:, 0] == h["distance"][:, 1]) & (h["index"][:, 1] < h["index"][:, 0])
            assert tie.mean() >= one, "%s, %s: a tie pair in slots 0 / 1 for %.2f of the rays only" % (what, subset, tie.mean())
            continue
        assert (counts[rows] >= 1).mean() >= one, "%s, %s: %.2f of the rays hit" % (what, subset, (counts[rows] >= 1).mean())
        if want[0].shape[1] >= 2:
            assert (counts[rows] >= 2).mean() >= two, "%s, %s: %.2f of the rays hit twice" % (what, subset, (counts[rows] >= 2).mean())


def ordered_along(form, d, starts, max_hits, after=None, mode=None, what="", dir_of=None, stray=None):
    """One call through guarded buffers: (hits[n, max_hits], counts[n], mirt.along_stats()).  d: one direction (3,) for
    mirt_intersect_ordered_along*, or several (k, 3) with dir_of (or None for k == 1) for mirt_intersect_ordered_alongs*."""
    return O.guarded_call(form, NAMES, mirt.along_stats, d, starts, dir_of, max_hits, after, mode, what, stray)


def bad_calls(n=5):
    """ordered_helpers.bad_calls for the four entry points, and the arrays the cases point into: (cases, arrays, snapshot())."""
    P = mirt._ptr
    d = np.array([0, 0, 1], np.float32)
    dirs = np.array([[0, 0, 1], [0, 1, 0]], np.float32)
    of = np.array([0, 1, 1, 0, 1], np.int32)[:n]
    origins = np.zeros((n, 3), np.float32)
    bad_heads = [((P(dirs), -1, P(of)), "a negative direction count"), ((None, 2, P(of)), "NULL dirs"),
                 ((P(dirs), 0, P(of)), "rays but no direction"), ((P(dirs), 2, None), "NULL dir_of for two directions")]
    cases, out, snapshot = O.bad_calls(NAMES, (P(d),), (P(dirs), 2, P(of)), bad_heads, "NULL dir", origins, "NULL origins")
    return cases, (d, dirs, of, origins) + out, snapshot
