"""What the tests of the ordered hits from shared origins (test_ordered_fans_host.py, test_gpu_ordered_fans.py,
test_gpu_placement_ordered_fans.py) share: the scenes, origins and batches of the many-origin fans' tests (test_gpu_fans_query.py:
origins_for with seed 3, make_batch with seed 5 -- the 182 seam directions of every origin among random ones, origins mixed within
every wave), the oracle's expectation on the rays written out (ordered_helpers.peel to 10 hits, computed once per case and left
read-only), the floors that keep the tests from being vacuous, and the calls through 0xAA-prefilled buffers with guard records and
guard counts behind them (ordered_helpers.guarded_call).  Test plumbing only."""
import numpy as np

import mirt
import ordered_helpers as O
from query_helpers import fan_scene_of
from test_gpu_fans_query import make_batch, origins_for

GUARD, REC, same, prefix, guarded_host = O.GUARD, O.REC, O.same, O.prefix, O.guarded_host
HITS = (1, 2, 3, 4, 5, 8)
CAP = 10                                                            # the oracle peels to 10 hits: "more than 8" shows
NAMES = ("mirt_intersect_ordered_from", "mirt_intersect_ordered_from_device", "mirt_intersect_ordered_fans", "mirt_intersect_ordered_fans_device")
# (scene, origins, rays) -> the floors of the issue's table: shares of rays with >= 1, 2, 4, 8 hits (None: not asserted), whether some
# ray must have more than 8 hits, and the share of rays with a tie pair (equal distance, the later index first) in slots 0 / 1
FLOORS = {("soup2000", 1, 2049): ((0.8, 0.55, 0.12, None), True, None),
          ("soup2000", 5, 2049): ((0.7, 0.5, 0.2, None), True, None),
          ("soup2000", 33, 6534): ((0.45, 0.3, None, None), False, None),
          ("cornell", 5, 1025): ((None, 0.3, None, None), False, 0.15),
          ("soup65x2", 5, 1025): ((None, None, None, None), False, 0.3),
          ("cornell+soup2000", 5, 2049): ((None, None, 0.5, 0.15), False, None)}
_cache = {}


def scene(name):
    """(triangles, b): fan_scene_of's, and soup65 twice (every hit has a partner at the same distance 65 indices later)."""
    if name == "soup65x2":
        return O.scene(name), 1.0
    return fan_scene_of(name)


def batch(name, K, nrays):
    """(tris, origins, origin_of, dirs) of scene `name`: origins_for (seed 3) and make_batch (seed 5) as test_gpu_fans_query.py
    makes them."""
    tris, b = scene(name)
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 15)
    origins = origins_for(tris, K)
    of, dirs = make_batch(origins, b, nrays)
    return tris, origins, of, dirs


def case(oracle, name, K, nrays, cap=CAP):
    """(tris, origins, origin_of, dirs, rays, (hits[n, cap], counts[n])): the oracle's enumeration of the batch's rays written out,
    computed once and left unchanged."""
    key = (name, K, nrays, cap)
    if key not in _cache:
        tris, origins, of, dirs = batch(name, K, nrays)
        rays = mirt.make_rays(origins[of], dirs)
        hits, counts = O.peel(oracle, tris, rays, cap)
        for x in (tris, origins, of, dirs, rays, hits, counts):
            x.setflags(write=False)
        _cache[key] = tris, origins, of, dirs, rays, (hits, counts)
    return _cache[key]


def shares(want):
    """The columns of the issue's table for the oracle's answer `want`."""
    hits, counts = want
    tie = (counts >= 2) & (hits["distance"][:, 0] == hits["distance"][:, 1]) & (hits["index"][:, 1] < hits["index"][:, 0])
    return [float((counts >= k).mean()) for k in (1, 2, 4, 8)], int((counts > 8).sum()), float(tie.mean())


def floors_hold(key, want):
    """The conditions of the issue's table on the oracle's answer for the case `key` = (scene, origins, rays)."""
    share, deep, tie = shares(want)
    floors, some_deep, tie_floor = FLOORS[key]
    for k, f, s in zip((1, 2, 4, 8), floors, share):
        assert f is None or s >= f, "%r: %.3f of the rays have >= %d hits, the floor is %.2f" % (key, s, k, f)
    assert not some_deep or deep > 0, "%r: no ray has more than 8 hits" % (key,)
    assert tie_floor is None or tie >= tie_floor, "%r: a tie pair in slots 0 / 1 for %.3f of the rays, the floor is %.2f" % (key, tie, tie_floor)
    return share, deep, tie


def ordered_fans(form, origins, of, dirs, max_hits, after=None, mode=None, what="", stray=None):
    """One call through guarded buffers: (hits[n, max_hits], counts[n], mirt.fan_stats()).  origins: one origin (3,) for
    mirt_intersect_ordered_from* (of is not used), or several (k, 3) with `of` (or None for k == 1) for mirt_intersect_ordered_fans*."""
    of = of if np.ndim(origins) == 2 else None
    return O.guarded_call(form, NAMES, mirt.fan_stats, origins, dirs, of, max_hits, after, mode, what, stray)


def peel_in_place(form, origins, of, dirs, mode, rounds):
    """The in-place peel (after == hits, max_hits 1) from fresh `after` records that admit everything, repeated `rounds` times or until
    every count is 0: (the records of every round [rounds_run, n], the counts of every round)."""
    from devbuf import DeviceArray, to_device
    origins = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    n = len(dirs)
    start = mirt.fresh_hits(n)
    start["distance"] = -1.0
    lib = mirt.load()
    P = mirt._ptr
    recs, cnts = [], []
    mirt.set_query_mode(mode)
    try:
        if form == "host":
            h = start.copy()
            c = np.zeros(n, np.int32)
            for _ in range(rounds):
                mirt._check(lib.mirt_intersect_ordered_fans(P(origins), len(origins), P(of), P(dirs), n, P(h), 1, P(h), P(c)))
                recs.append(h.copy()); cnts.append(c.copy())
                if not c.any():                                     # (an exhausted ray stays exhausted: the fresh record in its slot admits nothing)
                    break
        else:
            d_dirs, d_of, d_h = to_device(dirs), to_device(of), to_device(start)
            try:
                with DeviceArray((n,), np.int32, 0xAA) as d_c:
                    for _ in range(rounds):
                        mirt.intersect_ordered_fans_device(origins, d_of.ptr, d_dirs.ptr, n, d_h.ptr, 1, d_h.ptr, d_c.ptr)
                        h = d_h.read().view(mirt.HIT_DTYPE).reshape(-1).copy()
                        c = d_c.read().copy()
                        recs.append(h.copy()); cnts.append(c)
                        if not c.any():
                            break
            finally:
                for x in (d_dirs, d_of, d_h):
                    x.free()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
    return recs, cnts


def bad_calls(n=5):
    """ordered_helpers.bad_calls for the four entry points, and the arrays the cases point into: (cases, arrays, snapshot())."""
    P = mirt._ptr
    origin = np.zeros(3, np.float32)
    origins = np.array([[0, 0, 0], [0, 1, 0]], np.float32)
    of = np.array([0, 1, 1, 0, 1], np.int32)[:n]
    dirs = np.ones((n, 3), np.float32)
    bad_heads = [((P(origins), -1, P(of)), "a negative origin count"), ((None, 2, P(of)), "NULL origins"),
                 ((P(origins), 0, P(of)), "rays but no origin"), ((P(origins), 2, None), "NULL origin_of for two origins")]
    cases, out, snapshot = O.bad_calls(NAMES, (P(origin),), (P(origins), 2, P(of)), bad_heads, "NULL origin", dirs, "NULL dirs")
    return cases, (origin, origins, of, dirs) + out, snapshot

