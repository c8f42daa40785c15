"""What the tests of the ordered hits along parallel rays (test_ordered_along_host.py, test_gpu_ordered_along.py) share: the starts,
the oracle's expectation on the rays written out (ordered_helpers.peel / from_table on mirt.make_rays(starts, d)), and the calls
through 0xAA-prefilled buffers with guard records and guard counts behind them.  Test plumbing only."""
import ctypes as C

import numpy as np

import mirt
import ordered_helpers as O
from along_helpers import OBLIQUE, plant_odd_starts
from query_helpers import make_batch

GUARD = 16
REC = mirt.HIT_DTYPE.itemsize
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


def prefix(want, n, max_hits):
    hits, counts = want
    return np.ascontiguousarray(hits[:n, :max_hits]), np.minimum(counts[:n], max_hits).astype(np.int32)


def same(got, want, what):
    gh, gc = got[:2]
    wh, wc = want[:2]
    assert np.array_equal(gc, wc), "%s: %d counts differ (first at ray %d)" % (what, int((gc != wc).sum()), int(np.flatnonzero(gc != wc)[0]))
    assert np.array_equal(gh["index"], wh["index"]), "%s: index differs in %d slots" % (what, int((gh["index"] != wh["index"]).sum()))
    assert np.array_equal(gh["distance"].view(np.uint32), wh["distance"].view(np.uint32)), "%s: distance not bit-identical" % what
    assert gh.tobytes() == wh.tobytes(), "%s: position not bit-identical" % what


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


# ---- calls through guarded buffers -------------------------------------------------------------------------------------------------------

def _checked(hbuf, cbuf, n, max_hits, what, stray=None):
    """The call's records and counts out of the 0xAA-prefilled buffers: all written (the slots of a stray ray all NOT), the guards
    untouched."""
    hraw = hbuf.view(np.uint8).reshape(-1, REC)
    craw = cbuf.view(np.uint8).reshape(-1, 4)
    assert (hraw[n * max_hits:] == 0xAA).all(), "%s: wrote beyond %d x %d records" % (what, n, max_hits)
    assert (craw[n:] == 0xAA).all(), "%s: wrote beyond %d counts" % (what, n)
    untouched = (hraw[:n * max_hits] == 0xAA).all(axis=1).reshape(n, max_hits)
    if stray is None:
        stray = np.zeros(n, bool)
    assert not untouched[~stray].any(), "%s: a slot of the call was not written" % what
    assert (hraw[:n * max_hits].reshape(n, max_hits, REC)[stray] == 0xAA).all(), "%s: a slot of a ray that names no direction was written" % what
    assert not (craw[:n] == 0xAA).all(axis=1).any(), "%s: a count of the call was not written" % what
    hits = hbuf[:n * max_hits].reshape(n, max_hits).copy()
    counts = cbuf[:n].copy()
    assert ((counts >= 0) & (counts <= max_hits)).all(), what
    return hits, counts


def ordered_along(form, d, starts, max_hits, after=None, mode=None, what="", dir_of=None, stray=None):
    """One call through guarded buffers: (hits[n, max_hits], counts[n], mirt.along_stats()).  d: one direction (3,) for
    mirt_intersect_ordered_along*, or several (k, 3) with dir_of (or None for k == 1) for mirt_intersect_ordered_alongs*."""
    from devbuf import DeviceArray, to_device
    d = np.ascontiguousarray(d, np.float32)
    several = d.ndim == 2
    starts = np.ascontiguousarray(starts, np.float32).reshape(-1, 3)
    n = len(starts)
    after = None if after is None else np.ascontiguousarray(after, mirt.HIT_DTYPE)
    dir_of = None if dir_of is None else np.ascontiguousarray(dir_of, np.int32)
    lib = mirt.load()
    P = mirt._ptr
    mirt.set_query_mode(mirt.QUERY_AUTO if mode is None else mode)
    try:
        if form == "host":
            hbuf = np.frombuffer(np.full((n * max_hits + GUARD) * REC, 0xAA, np.uint8).tobytes(), mirt.HIT_DTYPE).copy()
            cbuf = np.frombuffer(np.full((n + GUARD) * 4, 0xAA, np.uint8).tobytes(), np.int32).copy()
            if several:
                mirt._check(lib.mirt_intersect_ordered_alongs(P(d), len(d), P(dir_of), P(starts), n, P(after), max_hits, P(hbuf), P(cbuf)))
            else:
                mirt._check(lib.mirt_intersect_ordered_along(P(d), P(starts), n, P(after), max_hits, P(hbuf), P(cbuf)))
            return _checked(hbuf, cbuf, n, max_hits, what, stray) + (mirt.along_stats(),)
        held = [to_device(starts)] + [to_device(x) for x in (after, dir_of) if x is not None]
        d_after = None if after is None else held[1].ptr
        d_of = None if dir_of is None else held[-1].ptr
        try:
            with DeviceArray(((n * max_hits + GUARD) * REC,), np.uint8, 0xAA) as d_hits, DeviceArray(((n + GUARD) * 4,), np.uint8, 0xAA) as d_counts:
                if several:
                    mirt.intersect_ordered_alongs_device(d, d_of, held[0].ptr, n, d_after, max_hits, d_hits.ptr, d_counts.ptr)
                else:
                    mirt.intersect_ordered_along_device(d, held[0].ptr, n, d_after, max_hits, d_hits.ptr, d_counts.ptr)
                st = mirt.along_stats()
                mirt.sync()
                hbuf = np.frombuffer(d_hits.read().tobytes(), mirt.HIT_DTYPE).copy()
                cbuf = np.frombuffer(d_counts.read().tobytes(), np.int32).copy()
            return _checked(hbuf, cbuf, n, max_hits, what, stray) + (st,)
        finally:
            for x in held:
                x.free()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


def last_records(hits, counts, max_hits):
    """after[i] for the next call: the last record written where the ray's count reached max_hits, a fresh record (which admits
    nothing: the ray is exhausted) otherwise."""
    nxt = mirt.fresh_hits(len(hits))
    full = counts == max_hits
    nxt[full] = hits[full, max_hits - 1]
    return nxt


def bad_calls(n=5):
    """(entry point name, arguments, what is wrong) for every argument the calls refuse -- test_gpu_ordered_hits.py:
    test_errors_and_an_empty_call's and test_gpu_along.py / test_gpu_alongs.py: test_argument_validation's --, and the arrays they
    point into: (cases, arrays, snapshot())."""
    P = mirt._ptr
    d = np.array([0, 0, 1], np.float32)
    dirs = np.array([[0, 0, 1], [0, 1, 0]], np.float32)
    of = np.array([0, 1, 1, 0, 1], np.int32)[:n]
    origins = np.zeros((n, 3), np.float32)
    hits = np.frombuffer(np.full(n * 9 * REC, 0xAA, np.uint8).tobytes(), mirt.HIT_DTYPE).copy()
    counts = np.full(n, -1431655766, np.int32)                      # 0xAAAAAAAA
    inside = C.c_void_p(hits.ctypes.data + REC)
    H, Cn, Or = P(hits), P(counts), P(origins)
    order = [((None, 0), "max_hits 0"), ((None, 9), "max_hits 9"), ((None, -1), "max_hits -1"),
             ((H, 2), "after == hits with two slots a ray"), ((inside, 1), "after inside hits")]
    cases = []
    for name in NAMES:
        head = (P(dirs), 2, P(of)) if "alongs" in name else (P(d),)
        for (after, m), why in order:
            cases.append((name, head + (Or, n, after, m, H, Cn), why))
        cases += [(name, head + (None, n, None, 2, H, Cn), "NULL origins"), (name, head + (Or, n, None, 2, None, Cn), "NULL hits"),
                  (name, head + (Or, n, None, 2, H, None), "NULL counts"), (name, head + (Or, -1, None, 2, H, Cn), "a negative count")]
        if "alongs" in name:
            cases += [(name, (P(dirs), -1, P(of), Or, n, None, 2, H, Cn), "a negative direction count"), (name, (None, 2, P(of), Or, n, None, 2, H, Cn), "NULL dirs"),
                      (name, (P(dirs), 0, P(of), Or, n, None, 2, H, Cn), "rays but no direction"), (name, (P(dirs), 2, None, Or, n, None, 2, H, Cn), "NULL dir_of for two directions")]
        else:
            cases.append((name, (None, Or, n, None, 2, H, Cn), "NULL dir"))
    keep = (d, dirs, of, origins, hits, counts)
    return cases, keep, lambda: (hits.tobytes(), counts.tobytes())
