"""What the tests of the ordered hits (test_gpu_ordered_hits.py) share: the scenes and ray sets, and the CPU oracle's expectations --
the enumeration of a ray's hits by peeling (ClosestIntersection on a fresh record against the scene with the rows of the triangles
already reported for that ray set to NaN: a NaN row accepts nothing and indices keep their meaning), and the per-triangle table
(one oracle call per (ray, triangle) on a fresh record) from which the answer behind an arbitrary `after` record is sorted; and, for
the calls along directions and from origins, the one call through guarded 0xAA buffers and the list of refused calls.
Test plumbing only."""
import ctypes as C

import numpy as np

import mirt
import ray_grid_helpers as H
from query_helpers import make_batch, odd_rays, scene_of

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
_cache = {}

GRID_SCENES = {"cornell": 4, "wall": 8, "soup2000": 16}              # test_gpu_ray_grid.py: these are binned, with this many cells a side


def scene(name):
    if name in GRID_SCENES:
        return H.scene(name)
    if name == "soup65x2":                                          # every hit has a partner at the same distance 65 indices later
        t = scene_of("soup65")[0]
        return np.concatenate([t, t])
    return scene_of(name)[0]


def rays_of(name, n=4097):
    """n rays: for the grid's scenes ray_grid_helpers.ray_set (its planted unfit rays included) interleaved with make_batch rays that
    carry query_helpers.odd_rays; make_batch with odd_rays otherwise."""
    key = ("rays", name, n)
    if key not in _cache:
        a, b = {"cornell": (0.9, 3.0), "wall": (1.0, 0.8), "soup2000": (1.5, 1.0), "soup65x2": (1.5, 1.0), "one": (1.5, 0.3)}[name]
        batch = odd_rays(make_batch(n, a, b))
        if name in GRID_SCENES:
            rays = batch.copy()
            rays[0::2] = H.as_rays(H.ray_set(name)[0])[:len(rays[0::2])]
        else:
            rays = batch
        rays.setflags(write=False)
        _cache[key] = rays
    return _cache[key]


def peel(oracle, tris, rays, cap):
    """(hits[n, cap], counts[n]): slot k of a ray is the oracle's ClosestIntersection on a fresh record against the scene in which the
    rows of the ray's slots 0 .. k - 1 are NaN; fresh records behind the ray's last hit."""
    tris = np.ascontiguousarray(tris, F32).reshape(-1, 15)
    hits = np.zeros((len(rays), cap), mirt.HIT_DTYPE)
    hits[:] = mirt.fresh_hits(1)[0]
    counts = np.zeros(len(rays), np.int32)
    with np.errstate(all="ignore"):
        for i in range(len(rays)):
            work = None
            for k in range(cap):
                _, p, d, ix = oracle.closest_intersection(tris if work is None else work, rays["start"][i], rays["dir"][i])
                if ix < 0:
                    break
                hits[i, k]["position"], hits[i, k]["distance"], hits[i, k]["index"] = p, d, ix
                counts[i] = k + 1
                if work is None:
                    work = tris.copy()
                work[ix, :] = np.nan
    return hits, counts


def peeled(oracle, name, n, cap):
    """peel() for the first n rays of the scene's set, computed once per (scene, n, cap) and left unchanged."""
    key = ("peel", name, n, cap)
    if key not in _cache:
        hits, counts = peel(oracle, scene(name), rays_of(name)[:n], cap)
        hits.setflags(write=False); counts.setflags(write=False)
        _cache[key] = hits, counts
    return _cache[key]


def table(oracle, tris, rays):
    """The per-triangle table: rec[r, j] is the record a fresh ClosestIntersection call on triangle j alone leaves for ray r
    (index 0 where it was accepted -- stored as j --, -1 where not)."""
    tris = np.ascontiguousarray(tris, F32).reshape(-1, 15)
    rays = np.ascontiguousarray(rays, mirt.RAY_DTYPE)
    rec = np.zeros((len(rays), len(tris)), mirt.HIT_DTYPE)
    rec[:] = mirt.fresh_hits(1)[0]
    # the oracle's entry point on plain addresses (the same calls as oracle.closest_intersection(tris[j:j + 1], start, dir) on a fresh
    # record, which it fills in place: millions of them without an array conversion each)
    import ctypes as C
    call = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)(("mirt_oracle_closest_intersection", oracle.lib))
    t0, r0, h0 = tris.ctypes.data, rays.ctypes.data, rec.ctypes.data
    rsize, hsize, nt = mirt.RAY_DTYPE.itemsize, mirt.HIT_DTYPE.itemsize, len(tris)
    for r in range(len(rays)):
        start, direction = r0 + r * rsize, r0 + r * rsize + 12
        for j in range(nt):
            h = h0 + (r * nt + j) * hsize
            call(start, direction, t0 + j * 60, 1, h, h + 12, h + 16)
    idx = np.broadcast_to(np.arange(nt, dtype=np.int32), rec.shape)
    rec["index"] = np.where(rec["index"] == 0, idx, -1)                # (the lone triangle was number 0 of its call)
    return rec


def tabled(oracle, name, n):
    key = ("table", name, n)
    if key not in _cache:
        t = table(oracle, scene(name), rays_of(name)[:n])
        t.setflags(write=False)
        _cache[key] = t
    return _cache[key]


def from_table(rec, after, max_hits):
    """(hits[n, max_hits], counts[n]) as the contract words it: of the accepted triangles of a ray those with FLT_MAX >= d and --
    `after` given -- d > a || (d == a && j < k), in the order d rising, j falling; float32 and int32 comparisons."""
    n = len(rec)
    hits = np.zeros((n, max_hits), mirt.HIT_DTYPE)
    hits[:] = mirt.fresh_hits(1)[0]
    counts = np.zeros(n, np.int32)
    with np.errstate(invalid="ignore"):
        for r in range(n):
            row = rec[r][rec[r]["index"] >= 0]
            d, j = row["distance"], row["index"]
            ok = F32(FLT_MAX) >= d
            if after is not None:
                a, k = after["distance"][r], after["index"][r]
                ok &= (d > a) | ((d == a) & (j < k))
            row = row[ok]
            row = row[np.lexsort((-row["index"].astype(np.int64), row["distance"]))][:max_hits]
            hits[r, :len(row)] = row
            counts[r] = len(row)
    return hits, counts


AFTER_KINDS = 11


def after_records(slot0, shift=0):
    """(records, kinds).  Per ray, in rotation from `shift` on: distance -1; the ray's own slot-0 distance with index -1, with the hit's
    index, with that index - 1 and + 1 and with INT_MAX; one float above and one float below that distance; FLT_MAX; +inf; NaN.
    (Distance 1 and index 3 where the ray hit nothing.)"""
    n = len(slot0)
    d = np.where(slot0["index"] >= 0, slot0["distance"], F32(1.0)).astype(F32)
    ix = np.where(slot0["index"] >= 0, slot0["index"], 3).astype(np.int32)
    kind = (np.arange(n) + shift) % AFTER_KINDS
    a = mirt.fresh_hits(n)
    a["position"] = 7.0                                             # (never read)
    a["distance"] = np.select([kind == 0, kind <= 5, kind == 6, kind == 7, kind == 8, kind == 9],
                              [F32(-1), d, np.nextafter(d, F32("inf")), np.nextafter(d, F32(0)), F32(FLT_MAX), F32("inf")], F32("nan")).astype(F32)
    a["index"] = np.select([kind == 1, kind == 2, kind == 3, kind == 4, kind == 5], [-1, ix, ix - 1, ix + 1, np.iinfo(np.int32).max], ix).astype(np.int32)
    return a, kind


# ---- what the tests of the ordered calls along directions and from origins (ordered_along_helpers.py, ordered_fans_helpers.py) share ----

GUARD = 16
REC = mirt.HIT_DTYPE.itemsize


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


def last_records(hits, counts, max_hits):
    """after[i] for the next call: the last record written where the ray's count reached max_hits, a fresh record (which admits
    nothing: the ray is exhausted) otherwise."""
    nxt = mirt.fresh_hits(len(hits))
    full = counts == max_hits
    nxt[full] = hits[full, max_hits - 1]
    return nxt


def guarded_host(n, max_hits):
    hbuf = np.frombuffer(np.full((n * max_hits + GUARD) * REC, 0xAA, np.uint8).tobytes(), mirt.HIT_DTYPE).copy()
    cbuf = np.frombuffer(np.full((n + GUARD) * 4, 0xAA, np.uint8).tobytes(), np.int32).copy()
    return hbuf, cbuf


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


def guarded_call(form, names, stats, head, per_ray, of, max_hits, after=None, mode=None, what="", stray=None):
    """One call through guarded buffers, host or device form: (hits[n, max_hits], counts[n], stats()).  names: the family's four entry
    points (NAMES of its helpers); head: what the rays share -- one direction or origin (3,) for the first two, or several (k, 3)
    with the rays' indices `of` (or None for k == 1) for the last two; per_ray: the rays' own (n, 3).  On the device `after` is read
    from a buffer of its own."""
    from devbuf import DeviceArray, to_device
    head = np.ascontiguousarray(head, np.float32)
    several = head.ndim == 2
    per_ray = np.ascontiguousarray(per_ray, np.float32).reshape(-1, 3)
    n = len(per_ray)
    after = None if after is None else np.ascontiguousarray(after, mirt.HIT_DTYPE)
    of = None if of is None else np.ascontiguousarray(of, np.int32)
    lib = mirt.load()
    P = mirt._ptr
    mirt.set_query_mode(mirt.QUERY_AUTO if mode is None else mode)
    try:
        if form == "host":
            hbuf, cbuf = guarded_host(n, max_hits)
            lead = (P(head), len(head), P(of)) if several else (P(head),)
            mirt._check(getattr(lib, names[2 if several else 0])(*lead, P(per_ray), n, P(after), max_hits, P(hbuf), P(cbuf)))
            return _checked(hbuf, cbuf, n, max_hits, what, stray) + (stats(),)
        held = [to_device(per_ray)] + [to_device(x) for x in (after, of) if x is not None]
        d_after = None if after is None else held[1].ptr
        d_of = None if of is None else held[-1].ptr
        try:
            with DeviceArray(((n * max_hits + GUARD) * REC,), np.uint8, 0xAA) as d_hits, DeviceArray(((n + GUARD) * 4,), np.uint8, 0xAA) as d_counts:
                lead = (head, d_of) if several else (head,)
                getattr(mirt, names[3 if several else 1][len("mirt_"):])(*lead, held[0].ptr, n, d_after, max_hits, d_hits.ptr, d_counts.ptr)
                st = stats()
                mirt.sync()
                hbuf = np.frombuffer(d_hits.read().tobytes(), mirt.HIT_DTYPE).copy()
                cbuf = np.frombuffer(d_counts.read().tobytes(), np.int32).copy()
            return _checked(hbuf, cbuf, n, max_hits, what, stray) + (st,)
        finally:
            for x in held:
                x.free()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


def bad_calls(names, one_head, several_head, bad_several_heads, no_head, per_ray, no_per_ray):
    """(entry point name, arguments, what is wrong) for every argument the family's four entry points `names` refuse --
    test_gpu_ordered_hits.py: test_errors_and_an_empty_call's and those of the family's closest-hit calls --, and the record and count
    arrays they point into: (cases, (hits, counts), snapshot()).  one_head / several_head: the leading arguments of the first and the
    last two entry points; bad_several_heads: (head, what is wrong) of the latter; no_head / no_per_ray: what a NULL head of the
    former and a NULL per-ray array are called; per_ray: the rays' own (n, 3)."""
    P = mirt._ptr
    n = len(per_ray)
    hits = np.frombuffer(np.full(n * 9 * REC, 0xAA, np.uint8).tobytes(), mirt.HIT_DTYPE).copy()
    counts = np.full(n, -1431655766, np.int32)                      # 0xAAAAAAAA
    inside = C.c_void_p(hits.ctypes.data + REC)
    H, Cn, R = P(hits), P(counts), P(per_ray)
    order = [((None, 0), "max_hits 0"), ((None, 9), "max_hits 9"), ((None, -1), "max_hits -1"),
             ((H, 2), "after == hits with two slots a ray"), ((inside, 1), "after inside hits")]
    cases = []
    for name in names:
        several = name in names[2:]
        head = several_head if several else one_head
        for (after, m), why in order:
            cases.append((name, head + (R, n, after, m, H, Cn), why))
        cases += [(name, head + (None, n, None, 2, H, Cn), no_per_ray), (name, head + (R, n, None, 2, None, Cn), "NULL hits"),
                  (name, head + (R, n, None, 2, H, None), "NULL counts"), (name, head + (R, -1, None, 2, H, Cn), "a negative count")]
        if several:
            cases += [(name, bad + (R, n, None, 2, H, Cn), why) for bad, why in bad_several_heads]
        else:
            cases.append((name, (None, R, n, None, 2, H, Cn), no_head))
    return cases, (hits, counts), lambda: (hits.tobytes(), counts.tobytes())
