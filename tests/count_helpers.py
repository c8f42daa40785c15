"""What the tests of the hit counts (test_count_host.py, test_gpu_count_hits.py) share: the deep scene `plates`, the ray sets, the CPU
oracle's expectation -- ordered_helpers.table (one oracle ClosestIntersection call per (ray, triangle) on a fresh record) with the
contract's predicate applied in numpy --, the limits and `after` records made from a ray's own hits, and the calls through
0xAA-prefilled count buffers with guard counts behind them.  Test plumbing only."""
import numpy as np

import mirt
import ordered_along_helpers as A
import ordered_helpers as O
import ray_grid_helpers as H
from along_helpers import OBLIQUE
from query_helpers import make_batch, odd_rays

F32 = np.float32
FLT_MAX = F32(np.finfo(np.float32).max)
INF, NAN = F32("inf"), F32("nan")
GUARD = 16
NAMES = ("mirt_count_hits", "mirt_count_hits_device", "mirt_count_hits_along", "mirt_count_hits_along_device",
         "mirt_count_hits_alongs", "mirt_count_hits_alongs_device")
PLATES = 24
# the three directions of the plates' cases: straight through, the oblique one, and a slanted one
PLATE_DIRS = (np.array([0, 0, 1], F32), OBLIQUE, np.array([0.3, -0.2, 1], F32))
LIMIT_KINDS = 13
_cache = {}


def plates():
    """24 squares of side 2 at z = -1.15 + 0.1 k, two triangles each: a ray through all of them has 24 hits."""
    if "plates" not in _cache:
        tris = []
        for k in range(PLATES):
            z = -1.15 + 0.1 * k
            q = [np.array([x, y, z]) for x, y in ((-1, -1), (1, -1), (-1, 1), (1, 1))]
            tris += [[q[0], q[1], q[2]], [q[3], q[2], q[1]]]
        v = H._tri_rows(np.array(tris))
        v.setflags(write=False)
        _cache["plates"] = v
    return _cache["plates"]


def scene(name):
    return plates() if name == "plates" else O.scene(name)


def rays_of(name, n):
    """n rays for a sweep: odd_rays(make_batch(n, 1.5, 1.0)) on the plates, the first n of ordered_helpers.rays_of otherwise."""
    if name == "plates":
        key = ("rays", name, n)
        if key not in _cache:
            _cache[key] = odd_rays(make_batch(n, 1.5, 1.0))
            _cache[key].setflags(write=False)
        return _cache[key]
    return O.rays_of(name)[:n]


def table_of(oracle, name, rays):
    """ordered_helpers.table for the scene and the rays, computed once per (scene, rays) and left unchanged."""
    rays = np.ascontiguousarray(rays, mirt.RAY_DTYPE)
    key = ("table", name, rays.tobytes())
    if key not in _cache:
        t = O.table(oracle, scene(name), rays)
        t.setflags(write=False)
        _cache[key] = t
    return _cache[key]


def starts_of(name, d, n):
    """ordered_along_helpers.starts_of(seed 7) for the scene along d: (starts, planted, back)."""
    d = np.ascontiguousarray(d, F32)
    key = ("starts", name, d.tobytes(), n)
    if key not in _cache:
        _cache[key] = A.starts_of(scene(name), d, n, seed=7)
        for x in _cache[key]:
            x.setflags(write=False)
    return _cache[key]


def along_case(oracle, name, d, n):
    """(tris, starts, planted, table) of scene `name` along d."""
    starts, planted, back = starts_of(name, d, n)
    return scene(name), starts, planted, table_of(oracle, name, mirt.make_rays(starts, d))


def expected(rec, after=None, limits=None):
    """The contract in numpy on the per-triangle table: per ray the number of accepted triangles with FLT_MAX >= d, behind `after`
    (d > a || (d == a && j < k)) when given, and d < limit when given; float32 and int32 comparisons."""
    d, j = rec["distance"], rec["index"]
    with np.errstate(invalid="ignore"):
        ok = (j >= 0) & (FLT_MAX >= d)
        if after is not None:
            a, k = after["distance"][:, None], after["index"][:, None]
            ok &= (d > a) | ((d == a) & (j < k))
        if limits is not None:
            ok &= d < np.asarray(limits, F32)[:, None]
    return ok.sum(axis=1).astype(np.int32)


def sorted_distances(rec):
    """Per ray the eligible distances in rising order (a list of float32 arrays)."""
    out = []
    with np.errstate(invalid="ignore"):
        for r in range(len(rec)):
            row = rec[r]
            d = row["distance"][(row["index"] >= 0) & (FLT_MAX >= row["distance"])]
            out.append(np.sort(d))
    return out


def slot0_of(rec):
    """The ray's own first hit in the reference's order (for ordered_helpers.after_records)."""
    return O.from_table(rec, None, 1)[0][:, 0]


def limits_of(rec, shift=0):
    """(limits, kinds).  Per ray, in rotation from `shift` on: the ray's first, third and last distance, each as it is, one float above
    and one float below (kinds 0 .. 8: which * 3 + how); +inf, NaN, 0 and -1 (kinds 9 .. 12).  A ray with fewer hits takes its last
    one, a ray with none the distance 1."""
    n = len(rec)
    ds = sorted_distances(rec)
    kind = (np.arange(n) + shift) % LIMIT_KINDS
    lim = np.zeros(n, F32)
    for r in range(n):
        k = int(kind[r])
        if k >= 9:
            lim[r] = (INF, NAN, F32(0), F32(-1))[k - 9]
            continue
        d = ds[r]
        base = F32(1.0) if len(d) == 0 else d[min((0, 2, len(d) - 1)[k // 3], len(d) - 1)]
        lim[r] = (base, np.nextafter(base, INF), np.nextafter(base, F32(0)))[k % 3]
    return lim, kind


# ---- calls through guarded buffers ------------------------------------------------------------------------------------------------------

def _checked(cbuf, n, what):
    raw = cbuf.view(np.uint8).reshape(-1, 4)
    assert (raw[n:] == 0xAA).all(), "%s: wrote beyond %d counts" % (what, n)
    assert not (raw[:n] == 0xAA).all(axis=1).any(), "%s: a count of the call was not written" % what
    counts = cbuf[:n].copy()
    assert (counts >= 0).all(), what
    return counts


def count_call(form, family, head, per_ray, of=None, after=None, limits=None, mode=None, what=""):
    """One call through a guarded count buffer, host or device form: (counts[n], mirt.along_stats() or None).  family: "rays" (per_ray:
    RAY_DTYPE rays; head unused), "along" (head: one direction, per_ray: (n, 3) starts) or "alongs" (head: (k, 3) directions, `of` the
    rays' indices or None for k == 1).  On the device every input is read from a buffer of its own; the inputs are checked unchanged."""
    from devbuf import DeviceArray, to_device
    lib = mirt.load()
    P = mirt._ptr
    if family == "rays":
        per_ray = np.ascontiguousarray(per_ray, mirt.RAY_DTYPE)
    else:
        per_ray = np.ascontiguousarray(per_ray, F32).reshape(-1, 3)
        head = np.ascontiguousarray(head, F32)
    n = len(per_ray)
    after = None if after is None else np.ascontiguousarray(after, mirt.HIT_DTYPE)
    limits = None if limits is None else np.ascontiguousarray(limits, F32)
    of = None if of is None else np.ascontiguousarray(of, np.int32)
    stats = (lambda: None) if family == "rays" else mirt.along_stats
    host_lead = {"rays": (), "along": (P(head),), "alongs": (P(head), len(head) if family == "alongs" else 0, P(of))}[family]
    name = {"rays": NAMES[0], "along": NAMES[2], "alongs": NAMES[4]}[family]
    before = [x.tobytes() for x in (per_ray, after, limits, of) if x is not None]
    mirt.set_query_mode(mirt.QUERY_AUTO if mode is None else mode)
    try:
        if form == "host":
            cbuf = np.frombuffer(np.full((n + GUARD) * 4, 0xAA, np.uint8).tobytes(), np.int32).copy()
            mirt._check(getattr(lib, name)(*host_lead, P(per_ray), n, P(after), P(limits), P(cbuf)))
            st = stats()
        else:
            held = {k: to_device(x) for k, x in (("rays", per_ray), ("after", after), ("limits", limits), ("of", of)) if x is not None}
            ptr = lambda k: held[k].ptr if k in held else None
            try:
                with DeviceArray(((n + GUARD) * 4,), np.uint8, 0xAA) as d_counts:
                    lead = {"rays": (), "along": (head,), "alongs": (head, ptr("of"))}[family]
                    getattr(mirt, name[len("mirt_"):] + "_device")(*lead, ptr("rays"), n, ptr("after"), ptr("limits"), d_counts.ptr)
                    st = stats()
                    mirt.sync()
                    cbuf = np.frombuffer(d_counts.read().tobytes(), np.int32).copy()
            finally:
                for x in held.values():
                    x.free()
        assert before == [x.tobytes() for x in (per_ray, after, limits, of) if x is not None], what + ": an input changed"
        return _checked(cbuf, n, what), st
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


def same_counts(got, want, what):
    assert np.array_equal(got, want), "%s: %d counts differ (first at ray %d: %d, expected %d)" % (
        what, int((got != want).sum()), int(np.flatnonzero(got != want)[0]), int(got[np.flatnonzero(got != want)[0]]), int(want[np.flatnonzero(got != want)[0]]))


def bad_calls(n=5):
    """(entry point name, arguments, what is wrong) for every argument the six entry points refuse, and the arrays the cases point
    into: (cases, keep, snapshot())."""
    P = mirt._ptr
    rays = np.zeros(n, mirt.RAY_DTYPE)
    d = np.array([0, 0, 1], F32)
    dirs = np.array([[0, 0, 1], [0, 1, 0]], F32)
    of = np.array([0, 1, 1, 0, 1], np.int32)[:n]
    origins = np.zeros((n, 3), F32)
    counts = np.full(n * 5, -1431655766, np.int32)                  # 0xAAAAAAAA; n * 20 bytes: an `after` array can lie on it
    after = mirt.fresh_hits(n)
    Cn, Aon = P(counts), P(counts.view(mirt.HIT_DTYPE))
    cases = []
    for name in NAMES:
        fam = "alongs" if "alongs" in name else ("along" if "along" in name else "rays")
        head = {"rays": (), "along": (P(d),), "alongs": (P(dirs), 2, P(of))}[fam]
        R = P(rays) if fam == "rays" else P(origins)
        cases += [(name, head + (R, -1, None, None, Cn), "a negative count"), (name, head + (None, n, None, None, Cn), "NULL rays or origins"),
                  (name, head + (R, n, None, None, None), "NULL counts"), (name, head + (R, n, Aon, None, Cn), "after overlaps counts")]
        if fam == "along":
            cases.append((name, (None, R, n, None, None, Cn), "NULL dir"))
        if fam == "alongs":
            cases += [(name, bad + (R, n, None, None, Cn), why) for bad, why in
                      (((P(dirs), -1, P(of)), "a negative direction count"), ((None, 2, P(of)), "NULL dirs"),
                       ((P(dirs), 0, P(of)), "rays but no direction"), ((P(dirs), 2, None), "NULL dir_of for two directions"))]
    keep = (rays, d, dirs, of, origins, counts, after)
    return cases, keep, lambda: counts.tobytes()
