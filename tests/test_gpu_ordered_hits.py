"""Every hit along a ray, in order, on the GPU: mirt_intersect_ordered* (k_order_sweep_wave, k_order_sweep, k_grid_order) against the
CPU oracle, byte for byte.

The oracle's expectation (ordered_helpers.py).  Enumerated from the start, slot k of a ray is oracle.closest_intersection on a fresh
record against the scene in which the rows of the triangles already reported for that ray are NaN (peel).  Behind an arbitrary `after`
record it is the per-triangle table -- one oracle call per (ray, triangle) -- filtered and sorted as the contract words it
(from_table); on 64 .. 257 rays the two agree on every scene here (asserted below, on the CPU).

Every call goes through buffers prefilled with 0xAA with guard records and guard counts behind them: each slot and count of the call
is written, and nothing beyond.  Ray counts 1, 63, 65 and 257 reach the wave kernel, 4097 the lane kernel (max_hits 2 there); the switch
of mirt_set_ray_grid off and on; host and device forms."""
import ctypes as C

import numpy as np
import pytest

import mirt
import ordered_helpers as O
from devbuf import DeviceArray, to_device
from query_helpers import make_batch, scene_of

pytestmark = pytest.mark.gpu

GUARD = 16
SCENES = ("cornell", "wall", "soup2000", "soup65x2", "one")
HITS = (1, 2, 3, 4, 5, 8)
REC = mirt.HIT_DTYPE.itemsize


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_ray_grid(False)
    mirt.set_profiling(False)
    mirt.set_frames_in_flight(1)
    mirt.shutdown()


def _checked(hbuf, cbuf, n, max_hits, what):
    """The call's records and counts out of the 0xAA-prefilled buffers: all written, the guards untouched."""
    hraw = hbuf.view(np.uint8).reshape(-1, REC)
    craw = cbuf.view(np.uint8).reshape(-1, 4)
    assert (hraw[n * max_hits:] == 0xAA).all(), "%s: wrote beyond %d x %d records" % (what, n, max_hits)
    assert (craw[n:] == 0xAA).all(), "%s: wrote beyond %d counts" % (what, n)
    assert not (hraw[:n * max_hits] == 0xAA).all(axis=1).any(), "%s: a slot of the call was not written" % what
    assert not (craw[:n] == 0xAA).all(axis=1).any(), "%s: a count of the call was not written" % what
    hits = hbuf[:n * max_hits].reshape(n, max_hits).copy()
    counts = cbuf[:n].copy()
    assert ((counts >= 0) & (counts <= max_hits)).all(), what
    return hits, counts


def ordered(form, rays, max_hits, after=None, grid=False, what=""):
    """One call through guarded buffers: (hits[n, max_hits], counts[n])."""
    n = len(rays)
    rays = np.ascontiguousarray(rays)
    after = None if after is None else np.ascontiguousarray(after, mirt.HIT_DTYPE)
    lib = mirt.load()
    mirt.set_ray_grid(grid)
    try:
        if form == "host":
            hbuf = np.frombuffer(np.full((n * max_hits + GUARD) * REC, 0xAA, np.uint8).tobytes(), mirt.HIT_DTYPE).copy()
            cbuf = np.frombuffer(np.full((n + GUARD) * 4, 0xAA, np.uint8).tobytes(), np.int32).copy()
            mirt._check(lib.mirt_intersect_ordered(mirt._ptr(rays), n, mirt._ptr(after), max_hits, mirt._ptr(hbuf), mirt._ptr(cbuf)))
            return _checked(hbuf, cbuf, n, max_hits, what)
        d_rays, d_after = to_device(rays), None if after is None else to_device(after)
        try:
            with DeviceArray(((n * max_hits + GUARD) * REC,), np.uint8, 0xAA) as d_hits, DeviceArray(((n + GUARD) * 4,), np.uint8, 0xAA) as d_counts:
                mirt.intersect_ordered_device(d_rays.ptr, n, None if d_after is None else d_after.ptr, max_hits, d_hits.ptr, d_counts.ptr)
                hbuf = np.frombuffer(d_hits.read().tobytes(), mirt.HIT_DTYPE).copy()
                cbuf = np.frombuffer(d_counts.read().tobytes(), np.int32).copy()
            return _checked(hbuf, cbuf, n, max_hits, what)
        finally:
            d_rays.free()
            if d_after is not None:
                d_after.free()
    finally:
        mirt.set_ray_grid(False)


def same(got, want, what):
    gh, gc = got
    wh, wc = want
    assert np.array_equal(gc, wc), "%s: %d counts differ (first at ray %d)" % (what, int((gc != wc).sum()), int(np.flatnonzero(gc != wc)[0]))
    assert np.array_equal(gh["index"], wh["index"]), "%s: index differs in %d slots" % (what, int((gh["index"] != wh["index"]).sum()))
    assert np.array_equal(gh["distance"].view(np.uint32), wh["distance"].view(np.uint32)), "%s: distance not bit-identical" % what
    assert gh.tobytes() == wh.tobytes(), "%s: position not bit-identical" % what


def binned(name, what):
    st = mirt.ray_grid_stats()
    if name in O.GRID_SCENES:
        assert st["mode_used"] == mirt.QUERY_BINNED and st["gave_up"] == 0 and st["source"] in (1, 2) and st["cells"] == O.GRID_SCENES[name], (what, st)
    else:
        assert st["mode_used"] in (mirt.QUERY_BRUTE, mirt.QUERY_BINNED), (what, st)


def prefix(want, n, max_hits):
    """The expectation for the first n rays and max_hits slots out of an enumeration of at least that many."""
    hits, counts = want
    return np.ascontiguousarray(hits[:n, :max_hits]), np.minimum(counts[:n], max_hits).astype(np.int32)


# ---- 1, 2, 5: records, counts and trailing fresh slots; the guards; rays outside the filter's range ------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_records_equal_the_oracle(oracle, name):
    tris = O.scene(name)
    mirt.scene_upload(tris)
    rays = O.rays_of(name)
    want8 = O.peeled(oracle, name, 257, 8)
    want2 = O.peeled(oracle, name, 4097, 2)
    if name != "one":
        assert (want8[1] > 0).mean() >= 0.2 and (want2[1] > 0).mean() >= 0.2, "the ray set hardly hits anything"
    if name in ("soup2000", "soup65x2"):
        assert (want8[1] >= 2).mean() >= 0.2 and (want2[1] >= 2).mean() >= 0.2, "hardly a ray has a second hit"
    if name == "soup65x2":
        h = want8[0]
        assert ((h["distance"][:, 1:] == h["distance"][:, :-1]) & (h["index"][:, 1:] >= 0) & (h["index"][:, 1:] < h["index"][:, :-1])).sum() > 50, "no ties"
    # (the rays outside the filter's range and the grid's window are among them: odd_rays at 11, 93, ..., ray_set's planted ones at 14, 218, ...)
    with np.errstate(invalid="ignore"):
        assert (np.abs(rays["start"][:257]) > 1e8).any() and not np.isfinite(rays["dir"][:257]).all() and not rays["dir"][:257].any(axis=1).all()
    fresh = mirt.intersect(rays)
    cases = [(n, m) for n in (1, 63, 65, 257) for m in HITS] + [(4097, 2)]
    for n, m in cases:
        want = prefix(want8 if n <= 257 else want2, n, m)
        for form in ("host", "device") if n in (65, 4097) else ("host",):
            what = "%s, %d rays, max_hits %d, %s form" % (name, n, m, form)
            off = ordered(form, rays[:n], m, what=what)
            same(off, want, what + " vs the oracle")
            on = ordered(form, rays[:n], m, grid=True, what=what + ", grid")
            binned(name, what)
            same(on, want, what + ", grid vs the oracle")
            same(on, off, what + ", the switch on vs off")
            # slot 0 is mirt_intersect on a fresh record
            hit = off[1] > 0
            assert np.array_equal(hit, fresh["index"][:n] >= 0), what
            assert off[0][:, 0][hit].tobytes() == fresh[:n][hit].tobytes(), what + ": slot 0 is not mirt_intersect's record"
            assert off[0][:, 0][~hit].tobytes() == mirt.fresh_hits(int((~hit).sum())).tobytes(), what


def test_the_wrapper_returns_the_same(oracle):
    name = "soup2000"
    mirt.scene_upload(O.scene(name))
    rays = O.rays_of(name)[:257]
    hits, counts = mirt.intersect_ordered(rays, 4)
    assert hits.shape == (257, 4) and counts.shape == (257,)
    same((hits, counts), prefix(O.peeled(oracle, name, 257, 8), 257, 4), "mirt.intersect_ordered")


# ---- 3: continuation ----------------------------------------------------------------------------------------------------------------------

def _last_records(hits, counts, max_hits):
    """after[i] for the next call: the last record written where the ray's count reached max_hits, a fresh record (which admits
    nothing: the ray is exhausted) otherwise."""
    nxt = mirt.fresh_hits(len(hits))
    full = counts == max_hits
    nxt[full] = hits[full, max_hits - 1]
    return nxt


@pytest.mark.parametrize("grid", (False, True))
@pytest.mark.parametrize("name", ("soup2000", "soup65x2"))
def test_continuation_enumerates_every_hit(oracle, name, grid):
    tris = O.scene(name)
    mirt.scene_upload(tris)
    a, b = scene_of("soup2000" if name == "soup2000" else "soup65")[1:]
    rays = make_batch(64, a, b, seed=7)
    key = ("full", name)
    if key not in O._cache:
        O._cache[key] = O.peel(oracle, tris, rays, 40)
    wh, wc = O._cache[key]
    assert wc.max() < 40
    if name == "soup2000":
        assert wc.max() > 8, "no ray has more than 8 hits"
    else:
        assert ((wh["distance"][:, 1:] == wh["distance"][:, :-1]) & (wh["index"][:, 1:] >= 0)).sum() > 20, "no ties"
    # max_hits = 2, again and again behind each ray's last record
    parts, after = [], None
    for rnd in range(25):
        hits, counts = ordered("host" if rnd % 2 == 0 else "device", rays, 2, after=after, grid=grid, what="%s, round %d" % (name, rnd))
        parts.append(hits)
        if (counts < 2).all():
            break
        after = _last_records(hits, counts, 2)
    else:
        raise AssertionError("the enumeration does not end")
    got = np.concatenate(parts, axis=1)
    assert got.shape[1] >= wc.max()
    width = max(got.shape[1], wh.shape[1])
    pad = lambda h: np.concatenate([h, np.broadcast_to(mirt.fresh_hits(1)[0], (len(h), width - h.shape[1]))], axis=1)
    assert pad(got).tobytes() == pad(wh).tobytes(), "%s: the concatenated rounds differ from the oracle's enumeration" % name
    # the in-place peel: max_hits == 1, after == hits; started behind distance -1, which admits everything
    mirt.set_ray_grid(grid)
    try:
        start = mirt.fresh_hits(len(rays))
        start["distance"] = -1.0
        d_rays, d_rec = to_device(rays), to_device(start)
        host_rec = start.copy()
        cnt = np.zeros(len(rays), np.int32)
        try:
            with DeviceArray((len(rays),), np.int32, 0xAA) as d_cnt:
                for k in range(int(wc.max()) + 1):
                    mirt.intersect_ordered_device(d_rays.ptr, len(rays), d_rec.ptr, 1, d_rec.ptr, d_cnt.ptr)
                    rec = np.frombuffer(d_rec.read().tobytes(), mirt.HIT_DTYPE)
                    assert rec.tobytes() == np.ascontiguousarray(wh[:, k]).tobytes(), "%s: in-place peel, device form, step %d" % (name, k)
                    assert np.array_equal(d_cnt.read(), (wc > k).astype(np.int32))
                    mirt._check(mirt.load().mirt_intersect_ordered(mirt._ptr(rays), len(rays), mirt._ptr(host_rec), 1, mirt._ptr(host_rec), mirt._ptr(cnt)))
                    assert host_rec.tobytes() == rec.tobytes() and np.array_equal(cnt, (wc > k).astype(np.int32)), "%s: in-place peel, host form, step %d" % (name, k)
        finally:
            d_rays.free(); d_rec.free()
    finally:
        mirt.set_ray_grid(False)


# ---- 4: `after` records of every kind -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n", (("soup2000", 64), ("soup65x2", 257), ("cornell", 257)))
def test_after_records(oracle, name, n):
    mirt.scene_upload(O.scene(name))
    rays = O.rays_of(name)[:n]
    rec = O.tabled(oracle, name, n)
    # the two expectations agree where both apply
    same(O.from_table(rec, None, 8), prefix(O.peeled(oracle, name, 257, 8), n, 8), name + ": table vs peel")
    slot0 = O.from_table(rec, None, 1)[0][:, 0]
    for shift in (0, 4, 8):                                         # (every ray meets three of the kinds)
        after, kind = O.after_records(slot0, shift)
        for m in (1, 3, 8):
            want = O.from_table(rec, after, m)
            for grid in (False, True):
                what = "%s, after kinds from %d on, max_hits %d, grid %s" % (name, shift, m, grid)
                same(ordered("host", rays, m, after=after, grid=grid, what=what), want, what)
        want = O.from_table(rec, after, 3)
        same(ordered("device", rays, 3, after=after, grid=True, what=name), want, name + ", device form")
        c = want[1]
        hit = slot0["index"] >= 0
        # behind -1: everything; behind the hit itself with index - 1: nothing of that triangle, so fewer than from the start
        assert np.array_equal(c[kind == 0], O.from_table(rec, None, 3)[1][kind == 0])
        assert c[kind == 0].sum() > 0 and c[kind == 7].sum() > 0 and c[kind >= 8].sum() == 0, "the kinds do not admit what they should"
        assert (want[0][:, 0]["index"][(kind == 4) & hit] == slot0["index"][(kind == 4) & hit]).all(), "a tie record with index + 1 admits the hit itself"
        assert (want[0][:, 0]["index"][(kind == 2) & hit] != slot0["index"][(kind == 2) & hit]).all()


# ---- 6: errors ------------------------------------------------------------------------------------------------------------------------------

def test_errors_and_an_empty_call():
    mirt.scene_upload(O.scene("cornell"))
    lib = mirt.load()
    rays = np.ascontiguousarray(O.rays_of("cornell")[:5])
    hits = np.frombuffer(np.full(5 * 9 * REC, 0xAA, np.uint8).tobytes(), mirt.HIT_DTYPE).copy()
    counts = np.full(5, -1431655766, np.int32)                      # 0xAAAAAAAA
    before_h, before_c = hits.tobytes(), counts.tobytes()
    P = mirt._ptr
    bad = [(P(rays), 5, None, 0, P(hits), P(counts)), (P(rays), 5, None, 9, P(hits), P(counts)), (P(rays), 5, None, -1, P(hits), P(counts)),
           (None, 5, None, 2, P(hits), P(counts)), (P(rays), 5, None, 2, None, P(counts)), (P(rays), 5, None, 2, P(hits), None),
           (P(rays), -1, None, 2, P(hits), P(counts)),
           # `after` inside `hits`, and after == hits with more than one slot a ray
           (P(rays), 5, P(hits), 2, P(hits), P(counts)), (P(rays), 5, C.c_void_p(hits.ctypes.data + REC), 1, P(hits), P(counts))]
    for fn in (lib.mirt_intersect_ordered, lib.mirt_intersect_ordered_device):
        for args in bad:
            assert fn(*args) == -3, args                            # MIRT_ERR_INVALID_ARGUMENT
            assert lib.mirt_last_error(), args
            with pytest.raises(mirt.MirtError):
                mirt._check(fn(*args))
        assert fn(P(rays), 0, None, 2, P(hits), P(counts)) == 0
        assert fn(None, 0, None, 8, None, None) == 0
    assert hits.tobytes() == before_h and counts.tobytes() == before_c, "a refused or empty call wrote something"


# ---- 7: a scene change; streams ---------------------------------------------------------------------------------------------------------------

def test_a_moved_scene_and_two_streams(oracle):
    name = "wall"
    tris = O.scene(name)
    rays = np.ascontiguousarray(O.rays_of(name)[:257])
    mirt.scene_upload(tris)
    same(ordered("host", rays, 4, grid=True), prefix(O.peeled(oracle, name, 257, 8), 257, 4), "wall")
    assert mirt.ray_grid_stats()["source"] == 1
    ordered("host", rays, 4, grid=True)
    assert mirt.ray_grid_stats()["source"] == 2
    rot = np.array([0, 1, 0, -1, 0, 0, 0, 0, 1], np.float32)
    shift = np.array([0.25, -0.125, 0.0625], np.float32)
    mirt.scene_transform(0, len(tris), rot, shift)
    moved = mirt.transform(tris, rot, shift)
    got = ordered("host", rays, 4, grid=True)
    st = mirt.ray_grid_stats()
    assert st["source"] == 1 and st["mode_used"] == mirt.QUERY_BINNED, st
    want = O.peel(oracle, moved, rays, 4)
    same(got, want, "wall, moved")
    assert (want[1] > 0).mean() > 0.2
    same(ordered("host", rays, 4), want, "wall, moved, the switch off")
    # four device calls on two streams right after an upload: the first one builds
    n = len(rays)
    want = prefix(O.peeled(oracle, name, 257, 8), 257, 4)
    mirt.set_frames_in_flight(2)
    try:
        mirt.set_ray_grid(True)
        d_rays = to_device(rays)
        outs = [(DeviceArray((n * 4 * REC,), np.uint8, 0xAA), DeviceArray((n,), np.int32, 0xAA)) for _ in range(4)]
        try:
            mirt.scene_upload(tris)
            for h, c in outs:
                mirt.intersect_ordered_device(d_rays.ptr, n, None, 4, h.ptr, c.ptr)
            mirt.sync()
            for k, (h, c) in enumerate(outs):
                got = np.frombuffer(h.read().tobytes(), mirt.HIT_DTYPE).reshape(n, 4), c.read()
                same(got, want, "wall, call %d of 4 on two streams" % k)
        finally:
            d_rays.free()
            for h, c in outs:
                h.free(); c.free()
    finally:
        mirt.set_ray_grid(False)
        mirt.set_frames_in_flight(1)
