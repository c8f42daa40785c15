"""Arbitrary rays through the cell grid on the GPU: mirt_intersect* and mirt_occluded* under mirt_set_ray_grid(1) (k_grid_closest,
k_grid_occluded) against the CPU oracle's ClosestIntersection per ray and against the same call with the switch off, bit for bit.

Scenes: Cornell (G = 4), soup2000 (G = 16) and the wall scene (G = 8; ray_grid_helpers.wall_scene).  Ray sets of 1, 63, 65 and 4097
rays (ray_grid_helpers.ray_set: uniform segments, axis-parallel rays, rays in cell faces and through cell corners, rays within one
triangle's plane and between two triangles, phantom rays, starts outside the box) with the unfit rays planted in them.  A scene's rays
and its oracle records per kind of incoming record are computed once and shared."""
import numpy as np
import pytest

import mirt
import ray_grid_helpers as H
from devbuf import DeviceArray, to_device
from query_helpers import INF, expected, make_batch, oracle_intersect, same_hits, scene_of

pytestmark = pytest.mark.gpu

GUARD = 64
COUNTS = (1, 63, 65, 4097)
SCENES = (("cornell", 4), ("wall", 8), ("soup2000", 16))
_oracle = {}


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_ray_grid(False)
    mirt.set_profiling(False)
    mirt.set_frames_in_flight(1)
    mirt.shutdown()


def want_of(oracle, name, kind):
    """(incoming records, the oracle's records after the calls) for the scene's full ray set and one kind of incoming record."""
    if (name, kind) not in _oracle:
        rays = H.as_rays(H.ray_set(name)[0])
        fresh = _oracle[name, "fresh"][1] if kind != "fresh" else None
        incoming = mirt.fresh_hits(len(rays)) if kind == "fresh" else H.incoming_records(kind, fresh)
        with np.errstate(all="ignore"):
            out = oracle_intersect(oracle, H.scene(name), rays, incoming)
        incoming.setflags(write=False); out.setflags(write=False)
        _oracle[name, kind] = incoming, out
    return _oracle[name, kind]


def intersect(on, form, rays, incoming):
    mirt.set_ray_grid(on)
    try:
        if form == "host":
            return mirt.intersect(rays, incoming)
        n = len(rays)
        d_rays, d_hits = to_device(rays), to_device(np.concatenate([incoming, mirt.fresh_hits(4)]))      # (four records of guard)
        try:
            mirt.intersect_device(d_rays.ptr, n, d_hits.ptr)
            mirt.sync()
            back = np.frombuffer(d_hits.read().tobytes(), mirt.HIT_DTYPE)
            assert back[n:].tobytes() == mirt.fresh_hits(4).tobytes(), "wrote beyond %d records" % n
            return back[:n].copy()
        finally:
            d_rays.free(); d_hits.free()
    finally:
        mirt.set_ray_grid(False)


def occluded(on, form, rays, limits, what):
    n = len(rays)
    mirt.set_ray_grid(on)
    try:
        if form == "host":
            buf = np.full(n + GUARD, 0xAA, np.uint8)
            mirt.occluded(rays, limits, buf[:n])
        else:
            d_rays, d_lim = to_device(rays), None if limits is None else to_device(limits)
            with DeviceArray((n + GUARD,), np.uint8, 0xAA) as d_out:
                try:
                    mirt.occluded_device(d_rays.ptr, n, None if d_lim is None else d_lim.ptr, d_out.ptr)
                    buf = d_out.read()
                finally:
                    d_rays.free()
                    if d_lim is not None:
                        d_lim.free()
        assert (buf[n:] == 0xAA).all(), "%s: wrote beyond %d rays" % (what, n)
        assert (buf[:n] <= 1).all(), "%s: bytes that are neither 0 nor 1" % what
        return buf[:n].copy()
    finally:
        mirt.set_ray_grid(False)


def binned(st, cells, what):
    assert st["mode_used"] == mirt.QUERY_BINNED and st["gave_up"] == 0 and st["source"] in (1, 2), (what, st)
    assert st["cells"] == cells and st["plane_bins"] == 64 and st["offset_bins"] == 64 and st["pairs"] > 0, (what, st)


# ---- the switch off ---------------------------------------------------------------------------------------------------------------------

def test_switch_off_changes_nothing(oracle):
    mirt.shutdown()                                                 # a context that has seen no call under the switch, wherever this test runs
    mirt.init(0)
    st = mirt.ray_grid_stats()
    assert st["mode_used"] == 0 and st["source"] == 0 and st["pairs"] == 0, st
    tris, a, b = scene_of("cornell")                                # test_gpu_ray_query.py's comparison, once more
    mirt.scene_upload(tris)
    rays = make_batch(300, a, b)
    same_hits(mirt.intersect(rays), oracle_intersect(oracle, tris, rays), "cornell, switch off")
    st = mirt.ray_grid_stats()
    assert st["mode_used"] == 0 and st["source"] == 0, st
    with pytest.raises(mirt.MirtError):
        mirt._check(mirt.load().mirt_set_ray_grid(2))


# ---- equality ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", H.INCOMING)
@pytest.mark.parametrize("name,cells", SCENES)
def test_records_equal_the_oracle_and_the_sweep(oracle, name, cells, kind):
    tris = H.scene(name)
    mirt.scene_upload(tris)
    r6, planted = H.ray_set(name)
    rays = H.as_rays(r6)
    want_of(oracle, name, "fresh")
    incoming, want = want_of(oracle, name, kind)
    if kind == "fresh":
        assert (want["index"] >= 0).mean() > 0.2, "the ray set hardly hits anything"
    for n in COUNTS:
        for form in ("host", "device") if n in (65, 4097) else ("host",):
            what = "%s, %s records, %d rays, %s form" % (name, kind, n, form)
            got = intersect(True, form, rays[:n], incoming[:n])
            binned(mirt.ray_grid_stats(), cells, what)
            same_hits(got, want[:n], what + " vs the oracle")
            if form == "host" or n == 65:
                same_hits(got, intersect(False, form, rays[:n], incoming[:n]), what + " vs the switch off")


@pytest.mark.parametrize("name,cells", SCENES)
def test_occlusion_bytes(oracle, name, cells):
    """Limits NULL, and at, one float above and one float below the closest distance (and +inf, 0, negative, NaN)."""
    mirt.scene_upload(H.scene(name))
    rays = H.as_rays(H.ray_set(name)[0])
    hits = want_of(oracle, name, "fresh")[1]
    d = np.where(hits["index"] >= 0, hits["distance"], np.float32(1.0)).astype(np.float32)
    k = np.arange(len(rays)) % 7
    limits = np.select([k == 0, k == 1, k == 2, k == 3, k == 4, k == 5], [d, np.nextafter(d, INF), np.nextafter(d, np.float32(0)), INF, np.float32(0), np.float32(-1)],
                       np.float32("nan")).astype(np.float32)
    assert expected(hits, limits)[k == 1].sum() > 10 and expected(hits, limits)[k == 0].sum() == 0
    for lim in (limits, None):
        for n in COUNTS:
            for form in ("host", "device") if n in (65, 4097) else ("host",):
                what = "%s, %d rays, %s form, %s" % (name, n, form, "limits" if lim is not None else "NULL limits")
                ln = None if lim is None else np.ascontiguousarray(lim[:n])
                got = occluded(True, form, rays[:n], ln, what)
                binned(mirt.ray_grid_stats(), cells, what)
                want = expected(hits[:n], ln)
                assert np.array_equal(got, want), "%s: %d bytes differ (first at ray %d)" % (what, int((got != want).sum()), int(np.flatnonzero(got != want)[0]))
                if form == "host" or n == 65:
                    assert np.array_equal(got, occluded(False, form, rays[:n], ln, what)), what + ": differs from the switch off"


def test_the_ray_sets_hold_phantoms(oracle):
    """Rays the oracle gives a hit on a triangle their exact half-line misses by more than two cells: the wall scene's set has them."""
    tris = H.scene("wall")
    ph = H.phantom_rays(tris, 64, seed=4, tries=20000)
    assert len(ph) >= 16, "the phantom generator found %d rays" % len(ph)
    t = np.asarray(tris, np.float64).reshape(-1, 15)
    rays = H.as_rays(ph)
    hits = oracle_intersect(oracle, tris, rays)
    assert (hits["index"] >= 0).all()
    # ... and the oracle's closest hit itself is such a triangle for some of them
    cen = (t[:, 0:3] + t[:, 3:6] + t[:, 6:9])[hits["index"]] / 3
    s, d = ph[:, 0:3].astype(np.float64), ph[:, 3:6].astype(np.float64)
    tt = np.maximum(0.0, ((cen - s) * d).sum(axis=1) / (d * d).sum(axis=1))
    gap = np.linalg.norm(cen - s - tt[:, None] * d, axis=1)
    assert (gap > 2 * H.grid_of(tris)[2]).sum() >= 4
    mirt.scene_upload(tris)
    same_hits(intersect(True, "host", rays, mirt.fresh_hits(len(rays))), hits, "wall, phantom rays")


# ---- statistics -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,cells", SCENES)
def test_statistics(oracle, name, cells):
    tris = H.scene(name)
    r6, planted = H.ray_set(name)
    rays = H.as_rays(r6)
    want = want_of(oracle, name, "fresh")[1]
    assert planted >= 11
    mirt.set_profiling(True)
    try:
        mirt.scene_upload(tris)
        sources = []
        for _ in range(2):
            got = intersect(True, "host", rays, mirt.fresh_hits(len(rays)))
            st = mirt.ray_grid_stats()
            binned(st, cells, name)
            sources.append(st["source"])
            same_hits(got, want, name)
            assert st["rays"] == len(rays) and st["swept_rays"] == planted, st
            assert st["pairs"] > st["plane_pairs"] + st["every_rows"] and st["plane_pairs"] > 0, st
            assert st["tests"] == st["rows_cells"] + st["rows_planes"] + st["rows_every"] + planted * len(tris), st
        assert sources == [1, 2], sources
        occluded(True, "host", rays, None, name)
        st = mirt.ray_grid_stats()
        assert st["source"] == 2 and st["rays"] == len(rays) and st["swept_rays"] == planted, st
        if name == "soup2000":
            # the uniform segments alone (every eighth ray of the set, scaled ones included), no unfit ray among them
            uni = np.ascontiguousarray(rays[0::8])
            ok = np.isfinite(r6[0::8]).all(axis=1) & (np.abs(r6[0::8, 0:3]).max(axis=1) < 2.0) & (np.abs(r6[0::8, 3:6]).max(axis=1) < 1e5) & (np.abs(r6[0::8, 3:6]).max(axis=1) > 1e-9)
            uni = np.ascontiguousarray(uni[ok])
            intersect(True, "host", uni, mirt.fresh_hits(len(uni)))
            st = mirt.ray_grid_stats()
            offered = st["rows_cells"] + st["rows_planes"] + st["rows_every"]
            print("soup2000 uniform segments: %d rays, rows offered %d = %.4f of rays x n" % (len(uni), offered, offered / (len(uni) * len(tris))))
            assert st["swept_rays"] == 0 and offered < len(uni) * len(tris) // 4, st
        # the scene moves: the structure is built again, for the moved triangles
        rot = np.array([0, 1, 0, -1, 0, 0, 0, 0, 1], np.float32)
        shift = np.array([0.25, -0.125, 0.0625], np.float32)
        mirt.scene_transform(0, len(tris), rot, shift)
        moved = mirt.transform(tris, rot, shift)
        sub = rays[:300]
        got = intersect(True, "host", sub, mirt.fresh_hits(len(sub)))
        st = mirt.ray_grid_stats()
        assert st["source"] == 1 and st["mode_used"] == mirt.QUERY_BINNED, st
        with np.errstate(all="ignore"):
            same_hits(got, oracle_intersect(oracle, moved, sub), name + ", moved")
    finally:
        mirt.set_profiling(False)


# ---- giving up, placements ----------------------------------------------------------------------------------------------------------------

def test_scenes_the_grid_does_not_serve(oracle):
    import placement as pl
    flat = np.array(mirt.scene_soup(3, 200, 0.4), np.float32)
    flat[:, 6:9] = flat[:, 0:3] + np.float32(0.5) * (flat[:, 3:6] - flat[:, 0:3])       # v2 on the edge v0 v1: zero area
    far = pl.placed_scene("soup2000", "1000_1000_1000")
    for what, tris, T in (("zero-area triangles", flat, (0, 0, 0)), ("soup2000 at (1000, 1000, 1000)", far, (1000, 1000, 1000))):
        mirt.scene_upload(tris)
        r6 = H.ray_set("soup2000", 257, seed=9)[0].copy()
        r6[:, 0:3] = pl.place(r6[:, 0:3], T, 1.0)
        rays = H.as_rays(r6)
        got = intersect(True, "host", rays, mirt.fresh_hits(len(rays)))
        st = mirt.ray_grid_stats()
        assert st["mode_used"] == mirt.QUERY_BRUTE, (what, st)
        assert st["gave_up"] == 1 or st["source"] == 0, (what, st)
        with np.errstate(all="ignore"):
            same_hits(got, oracle_intersect(oracle, tris, rays), what)
        occ = occluded(True, "host", rays, None, what)
        assert np.array_equal(occ, expected(got, None)), what


def test_a_placed_scene_bins(oracle):
    import placement as pl
    tris = pl.placed_scene("soup2000", "3_0_0")
    mirt.scene_upload(tris)
    r6 = H.ray_set("soup2000", 1025, seed=11)[0].copy()
    r6[:, 0:3] = pl.place(r6[:, 0:3], (3, 0, 0), 1.0)
    rays = H.as_rays(r6)
    got = intersect(True, "host", rays, mirt.fresh_hits(len(rays)))
    binned(mirt.ray_grid_stats(), 16, "soup2000 at (3, 0, 0)")
    with np.errstate(all="ignore"):
        want = oracle_intersect(oracle, tris, rays)
    same_hits(got, want, "soup2000 at (3, 0, 0)")
    assert (want["index"] >= 0).mean() > 0.2


# ---- streams ------------------------------------------------------------------------------------------------------------------------------

def test_two_streams_right_after_a_scene_change(oracle):
    name = "wall"
    rays = H.as_rays(H.ray_set(name)[0])[:1025]
    want = want_of(oracle, name, "fresh")[1][:1025]
    n = len(rays)
    mirt.set_frames_in_flight(2)
    try:
        mirt.scene_upload(H.scene("cornell"))
        mirt.set_ray_grid(True)
        d_rays = to_device(rays)
        outs = [to_device(mirt.fresh_hits(n)) for _ in range(4)]
        try:
            mirt.intersect_device(d_rays.ptr, n, outs[0].ptr)           # (the other scene's structure is in place)
            mirt.scene_upload(H.scene(name))
            outs[0].free()
            outs[0] = to_device(mirt.fresh_hits(n))
            for o in outs:                                              # four calls on alternating streams: the first one builds
                mirt.intersect_device(d_rays.ptr, n, o.ptr)
            mirt.sync()
            for k, o in enumerate(outs):
                same_hits(np.frombuffer(o.read().tobytes(), mirt.HIT_DTYPE), want, "wall, call %d of 4 on two streams" % k)
        finally:
            d_rays.free()
            for o in outs:
                o.free()
    finally:
        mirt.set_ray_grid(False)
        mirt.set_frames_in_flight(1)
