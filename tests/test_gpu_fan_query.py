"""Origin fans on the GPU: mirt_intersect_from* -- many directions from one origin through a cube around it (k_query_fan_binned)
or by a sweep of the origin's table (k_query_fan) -- against mirt_intersect on the rays {origin, dir} and against the CPU
oracle's ClosestIntersection.

Every comparison is bit-exact and covers every ray of its batch: `index` equal, `distance` and `position` compared as uint32
views (NaN payloads count).  The oracle sees the first 1024 rays of a larger batch; the 26 axis, face-diagonal and corner
directions and their one-ulp neighbours -- the face seams of cube_bin_of -- come first in every batch."""
import ctypes as C

import numpy as np
import pytest

import mirt
from devbuf import hip_fill, to_device
from query_helpers import INSIDE, LIGHTS, OUTSIDE, oracle_intersect, primary_rays, same_hits, seam_directions
from query_helpers import fan_scene_of as scene_of

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
NDIRS = 4096
ORACLE_RAYS = 1024


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_query_mode(mirt.QUERY_AUTO)
    mirt.set_profiling(False)
    mirt.set_frames_in_flight(1)
    mirt.shutdown()


# ---- scenes, origins, directions -----------------------------------------------------------------------------------------

def origins_of(tris):
    """Inside the scene, outside its box, and exactly on a vertex of triangle 0."""
    return {"inside": INSIDE, "outside": OUTSIDE, "vertex": np.array(tris[0, 0:3], np.float32)}


def directions_from(origin, b, n=NDIRS, seed=7):
    """The seam directions, then n directions towards U[-b, b]^3."""
    rng = np.random.default_rng(seed)
    target = rng.uniform(-b, b, (n, 3)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([seam_directions(), (target - np.asarray(origin, np.float32)).astype(np.float32)]))


def fan(origin, dirs, mode, hits=None):
    mirt.set_query_mode(mode)
    try:
        out = mirt.intersect_from(origin, dirs, hits)
        return out, mirt.fan_stats()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


# ---- 1. the modes agree ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell", "soup2000", "soup65", "one", "cornell+soup2000"])
def test_modes_agree(oracle, name):
    tris, b = scene_of(name)
    mirt.scene_upload(tris)
    shares = {}
    for oname, origin in origins_of(tris).items():
        what = "%s from %s" % (name, oname)
        dirs = directions_from(origin, b)
        assert len(dirs) == 26 * 7 + NDIRS
        rays = mirt.make_rays(origin, dirs)
        want = mirt.intersect(rays)
        brute, sb = fan(origin, dirs, mirt.QUERY_BRUTE)
        binned, st = fan(origin, dirs, mirt.QUERY_BINNED)
        assert sb["mode_used"] == mirt.QUERY_BRUTE and sb["cube_source"] == 0 and sb["cube_bins"] == 0
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 1 and st["cube_bins"] in (64, 128, 256) and st["shells"] >= 1
        same_hits(brute, want, what + ": brute vs mirt.intersect")
        same_hits(binned, want, what + ": binned vs mirt.intersect")
        same_hits(binned[:ORACLE_RAYS], oracle_intersect(oracle, tris, rays[:ORACLE_RAYS]), what + ": binned vs oracle")
        shares[oname] = float((binned["index"] >= 0).mean())
        miss = binned["index"] < 0                               # a miss leaves the fresh record as it was
        assert np.all(binned["distance"][miss] == FLT_MAX) and not binned["position"][miss].any()
    print(name, "hit shares", shares)
    if name.startswith("soup"):
        # neither branch is vacuous.  From a vertex of triangle 0 every ray that is not parallel to that triangle meets it at
        # t = u = v = 0, so that origin's share is 1 by construction; the share of the scene's rays over the three origins, and of
        # each of the two other origins alone, lies inside the range
        assert 0.05 <= np.mean(list(shares.values())) <= 0.95, shares
        assert 0.05 <= shares["inside"] <= 0.95 and 0.05 <= shares["outside"] <= 0.95, shares
        assert shares["vertex"] > 0.99, shares


# ---- 2. the bins are used ---------------------------------------------------------------------------------------------------

def test_the_bins_are_used(oracle):
    """candidates < rays x n / 4 is a condition, not a measurement.  What to expect, from the CPU alone (the oracle's hits of these
    rays from this origin): 0.89 of the rays hit, at a median distance of 0.37 against a scene depth of 2.0 from the origin, so
    most walks end in the first quarter of their bin's shells; and a whole bin list is short -- the triangles whose bounding
    disc, widened by two bins of a 128 x 128 face, holds a ray's direction number 33 on average and 50 at most over 512 of these
    rays.  Some tens of rows a ray against the bound's n / 4 = 500."""
    tris, b = scene_of("soup2000")
    n = len(tris)
    mirt.scene_upload(tris)
    dirs = directions_from(INSIDE, b)
    want = mirt.intersect(mirt.make_rays(INSIDE, dirs))
    mirt.set_profiling(True)
    try:
        binned, st = fan(INSIDE, dirs, mirt.QUERY_BINNED)
        brute, sb = fan(INSIDE, dirs, mirt.QUERY_BRUTE)
    finally:
        mirt.set_profiling(False)
    print(st, "rows per ray %.1f" % (st["candidates"] / len(dirs)))
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 1
    assert st["shadow_rays"] == len(dirs)
    assert 0 < st["candidates"] < len(dirs) * n / 4
    assert 0 < st["tests"] <= st["candidates"]
    assert st["fallback_records"] == 0
    assert sb["mode_used"] == mirt.QUERY_BRUTE and sb["cube_source"] == 0 and sb["candidates"] == 0
    same_hits(binned, want, "profiled kernel")
    same_hits(brute, want, "brute")
    # without profiling the counters stay zero
    _, st = fan(INSIDE, dirs, mirt.QUERY_BINNED)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2 and st["candidates"] == 0 and st["shadow_rays"] == 0
    assert mirt.load().mirt_get_fan_stats(None) == -3


# ---- 3. direction length ------------------------------------------------------------------------------------------------------

SCALES = np.array([2.0 ** -10, 2.0 ** 10, 3e-5, 1e3, 0.37], np.float32)


def test_direction_length(oracle):
    tris, b = scene_of("soup2000")
    mirt.scene_upload(tris)
    dirs = directions_from(INSIDE, b)
    unscaled, _ = fan(INSIDE, dirs, mirt.QUERY_BINNED)
    assert 0.05 <= (unscaled["index"] >= 0).mean() <= 0.95
    scaled = (dirs * SCALES[np.arange(len(dirs)) % len(SCALES)][:, None]).astype(np.float32)       # mixed within every wave
    want = mirt.intersect(mirt.make_rays(INSIDE, scaled))
    mirt.set_profiling(True)
    try:
        for mode in (mirt.QUERY_BINNED, mirt.QUERY_BRUTE):
            got, st = fan(INSIDE, scaled, mode)
            assert np.array_equal(got["index"], unscaled["index"]), "mode %d: %d indices moved with the direction's length" % (
                mode, int((got["index"] != unscaled["index"]).sum()))
            same_hits(got, want, "scaled directions, mode %d" % mode)
            if mode == mirt.QUERY_BINNED:
                assert st["mode_used"] == mirt.QUERY_BINNED and st["fallback_records"] == 0          # all inside the window
        same_hits(got[:ORACLE_RAYS], oracle_intersect(oracle, tris, mirt.make_rays(INSIDE, scaled)[:ORACLE_RAYS]), "scaled directions vs oracle")

        # directions outside the window, scattered among ordinary ones
        odd_dirs = dirs.copy()
        rng = np.random.default_rng(11)
        odd = rng.permutation(len(dirs))[:600]
        for k, i in enumerate(odd):
            kind = k % 5
            if kind == 0:
                odd_dirs[i] = dirs[i] * np.float32(1e-30)
            elif kind == 1:
                odd_dirs[i] = dirs[i] * np.float32(1e30)          # beyond the direction bound too: the exact-only override
            elif kind == 2:
                odd_dirs[i] = 0
            elif kind == 3:
                odd_dirs[i][k % 3] = np.float32("nan")
            else:
                odd_dirs[i][k % 3] = np.float32("inf") * (1 if k % 2 else -1)
        assert np.all(np.abs(dirs[odd]).max(axis=1) > 1e-3) and np.all(np.abs(dirs[odd]).max(axis=1) < 1e3)
        rays = mirt.make_rays(INSIDE, odd_dirs)
        want = mirt.intersect(rays)
        got, st = fan(INSIDE, odd_dirs, mirt.QUERY_BINNED)
        same_hits(got, want, "directions outside the window")
        assert st["mode_used"] == mirt.QUERY_BINNED and st["fallback_records"] == len(odd)
        same_hits(fan(INSIDE, odd_dirs, mirt.QUERY_BRUTE)[0], want, "directions outside the window, brute")
        first = np.sort(odd)[:256]
        same_hits(got[first], oracle_intersect(oracle, tris, rays[first]), "directions outside the window vs oracle")
        assert (got["index"][odd[0::5]] >= 0).any() and (got["index"][odd[1::5]] >= 0).any()       # tiny and huge ones do find hits
    finally:
        mirt.set_profiling(False)


# ---- 4. carried records and ties ----------------------------------------------------------------------------------------------

def test_carried_records_and_ties(oracle):
    tris, b = scene_of("cornell x 2")
    box = tris[:30]
    mirt.scene_upload(tris)
    origin = np.array([0.125, -0.0625, -0.25], np.float32)
    dirs = directions_from(origin, b)
    rays = mirt.make_rays(origin, dirs)
    fresh, _ = fan(origin, dirs, mirt.QUERY_BINNED)
    hit = fresh["index"] >= 0
    assert hit.sum() > 2000 and np.all(fresh["index"][hit] >= 30)           # every hit names the later copy
    same_hits(fresh, mirt.intersect(rays), "cornell x 2")
    single = oracle_intersect(oracle, box, rays[:ORACLE_RAYS])
    assert np.array_equal(np.where(hit[:ORACLE_RAYS], fresh["index"][:ORACLE_RAYS] - 30, -1), single["index"])

    # incoming records, mixed per ray
    rec = mirt.fresh_hits(len(dirs))
    kind = np.arange(len(dirs)) % 8
    own = kind != 0                                                          # 0: fresh
    rec["position"][own] = (9, 9, 9)
    rec["index"][own] = 7
    rec["distance"][kind == 1] = 0
    rec["distance"][kind == 2] = fresh["distance"][kind == 2]               # equal to the ray's own hit distance: loses the tie
    rec["distance"][kind == 3] = np.nextafter(fresh["distance"][kind == 3], np.float32(0))       # just below: stays, all 20 bytes
    rec["distance"][kind == 4] = -1
    rec["distance"].view(np.uint32)[kind == 5] = 0x7fc12345                 # NaN with a payload
    rec["distance"][kind == 6] = np.float32("inf")
    rec["distance"][kind == 7] = 1.0                                        # a record of the caller's own somewhere in the scene
    rec["index"][kind == 7] = 123456
    want = mirt.intersect(rays, rec)
    for mode in (mirt.QUERY_BINNED, mirt.QUERY_BRUTE):
        got, _ = fan(origin, dirs, mode, rec)
        same_hits(got, want, "carried records, mode %d" % mode)
        same_hits(got[hit & (kind == 2)], fresh[hit & (kind == 2)], "equal: replaced")
        for k in (3, 4, 5):
            assert got[kind == k].tobytes() == rec[kind == k].tobytes(), k
        keep = (kind == 1) & ~(hit & (fresh["distance"] == 0))
        assert got[keep].tobytes() == rec[keep].tobytes()
        same_hits(got[hit & (kind == 6)], fresh[hit & (kind == 6)], "inf: replaced")
        assert got[~hit & (kind == 6)].tobytes() == rec[~hit & (kind == 6)].tobytes()
        assert (got["index"][kind == 7] == 123456).any() and (got["index"][kind == 7] != 123456).any()
    same_hits(got[:ORACLE_RAYS], oracle_intersect(oracle, tris, rays[:ORACLE_RAYS], rec[:ORACLE_RAYS]), "carried records vs oracle")
    # ties at distance 0: from a shared vertex every triangle around it is met at t = 0; the latest index wins
    corner = np.array(tris[0, 0:3], np.float32)
    d0 = directions_from(corner, b)
    same_hits(fan(corner, d0, mirt.QUERY_BINNED)[0], mirt.intersect(mirt.make_rays(corner, d0)), "ties at a vertex")


# ---- 5. the frame path ----------------------------------------------------------------------------------------------------------

def test_fans_equal_the_frame_path(oracle):
    W, H, cam, focal = 64, 48, (0.1, -0.05, -2.0), 40.0
    rot = oracle.rot_from_yaw(0.15, 1.0)
    tris, _ = scene_of("cornell+soup2000")
    mirt.scene_upload(tris)
    frame = mirt.raytrace(mirt.make_view(cam, rot, focal, W, H), LIGHTS, mode=mirt.RT_BRUTE, want_intersection=True)
    dirs = np.ascontiguousarray(primary_rays(oracle, cam, rot, focal, W, H)["dir"])
    for mode in (mirt.QUERY_BINNED, mirt.QUERY_BRUTE):
        hits, st = fan(cam, dirs, mode)
        assert st["mode_used"] == mode
        assert np.array_equal(hits["index"], frame["index"].ravel())
        assert np.array_equal(hits["distance"].view(np.uint32), frame["dist"].ravel().view(np.uint32)), "distance plane"
        assert np.array_equal(hits["position"].view(np.uint32), np.ascontiguousarray(frame["pos"].reshape(-1, 3)).view(np.uint32)), "position plane"
    assert (hits["index"] >= 0).sum() > 1000


# ---- 6. cache and streams -----------------------------------------------------------------------------------------------------

def test_cube_cache(oracle):
    tris, b = scene_of("soup2000")
    mirt.scene_upload(tris)
    dirs = directions_from(INSIDE, b, 1024)
    want = mirt.intersect(mirt.make_rays(INSIDE, dirs))
    frame = mirt.raytrace(mirt.make_view((0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 32.0, 64, 64), LIGHTS)
    stats0 = mirt.stats()
    assert stats0 == frame["stats"]
    recs = want[want["index"] >= 0]
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        lit = mirt.direct_light(recs, LIGHTS)
        qs0 = mirt.query_stats()
        assert qs0["mode_used"] == mirt.QUERY_BINNED and qs0["cube_source"] == 1
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
    out, st = fan(INSIDE, dirs, mirt.QUERY_BINNED)
    assert st["cube_source"] == 1
    same_hits(out, want, "built")
    out, st = fan(INSIDE, dirs, mirt.QUERY_BINNED)
    assert st["cube_source"] == 2
    same_hits(out, want, "kept")
    out, st = fan(INSIDE, dirs[:64], mirt.QUERY_AUTO)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2
    same_hits(out, want[:64], "auto, cube held")
    # a fan leaves the frame's and DirectLight's statistics alone, and DirectLight's cube
    assert mirt.stats() == stats0 and mirt.query_stats() == qs0
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        again = mirt.direct_light(recs, LIGHTS)
        assert mirt.query_stats()["cube_source"] == 2
        assert np.array_equal(again.view(np.uint32), lit.view(np.uint32))
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
    assert mirt.fan_stats() == st                                           # ... and a DirectLight query the fan's
    out, st = fan(INSIDE, dirs, mirt.QUERY_BINNED)
    assert st["cube_source"] == 2                                           # DirectLight did not evict the fan's cube either
    # another origin
    moved = INSIDE + np.float32(0.125)
    out, st = fan(moved, dirs, mirt.QUERY_BINNED)
    assert st["cube_source"] == 1
    same_hits(out, mirt.intersect(mirt.make_rays(moved, dirs)), "another origin")
    # AUTO without a cube for the origin: from 2000 triangles on it bins whatever the ray count (measured)
    out, st = fan(INSIDE, dirs[:64], mirt.QUERY_AUTO)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 1
    same_hits(out, want[:64], "auto, 2000 triangles")
    # a new scene forgets the cube, and the results follow the new scene
    tris2 = mirt.scene_soup(42, 2000, 0.2)
    mirt.scene_upload(tris2)
    out, st = fan(INSIDE, dirs, mirt.QUERY_BINNED)
    assert st["cube_source"] == 1
    want2 = mirt.intersect(mirt.make_rays(INSIDE, dirs))
    same_hits(out, want2, "new scene")
    assert not np.array_equal(want2["index"], want["index"])
    # an origin outside the filter's range: the frame path would not bin, nor does a fan under BINNED
    far = np.array([3e8, 0, 0], np.float32)
    out, st = fan(far, dirs[:256], mirt.QUERY_BINNED)
    assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0
    rays = mirt.make_rays(far, dirs[:256])
    same_hits(out, mirt.intersect(rays), "origin out of range")
    same_hits(out, oracle_intersect(oracle, tris2, rays), "origin out of range vs oracle")


def test_auto_below_2000_triangles_follows_the_frame_paths_rule(oracle):
    tris = mirt.scene_soup(41, 1000, 0.2)
    mirt.scene_upload(tris)                                   # (a new scene version: no cube is held)
    dirs = directions_from(INSIDE, 1.0, 1024)
    rays = mirt.make_rays(INSIDE, dirs)
    want = mirt.intersect(rays)
    same_hits(want[:256], oracle_intersect(oracle, tris, rays[:256]), "soup1000")
    out, st = fan(INSIDE, dirs, mirt.QUERY_AUTO)               # 1206 x 1000 = 1.2e6: the sweep
    assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0
    same_hits(out, want, "auto, small call")
    big = np.ascontiguousarray(np.concatenate([dirs] * 34))
    assert len(big) * len(tris) >= 40000000 > (len(big) - len(dirs)) * len(tris)
    out, st = fan(INSIDE, big, mirt.QUERY_AUTO)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 1
    same_hits(out, np.concatenate([want] * 34), "auto, large call")
    out, st = fan(INSIDE, dirs[:64], mirt.QUERY_AUTO)          # the cube is held now: the small call uses it
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2
    same_hits(out, want[:64], "auto, small call, cube held")
    out, st = fan(OUTSIDE, dirs[:64], mirt.QUERY_AUTO)         # ... but not for another origin
    assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0


@pytest.mark.parametrize("in_flight", [1, 2, 3, 4])
def test_device_fans_between_binned_frames_in_flight(oracle, in_flight):
    from devbuf import DeviceArray
    tris, b = scene_of("soup2000")
    mirt.scene_upload(tris)
    W, H = 160, 120
    view = mirt.make_view((0, 0, -2.5), oracle.rot_from_yaw(0.1, 1.0), 120.0, W, H)
    light = LIGHTS[:1]
    want_frame = mirt.raytrace(view, light, mode=mirt.RT_BRUTE)["xrgb"]
    origins = [INSIDE, OUTSIDE, INSIDE, INSIDE + np.float32(0.25), OUTSIDE, INSIDE]
    batches = [directions_from(o, b, n, seed=20 + i) for i, (o, n) in enumerate(zip(origins, (1500, 3, 700, 5000, 64, 2049)))]
    want = [mirt.intersect(mirt.make_rays(o, d)) for o, d in zip(origins, batches)]
    bufs = []
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        mirt.set_frames_in_flight(in_flight)
        for o, d in zip(origins, batches):
            d_dirs, d_hits = to_device(d), to_device(mirt.fresh_hits(len(d)))
            x = DeviceArray((H, W), np.uint32, 0)
            bufs.append((d_dirs, d_hits, x))
            mirt.raytrace_device(view, light, (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, x.ptr, W * 4)
            mirt.intersect_from_device(o, d_dirs.ptr, len(d), d_hits.ptr)
        mirt.sync()
        for i, (d_dirs, d_hits, x) in enumerate(bufs):
            same_hits(d_hits.read().view(mirt.HIT_DTYPE).reshape(-1), want[i], "fan %d of %d in flight" % (i, in_flight))
            assert np.array_equal(x.read()[1:-1, 1:-1], want_frame[1:-1, 1:-1]), "frame %d" % i
        # a standing view: every stream holds its pass by now; fans between its frames leave the passes alone
        x = bufs[0][2]
        for i in range(2 * in_flight):
            assert hip_fill(x, 0x11)
            mirt.raytrace_device(view, light, (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, x.ptr, W * 4)
            st = mirt.stats()
            assert st["mode_used"] == mirt.RT_BINNED and st["bins_reused"] == 1, (i, st)
            assert np.array_equal(x.read()[1:-1, 1:-1], want_frame[1:-1, 1:-1]), "standing frame %d" % i
            k = i % len(origins)
            d_hits = bufs[k][1]
            assert hip().hipMemcpy(d_hits.ptr, mirt.fresh_hits(len(batches[k])).ctypes.data_as(C.c_void_p), d_hits.nbytes, 1) == 0
            mirt.intersect_from_device(origins[k], bufs[k][0].ptr, len(batches[k]), d_hits.ptr)
            assert mirt.fan_stats()["mode_used"] == mirt.QUERY_BINNED
            same_hits(d_hits.read().view(mirt.HIT_DTYPE).reshape(-1), want[k], "standing fan %d" % i)
            assert mirt.stats() == st
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
        mirt.set_frames_in_flight(1)
        for t in bufs:
            for d in t:
                d.free()


def hip():
    import devbuf
    return devbuf.hip()


# ---- 7. arguments -----------------------------------------------------------------------------------------------------------------

def test_argument_validation():
    lib = mirt.load()
    dirs, hits = np.ones((4, 3), np.float32), mirt.fresh_hits(4)
    origin = np.zeros(3, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    mirt.scene_upload(mirt.scene_cornell())
    INVALID = -3
    assert lib.mirt_intersect_from(p(origin), None, 4, p(hits)) == INVALID and lib.mirt_intersect_from(p(origin), p(dirs), 4, None) == INVALID
    assert b"direction arrays must not be NULL" in lib.mirt_last_error()
    assert lib.mirt_intersect_from(p(origin), p(dirs), -1, p(hits)) == INVALID
    assert b"direction count -1 is negative" in lib.mirt_last_error()
    assert lib.mirt_intersect_from(None, p(dirs), 4, p(hits)) == INVALID
    assert b"origin must not be NULL" in lib.mirt_last_error()
    assert lib.mirt_intersect_from_device(p(origin), None, 4, None) == INVALID and lib.mirt_intersect_from_device(p(origin), None, -2, None) == INVALID
    assert lib.mirt_intersect_from_device(None, p(dirs), 4, p(hits)) == INVALID
    # n == 0 succeeds and does nothing, NULL arrays included
    assert lib.mirt_intersect_from(p(origin), None, 0, None) == 0 and lib.mirt_intersect_from_device(None, None, 0, None) == 0
    assert hits.tobytes() == mirt.fresh_hits(4).tobytes()
    assert mirt.intersect_from(origin, np.zeros((0, 3), np.float32)).shape == (0,)
    with pytest.raises(ValueError):
        mirt.intersect_from(origin, dirs, mirt.fresh_hits(3))


def test_no_scene():
    mirt.shutdown()
    mirt.init(0)
    with pytest.raises(mirt.MirtError, match="no scene uploaded"):
        mirt.intersect_from((0, 0, 0), np.ones((4, 3), np.float32))
    assert mirt.load().mirt_intersect_from_device(None, None, 0, None) == 0
    st = mirt.fan_stats()
    assert st["mode_used"] == 0 and st["cube_source"] == 0
