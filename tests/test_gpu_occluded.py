"""Occlusion queries on the GPU: mirt_occluded* (k_query_occluded, k_query_occluded_wave) and mirt_occluded_fans*
(k_query_occluded_fans_binned through the many-origin fans' cubes, or the rays written out for the two sweep kernels).

The expected byte of a ray is the reference's own two steps: ClosestIntersection on a fresh record (the CPU oracle,
query_helpers.oracle_intersect), then `distance < limit`, strictly -- expected = (index >= 0) & (distance < limit).  Every output
buffer starts as 0xAA with 64 guard bytes behind it: every byte in range must come back 0 or 1, the guard untouched.  A batch
and its oracle records are computed once per scene and shared by the ray counts, forms and modes compared with them."""
import ctypes as C

import numpy as np
import pytest

import mirt
from devbuf import DeviceArray, hip_fill, to_device
from query_helpers import (FLT_MAX, INF, INSIDE, LIGHTS, NAN, NKINDS, OUTSIDE, expected, fan_scene_of, jitter, limits_for, make_batch, odd_rays,
                           oracle_intersect, scene_of, seam_directions)

pytestmark = pytest.mark.gpu

GUARD = 64
INVALID = -3
NBATCH = 4097 + 300                                  # the lane kernel: a ragged last block, P = 2 with an odd tail
COUNTS = (1, 257, 4096, NBATCH)                      # ... and a wave per ray up to 4096 rays (MIRT_QUERY_WAVE_RAYS)
MODES = (("brute", mirt.QUERY_BRUTE), ("binned", mirt.QUERY_BINNED), ("auto", mirt.QUERY_AUTO))
BOTH = MODES[:2]
_batches, _fans = {}, {}


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_query_mode(mirt.QUERY_AUTO)
    mirt.set_profiling(False)
    mirt.set_frames_in_flight(1)
    mirt.set_soft_shadows(1)
    mirt.set_depth_of_field(0)
    mirt.shutdown()


# ---- expectations, limits, calls -------------------------------------------------------------------------------------------------

def strictness_holds(hits, kind, want):
    """What the limits are there to show, read off the expectation itself: d gives 0, one float more gives 1, one less 0."""
    hit = (hits["index"] >= 0) & np.isfinite(hits["distance"])
    assert not want[kind == 2].any() and not want[kind == 4].any() and not want[kind >= 5].any()
    assert want[hit & (kind == 3)].all() and want[hit & (kind <= 1)].all()
    assert not want[~hit].any()


def checked(buf, n, what):
    """The n bytes of a prefilled buffer after a call: 0 or 1 each, the guard behind them as it was."""
    assert buf.shape == (n + GUARD,) and (buf[n:] == 0xAA).all(), "%s: wrote beyond %d rays" % (what, n)
    assert (buf[:n] <= 1).all(), "%s: %d bytes are neither 0 nor 1" % (what, int((buf[:n] > 1).sum()))
    return buf[:n]


def host_call(rays, limits, n, what):
    buf = np.full(n + GUARD, 0xAA, np.uint8)
    mirt.occluded(rays[:n], None if limits is None else limits[:n], buf[:n])
    return checked(buf, n, what)


def device_call(rays, limits, n, what):
    d_rays, d_lim = to_device(rays[:n]), None if limits is None else to_device(limits[:n])
    with DeviceArray((n + GUARD,), np.uint8, 0xAA) as d_out:
        try:
            mirt.occluded_device(d_rays.ptr, n, None if d_lim is None else d_lim.ptr, d_out.ptr)
            return checked(d_out.read(), n, what)
        finally:
            d_rays.free()
            if d_lim is not None:
                d_lim.free()


def fans_host(origins, of, dirs, limits, mode, what):
    n = len(dirs)
    buf = np.full(n + GUARD, 0xAA, np.uint8)
    mirt.set_query_mode(mode)
    try:
        mirt.occluded_fans(origins, of, dirs, limits, buf[:n])
        return checked(buf, n, what), mirt.occlusion_stats()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


def fans_device(origins, of, dirs, limits, mode, what):
    n = len(dirs)
    d_of, d_dirs, d_lim = to_device(of), to_device(dirs), None if limits is None else to_device(limits)
    with DeviceArray((n + GUARD,), np.uint8, 0xAA) as d_out:
        mirt.set_query_mode(mode)
        try:
            mirt.occluded_fans_device(origins, d_of.ptr, d_dirs.ptr, n, None if d_lim is None else d_lim.ptr, d_out.ptr)
            st = mirt.occlusion_stats()
            return checked(d_out.read(), n, what), st
        finally:
            mirt.set_query_mode(mirt.QUERY_AUTO)
            for d in (d_of, d_dirs) + (() if d_lim is None else (d_lim,)):
                d.free()


# ---- arbitrary rays: the batches ---------------------------------------------------------------------------------------------------

def batch_of(oracle, name):
    """Scene `name` uploaded; its shared batch of NBATCH rays, their oracle records, limits and expectations."""
    tris, a, b = scene_of(name)
    mirt.scene_upload(tris)
    if name not in _batches:
        rays = odd_rays(make_batch(NBATCH, a, b))
        hits = oracle_intersect(oracle, tris, rays)
        limits, kind = limits_for(hits)
        v = rays, hits, limits, kind, expected(hits, limits), expected(hits, None)
        for x in v:
            x.setflags(write=False)
        _batches[name] = v
    return (tris,) + _batches[name]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", ["one", "soup65", "cornell", "soup2000"])
def test_equals_the_reference_decision(oracle, name, n):
    tris, rays, hits, limits, kind, want, want_null = batch_of(oracle, name)
    what = "%s, %d rays" % (name, n)
    if n == NBATCH:
        strictness_holds(hits, kind, want)
        assert name == "one" or (want_null.mean() > 0.05 and want[kind == 3].sum() > 20), "the batch hardly hits anything"
    for form, fname in ((host_call, "host form"), (device_call, "device form")):
        got = form(rays, limits, n, what)
        assert np.array_equal(got, want[:n]), "%s, %s: %d bytes differ (first at ray %d)" % (
            what, fname, int((got != want[:n]).sum()), int(np.flatnonzero(got != want[:n])[0]))
        got = form(rays, None, n, what + ", no limits")
        assert np.array_equal(got, want_null[:n]), "%s, %s, NULL limits: %d bytes differ" % (what, fname, int((got != want_null[:n]).sum()))
    st = mirt.occlusion_stats()
    assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0 and st["cube_bins"] == 0, st


def test_block_exit_across_the_chunk_boundary(oracle):
    """soup2000 is two LDS chunks (1024 + 976 rows).  Workgroups of 512 rays all of which are settled by a row of chunk 0 -- their
    closest hit, at the latest --, which leave at the boundary, beside a workgroup that holds the rays that hit nothing -- four
    waves of them, open to the last row of chunk 1 -- and mixed ones."""
    tris, rays, hits, limits, kind, want, want_null = batch_of(oracle, "soup2000")
    plain = np.ones(len(rays), bool)
    plain[5::41] = False
    early = np.flatnonzero(plain & (hits["index"] >= 0) & (hits["index"] < 1024))
    never = np.flatnonzero(plain & (hits["index"] < 0))
    assert len(early) >= 1024 and len(never) >= 256, (len(early), len(never))
    early = early[:len(early) // 512 * 512]
    rest = np.setdiff1d(np.arange(len(rays)), np.concatenate([early, never]))
    order = np.concatenate([early, never, rest])
    assert len(order) == len(rays) > 4096
    got = device_call(rays[order], None, len(order), "settled blocks first")
    assert np.array_equal(got, want_null[order])
    assert got[:len(early)].all() and not got[len(early):len(early) + len(never)].any()
    got = host_call(rays[order], np.ascontiguousarray(limits[order]), len(order), "settled blocks first, limits")
    assert np.array_equal(got, want[order])


# ---- many origins ------------------------------------------------------------------------------------------------------------------

def fan_origins(K, seed=3):
    """INSIDE, OUTSIDE and the two LIGHTS first, then points of U[-0.8, 0.8]^3."""
    rng = np.random.default_rng(seed)
    first = [INSIDE, OUTSIDE, LIGHTS[0, :3], LIGHTS[1, :3]]
    out = first[:K] + [rng.uniform(-0.8, 0.8, 3) for _ in range(K - len(first))]
    return np.ascontiguousarray(np.array(out, np.float32).reshape(K, 3))


def fan_batch(origins, b, nrays, seed=11):
    """(origin_of, dirs, unformed): the seam directions and their one-ulp neighbours from the first four origins, directions aimed
    at U[-b, b]^3 from origins drawn at random, every 37th of those replaced by one fan_dir_of does not form (zero, a NaN component,
    scaled to 2^-40, scaled to 2^20); the whole batch shuffled, so that waves mix origins, kinds of direction and passes."""
    K = len(origins)
    rng = np.random.default_rng(seed)
    seams = seam_directions()
    ks = min(K, 4)
    extra = nrays - ks * len(seams)
    of = np.concatenate([np.repeat(np.arange(ks), len(seams)), rng.integers(0, K, extra)]).astype(np.int32)
    target = rng.uniform(-b, b, (extra, 3)).astype(np.float32)
    aimed = (target - origins[of[ks * len(seams):]]).astype(np.float32)
    unformed = np.zeros(nrays, bool)
    for k, i in enumerate(range(3, extra, 37)):
        unit = aimed[i] / np.abs(aimed[i]).max()
        kind = k % 4
        if kind == 0:
            aimed[i] = 0
        elif kind == 1:
            aimed[i][k % 3] = NAN
        elif kind == 2:
            aimed[i] = unit * np.float32(2.0 ** -40)
        else:
            aimed[i] = unit * np.float32(2.0 ** 20)
        unformed[ks * len(seams) + i] = True
    dirs = np.concatenate([np.tile(seams, (ks, 1)), aimed]).astype(np.float32)
    order = rng.permutation(nrays)
    return np.ascontiguousarray(of[order]), np.ascontiguousarray(dirs[order]), unformed[order]


def fans_of(oracle, name, K, nrays=4500):
    """Scene `name` uploaded; the shared batch of K origins on it with its oracle records, limits and expectations."""
    tris, b = fan_scene_of(name)
    mirt.scene_upload(tris)
    if (name, K) not in _fans:
        origins = fan_origins(K)
        of, dirs, unformed = fan_batch(origins, b, nrays)
        hits = oracle_intersect(oracle, tris, mirt.make_rays(origins[of], dirs))
        limits, kind = limits_for(hits)
        v = origins, of, dirs, unformed, hits, limits, kind, expected(hits, limits), expected(hits, None)
        for x in v:
            x.setflags(write=False)
        _fans[name, K] = v
    return (tris,) + _fans[name, K]


@pytest.mark.parametrize("name,K", [("cornell", 4), ("soup2000", 4), ("cornell x 2", 33)])
def test_fans_equal_the_reference_decision(oracle, name, K):
    tris, origins, of, dirs, unformed, hits, limits, kind, want, want_null = fans_of(oracle, name, K)
    assert len(dirs) <= 5000 and len(np.unique(of)) == K and unformed.sum() > 50
    strictness_holds(hits, kind, want)
    assert want_null.mean() > 0.05 and want_null[unformed].any(), "the batch hardly hits anything"
    for mname, mode in MODES:
        what = "%s, %d origins, %s" % (name, K, mname)
        for form in (fans_host, fans_device):
            got, st = form(origins, of, dirs, limits, mode, what)
            assert np.array_equal(got, want), "%s: %d bytes differ (first at ray %d)" % (what, int((got != want).sum()), int(np.flatnonzero(got != want)[0]))
            got, st = form(origins, of, dirs, None, mode, what + ", no limits")
            assert np.array_equal(got, want_null), "%s, NULL limits: %d bytes differ" % (what, int((got != want_null).sum()))
            if mode == mirt.QUERY_BRUTE:
                assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0 and st["cube_bins"] == 0, st
            elif mode == mirt.QUERY_BINNED:
                assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] in (1, 2) and st["shells"] >= 1, st
    # the same answers from mirt_occluded on the rays written out
    rays = mirt.make_rays(origins[of], dirs)
    assert np.array_equal(host_call(rays, limits, len(rays), "expanded"), want)


def test_fans_equal_occluded_on_a_large_batch():
    """65 536 rays from four origins on cornell + soup2000, GPU against GPU: the bytes of mirt_occluded on the expanded rays, which
    in turn are the reference's decision on the library's own (bit-exact) closest hits."""
    tris, b = fan_scene_of("cornell+soup2000")
    mirt.scene_upload(tris)
    origins = fan_origins(4)
    of, dirs, unformed = fan_batch(origins, b, 65536, seed=17)
    rays = mirt.make_rays(origins[of], dirs)
    hits = mirt.intersect(rays)
    limits, kind = limits_for(hits)
    want = host_call(rays, limits, len(rays), "expanded")
    assert np.array_equal(want, expected(hits, limits))
    strictness_holds(hits, kind, want)
    want_null = host_call(rays, None, len(rays), "expanded, no limits")
    assert np.array_equal(want_null, expected(hits, None)) and 0.05 < want_null.mean() < 0.999
    for mname, mode in MODES:
        got, st = fans_device(origins, of, dirs, limits, mode, mname)
        assert got.tobytes() == want.tobytes(), "%s: %d bytes differ" % (mname, int((got != want).sum()))
        got, st = fans_host(origins, of, dirs, None, mode, mname + ", no limits")
        assert got.tobytes() == want_null.tobytes(), "%s, NULL limits: %d bytes differ" % (mname, int((got != want_null).sum()))
        assert st["mode_used"] == (mirt.QUERY_BRUTE if mode == mirt.QUERY_BRUTE else mirt.QUERY_BINNED), (mname, st)


@pytest.mark.parametrize("name,K", [("soup2000", 4), ("cornell x 2", 33)])
def test_indices_outside_the_list(oracle, name, K):
    tris, origins, of, dirs, unformed, hits, limits, kind, want, want_null = fans_of(oracle, name, K)
    bad_of = of.copy()
    bad = np.concatenate([w + np.array([1, 30, 63]) for w in range(0, len(of) - 64, 64)])     # three in every wave
    bad_of[bad[0::3]] = -1
    bad_of[bad[1::3]] = K
    bad_of[bad[2::3]] = 2 ** 30
    bad_of[bad[0]] = -2 ** 31
    stray_want = want_null.copy()
    stray_want[bad] = 0
    assert want_null[bad].sum() > 20
    for mname, mode in BOTH:
        got, st = fans_device(origins, bad_of, dirs, None, mode, mname)
        assert st["mode_used"] == mode
        assert not got[bad].any(), "%s: a ray with an index outside the list is not 0" % mname
        assert np.array_equal(got, stray_want), "%s: the rays around them" % mname
    # the host form looks first and writes nothing
    lib = mirt.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for i in bad[:4]:
        one = of.copy()
        one[i] = bad_of[i]
        out = np.full(len(dirs) + GUARD, 0xAA, np.uint8)
        assert lib.mirt_occluded_fans(p(origins), K, p(one), p(dirs), len(dirs), None, p(out)) == INVALID
        assert b"origin_of[%d]" % i in lib.mirt_last_error()
        assert (out == 0xAA).all()


# ---- statistics and caches ---------------------------------------------------------------------------------------------------------

def test_stats(oracle):
    tris, origins, of, dirs, unformed, hits, limits, kind, want, want_null = fans_of(oracle, "soup2000", 4)
    mirt.scene_upload(tris)                                                 # (a new scene version: nothing is held)
    view = mirt.make_view((0, 0, -2.5), oracle.rot_from_yaw(0.1, 1.0), 60.0, 32, 24)
    mirt.raytrace(view, LIGHTS[:1])
    frame, light, fan = mirt.stats(), mirt.query_stats(), mirt.fan_stats()
    mirt.set_profiling(True)
    try:
        got, st = fans_host(origins, of, dirs, None, mirt.QUERY_BINNED, "profiled")
        assert np.array_equal(got, want_null)
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 1 and st["cube_bins"] in (64, 128, 256) and st["shells"] >= 1, st
        assert st["shadow_rays"] == len(dirs) and st["fallback_records"] == int(unformed.sum()), (st, int(unformed.sum()))
        assert 0 < st["tests"] <= st["candidates"], st
        assert mirt.fan_stats() == fan and mirt.query_stats() == light
        got, st2 = fans_device(origins, of, dirs, None, mirt.QUERY_BINNED, "profiled, kept cube")
        assert st2["cube_source"] == 2 and np.array_equal(got, want_null), st2
        # the closest-hit call on the same rays reads the same cube, and steps over no fewer rows: a ray's first accepted row lies
        # no later than the end of its closest hit's shell
        mirt.set_query_mode(mirt.QUERY_BINNED)
        closest = mirt.intersect_fans(origins, of, dirs)
        fs = mirt.fan_stats()
        assert closest.tobytes() == hits.tobytes()
        assert fs["mode_used"] == mirt.QUERY_BINNED and fs["cube_source"] == 2 and fs["cube_bins"] == st["cube_bins"], fs
        assert st["candidates"] <= fs["candidates"] and st2["candidates"] == st["candidates"], (st, st2, fs)
        assert mirt.occlusion_stats() == st2                                # ... and the fans' call leaves these alone
        # limits: nothing to walk for a limit nothing is below, and never more than without limits
        got, st3 = fans_host(origins, of, dirs, limits, mirt.QUERY_BINNED, "profiled, limits")
        assert np.array_equal(got, want) and st3["shadow_rays"] == len(dirs) and st3["tests"] <= st3["candidates"], st3
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
        mirt.set_profiling(False)
    # without profiling the counters stay zero; the brute path reports no cube; mirt_occluded* reports brute force
    _, st = fans_host(origins, of, dirs, None, mirt.QUERY_BINNED, "plain")
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2 and st["shadow_rays"] == st["candidates"] == st["tests"] == 0, st
    _, st = fans_host(origins, of, dirs, None, mirt.QUERY_BRUTE, "brute")
    assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0 and st["cube_bins"] == 0, st
    _, st = fans_host(origins, of[:64], dirs[:64], None, mirt.QUERY_AUTO, "auto, cube held")
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2, st
    host_call(mirt.make_rays(origins[of], dirs), None, 300, "arbitrary rays")
    st = mirt.occlusion_stats()
    assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0, st
    # no occlusion call touched the statistics of the last frame, the last DirectLight query or the last fan
    assert mirt.stats() == frame and mirt.query_stats() == light
    assert mirt.fan_stats() == fs
    assert mirt.load().mirt_get_occlusion_stats(None) == INVALID


def test_fallback_sweep_counters(oracle):
    """The whole-table sweep of the lanes the bins do not cover counts every row a live lane tests, into `candidates` and `tests`
    alike.  70 rays (more than one wave) from two origins off every triangle of the 65-triangle soup, all along (2^20, 0, 0):
    finite, outside the fan window (fan_dir_of forms nothing) and above the filter's direction range (every test takes the exact
    path).  With a limit of 1e-30 no accepted distance is below it, so every ray stays open over all 65 rows."""
    tris, _, _ = scene_of("soup65")
    mirt.scene_upload(tris)
    n, nrays = len(tris), 70
    assert n == 65
    origins = fan_origins(2)
    of = np.ascontiguousarray((np.arange(nrays) % 2).astype(np.int32))
    dirs = np.ascontiguousarray(np.tile(np.array([2.0 ** 20, 0, 0], np.float32), (nrays, 1)))
    limits = np.full(nrays, 1e-30, np.float32)
    want = expected(oracle_intersect(oracle, tris, mirt.make_rays(origins[of], dirs)), limits)
    mirt.set_profiling(True)
    try:
        got, st = fans_host(origins, of, dirs, limits, mirt.QUERY_BINNED, "unformed directions")
    finally:
        mirt.set_profiling(False)
    print(st)
    assert not got.any() and np.array_equal(got, want)
    assert st["mode_used"] == mirt.QUERY_BINNED, st
    assert st["shadow_rays"] == nrays and st["fallback_records"] == nrays, st
    assert st["candidates"] == st["tests"] == nrays * n, st


def test_a_repeated_call_of_two_passes_builds_nothing(oracle):
    """33 origins are two passes, each with a cube of its own (tests/fuzz_queries.py seed 2015, shrunk to: upload, set_query_mode
    BINNED, occluded_fans with 33 origins twice -- when one cube served every pass, the second call built both again): the
    repeated call, either form, and mirt_intersect_fans on the same origins find both held."""
    tris, origins, of, dirs, unformed, hits, limits, kind, want, want_null = fans_of(oracle, "cornell x 2", 33)
    mirt.scene_upload(tris)                                                 # (a new scene version: nothing is held)
    got, st = fans_host(origins, of, dirs, limits, mirt.QUERY_BINNED, "first call")
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 1 and np.array_equal(got, want), st
    for form in (fans_host, fans_device):
        got, st = form(origins, of, dirs, limits, mirt.QUERY_BINNED, "repeated call")
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2 and np.array_equal(got, want), st
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        closest = mirt.intersect_fans(origins, of, dirs)
        assert mirt.fan_stats()["cube_source"] == 2 and closest.tobytes() == hits.tobytes()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


def test_cube_shared_with_the_fans_and_the_frame_path(oracle):
    tris, origins, of, dirs, unformed, hits, limits, kind, want, want_null = fans_of(oracle, "soup2000", 4)
    # a fresh library state: mirt_intersect_fans builds the cube, the occlusion call finds it held -- under AUTO with few rays too
    mirt.shutdown()
    mirt.init(0)
    mirt.scene_upload(tris)
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        closest = mirt.intersect_fans(origins, of, dirs)
        assert mirt.fan_stats()["cube_source"] == 1 and closest.tobytes() == hits.tobytes()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
    got, st = fans_host(origins, of[:100], dirs[:100], limits[:100], mirt.QUERY_AUTO, "held by the fans")
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2, st
    assert np.array_equal(got, want[:100])
    # ... and the reverse
    mirt.scene_upload(tris)
    got, st = fans_host(origins, of, dirs, limits, mirt.QUERY_BINNED, "built here")
    assert st["cube_source"] == 1 and np.array_equal(got, want), st
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        closest = mirt.intersect_fans(origins, of, dirs)
        assert mirt.fan_stats()["cube_source"] == 2 and closest.tobytes() == hits.tobytes()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
    # the frame path's cube: binned frames under standing lights settle into the shared cube; rays from those lights read it
    W, H = 160, 120
    view = mirt.make_view((0, 0, -2.5), oracle.rot_from_yaw(0.1, 1.0), 120.0, W, H)
    with DeviceArray((H, W), np.uint32, 0) as x:
        for i in range(7):
            mirt.raytrace_device(view, LIGHTS[:2], (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, x.ptr, W * 4)
            mirt.sync()
    frame = mirt.stats()
    lpos = np.ascontiguousarray(LIGHTS[:2, :3])
    from_lights = of >= 2                                                   # origins 2 and 3 of the batch ARE the lights
    assert np.array_equal(origins[2:4], lpos)
    lof = np.ascontiguousarray((of[from_lights] - 2).astype(np.int32))
    got, st = fans_host(lpos, lof, np.ascontiguousarray(dirs[from_lights]), np.ascontiguousarray(limits[from_lights]), mirt.QUERY_BINNED,
                        "the frame path's cube")
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 3, st
    assert np.array_equal(got, want[from_lights])
    assert mirt.stats() == frame


# ---- state --------------------------------------------------------------------------------------------------------------------------

def test_results_follow_the_scene(oracle):
    tris, origins, of, dirs, unformed, hits, limits, kind, want, want_null = fans_of(oracle, "soup2000", 4)
    rays = mirt.make_rays(origins[of], dirs)
    lim = np.full(len(rays), 1.5, np.float32)
    before = expected(hits, lim)
    assert np.array_equal(host_call(rays, lim, len(rays), "before"), before)
    got, st = fans_host(origins, of, dirs, lim, mirt.QUERY_BINNED, "before, binned")
    assert np.array_equal(got, before)
    eye = np.eye(3, dtype=np.float32).ravel()
    mirt.scene_transform(0, len(tris), eye, (0.0625, 0.0, 0.0))
    after = expected(mirt.intersect(rays), lim)                             # (the library's closest hits on the moved scene,
    first = np.arange(300)                                                  # themselves checked against the oracle on the first 300)
    assert np.array_equal(after[first], expected(oracle_intersect(oracle, mirt.scene_download(), rays[first]), lim[first]))
    assert not np.array_equal(after, before)
    assert np.array_equal(host_call(rays, lim, len(rays), "after"), after)
    got, st = fans_host(origins, of, dirs, lim, mirt.QUERY_BINNED, "after, binned")
    assert st["cube_source"] == 1 and np.array_equal(got, after), st
    mirt.scene_upload(tris)


def test_two_frames_in_flight(oracle):
    tris, rays, hits, limits, kind, want, want_null = batch_of(oracle, "soup2000")
    _, origins, of, dirs, unformed, fhits, flimits, fkind, fwant, fwant_null = fans_of(oracle, "soup2000", 4)
    mirt.scene_upload(tris)
    n, m = len(rays), len(dirs)
    d_rays, d_lim, d_of, d_dirs, d_flim = to_device(rays), to_device(limits), to_device(of), to_device(dirs), to_device(flimits)
    outs = [DeviceArray((k + GUARD,), np.uint8, 0xAA) for k in (n, n, m, m)]
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        mirt.set_frames_in_flight(2)
        mirt.occluded_device(d_rays.ptr, n, d_lim.ptr, outs[0].ptr)
        mirt.occluded_device(d_rays.ptr, n, None, outs[1].ptr)
        mirt.occluded_fans_device(origins, d_of.ptr, d_dirs.ptr, m, d_flim.ptr, outs[2].ptr)
        mirt.occluded_fans_device(origins, d_of.ptr, d_dirs.ptr, m, None, outs[3].ptr)
        mirt.sync()
        for i, (o, k, w) in enumerate(zip(outs, (n, n, m, m), (want, want_null, fwant, fwant_null))):
            assert np.array_equal(checked(o.read(), k, "call %d" % i), w), "call %d of four on two streams" % i
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
        mirt.set_frames_in_flight(1)
        for d in [d_rays, d_lim, d_of, d_dirs, d_flim] + outs:
            d.free()


def test_render_settings_do_not_matter(oracle):
    tris, rays, hits, limits, kind, want, want_null = batch_of(oracle, "cornell")
    _, origins, of, dirs, unformed, fhits, flimits, fkind, fwant, fwant_null = fans_of(oracle, "cornell", 4)
    mirt.set_soft_shadows(4, jitter(oracle, LIGHTS[:1], 4))
    mirt.set_depth_of_field(8, 1.3)
    try:
        assert np.array_equal(host_call(rays, limits, len(rays), "soft shadows, depth of field"), want)
        for mname, mode in BOTH:
            got, _ = fans_host(origins, of, dirs, flimits, mode, mname)
            assert np.array_equal(got, fwant), mname
    finally:
        mirt.set_soft_shadows(1)
        mirt.set_depth_of_field(0)


# ---- the reference's own use: DirectLight's shadow rays -------------------------------------------------------------------------------

def test_shadow_rays_of_a_primary_frame(oracle):
    """raytracer.cpp:306-315 with the caller's arithmetic: start = the light, dir = record - light, limit = 0.99f * |dir| in
    float32.  (The hand-built dir is not bit for bit the reference's normalised rDir, so the colours of direct_light are no
    yardstick here: the oracle's decision on these very rays is.)"""
    tris = mirt.scene_cornell()
    mirt.scene_upload(tris)
    light = LIGHTS[0, :3]
    view = mirt.make_view((0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 16.0, 32, 32)
    frame = mirt.raytrace(view, LIGHTS[:1], want_intersection=True)
    on = frame["index"].reshape(-1) >= 0
    pos = np.ascontiguousarray(frame["pos"].reshape(-1, 3)[on], np.float32)
    assert len(pos) > 900
    dirs = (pos - light).astype(np.float32)
    length = np.sqrt((dirs[:, 0] * dirs[:, 0] + dirs[:, 1] * dirs[:, 1] + dirs[:, 2] * dirs[:, 2]).astype(np.float32)).astype(np.float32)
    limits = np.ascontiguousarray((np.float32(0.99) * length).astype(np.float32))
    rays = mirt.make_rays(light, dirs)
    want = expected(oracle_intersect(oracle, tris, rays), limits)
    assert 20 <= want.sum() < 0.9 * len(want), want.sum()                   # some records lie in shadow, most do not
    assert np.array_equal(host_call(rays, limits, len(rays), "shadow rays"), want)
    assert np.array_equal(device_call(rays, limits, len(rays), "shadow rays, device form"), want)
    for mname, mode in MODES:
        got, _ = fans_host(light.reshape(1, 3), None, dirs, limits, mode, mname)
        assert np.array_equal(got, want), mname


# ---- arguments ------------------------------------------------------------------------------------------------------------------------

def test_argument_validation():
    lib = mirt.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    mirt.scene_upload(mirt.scene_cornell())
    rays = mirt.make_rays(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32))
    limits = np.ones(4, np.float32)
    origins = np.zeros((2, 3), np.float32)
    of = np.array([0, 1, 1, 0], np.int32)
    dirs = np.ones((4, 3), np.float32)
    out = np.full(4 + GUARD, 0xAA, np.uint8)
    # (the device forms are given host pointers here: every one of these calls returns before anything touches the device)
    for f in (lib.mirt_occluded, lib.mirt_occluded_device):
        assert f(p(rays), -1, p(limits), p(out)) == INVALID and b"ray count -1 is negative" in lib.mirt_last_error()
        assert f(None, 4, p(limits), p(out)) == INVALID and f(p(rays), 4, p(limits), None) == INVALID
        assert b"ray arrays must not be NULL" in lib.mirt_last_error()
        assert f(None, 0, None, None) == 0 and f(p(rays), 0, p(limits), p(out)) == 0
    for f in (lib.mirt_occluded_fans, lib.mirt_occluded_fans_device):
        assert f(p(origins), -1, p(of), p(dirs), 4, p(limits), p(out)) == INVALID and b"origin count -1 is negative" in lib.mirt_last_error()
        assert f(p(origins), 2, p(of), p(dirs), -1, p(limits), p(out)) == INVALID and b"direction count -1 is negative" in lib.mirt_last_error()
        assert f(p(origins), 2, p(of), None, 4, p(limits), p(out)) == INVALID and f(p(origins), 2, p(of), p(dirs), 4, p(limits), None) == INVALID
        assert b"direction arrays must not be NULL" in lib.mirt_last_error()
        assert f(None, 2, p(of), p(dirs), 4, p(limits), p(out)) == INVALID and b"origins must not be NULL" in lib.mirt_last_error()
        assert f(p(origins), 0, p(of), p(dirs), 4, p(limits), p(out)) == INVALID and b"no origin" in lib.mirt_last_error()
        assert f(p(origins), 2, None, p(dirs), 4, p(limits), p(out)) == INVALID
        assert b"origin_of may be NULL only for a single origin" in lib.mirt_last_error()
        assert f(p(origins), 2, p(of), None, 0, None, None) == 0 and f(None, 0, None, None, 0, None, None) == 0
    assert (out == 0xAA).all()
    assert mirt.occluded(rays[:0]).shape == (0,) and mirt.occluded_fans(origins, np.zeros(0, np.int32), np.zeros((0, 3), np.float32)).shape == (0,)


def test_no_scene():
    mirt.shutdown()
    mirt.init(0)
    rays = mirt.make_rays(np.zeros((2, 3), np.float32), np.ones((2, 3), np.float32))
    with pytest.raises(mirt.MirtError, match="no scene uploaded"):
        mirt.occluded(rays)
    with pytest.raises(mirt.MirtError, match="no scene uploaded"):
        mirt.occluded_fans(np.zeros((2, 3), np.float32), np.array([0, 1], np.int32), np.ones((2, 3), np.float32))
    st = mirt.occlusion_stats()
    assert st["mode_used"] == 0 and st["cube_source"] == 0
