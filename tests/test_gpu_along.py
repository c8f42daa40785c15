"""Ray queries along one direction on the GPU: mirt_intersect_along* (k_along_closest) and mirt_occluded_along* (k_along_occluded)
through the grid across the direction, and by brute force over the rays written out.

Expected records are the CPU oracle's ClosestIntersection per ray on the rays {origins[i], dir} (query_helpers.oracle_intersect),
compared bit for bit (same_hits); expected bytes are the reference's two steps on fresh-record results (query_helpers.expected).
Occlusion buffers start as 0xAA with 64 guard bytes behind them.  A scene's batch and its oracle records are computed once and
shared by the ray counts, forms and modes compared with them."""
import ctypes as C

import numpy as np
import pytest

import mirt
import silhouette
from along_helpers import OBLIQUE, SHELLS, cell_of, directions, grid_of, plant_odd_starts, silhouette_starts
from devbuf import DeviceArray, to_device
from query_helpers import FLT_MAX, INF, LIGHTS, NAN, expected, limits_for, make_batch, oracle_intersect, same_hits, scene_of

pytestmark = pytest.mark.gpu

GUARD = 64
INVALID = -3
NBATCH = 4097 + 300
COUNTS = (1, 257, 4096, NBATCH)
MODES = (("brute", mirt.QUERY_BRUTE), ("binned", mirt.QUERY_BINNED), ("auto", mirt.QUERY_AUTO))
BOTH = MODES[:2]
_batches, _sweeps = {}, {}


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_query_mode(mirt.QUERY_AUTO)
    mirt.set_profiling(False)
    mirt.set_frames_in_flight(1)
    mirt.shutdown()


# ---- calls ---------------------------------------------------------------------------------------------------------------------------

def checked(buf, n, what):
    assert buf.shape == (n + GUARD,) and (buf[n:] == 0xAA).all(), "%s: wrote beyond %d rays" % (what, n)
    assert (buf[:n] <= 1).all(), "%s: %d bytes are neither 0 nor 1" % (what, int((buf[:n] > 1).sum()))
    return buf[:n]


def closest(form, d, starts, mode, hits=None):
    """(records, statistics) of one closest-hit call in `mode`; form: "host" or "device"."""
    n = len(starts)
    mirt.set_query_mode(mode)
    try:
        if form == "host":
            return mirt.intersect_along(d, starts, hits), mirt.along_stats()
        incoming = mirt.fresh_hits(n) if hits is None else hits
        d_starts, d_hits = to_device(starts), to_device(np.concatenate([incoming, mirt.fresh_hits(4)]))     # (four records of guard)
        try:
            mirt.intersect_along_device(d, d_starts.ptr, n, d_hits.ptr)
            st = mirt.along_stats()
            mirt.sync()
            back = np.frombuffer(d_hits.read().tobytes(), mirt.HIT_DTYPE)
            assert back[n:].tobytes() == mirt.fresh_hits(4).tobytes(), "wrote beyond %d records" % n
            return back[:n].copy(), st
        finally:
            d_starts.free(); d_hits.free()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


def occluded(form, d, starts, limits, mode, what=""):
    n = len(starts)
    mirt.set_query_mode(mode)
    try:
        if form == "host":
            buf = np.full(n + GUARD, 0xAA, np.uint8)
            mirt.occluded_along(d, starts, limits, buf[:n])
            return checked(buf, n, what), mirt.along_stats()
        d_starts, d_lim = to_device(starts), None if limits is None else to_device(limits)
        with DeviceArray((n + GUARD,), np.uint8, 0xAA) as d_out:
            try:
                mirt.occluded_along_device(d, d_starts.ptr, n, None if d_lim is None else d_lim.ptr, d_out.ptr)
                st = mirt.along_stats()
                return checked(d_out.read(), n, what), st
            finally:
                d_starts.free()
                if d_lim is not None:
                    d_lim.free()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


def mode_is(st, mode, what):
    if mode == mirt.QUERY_BRUTE:
        assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0 and st["cube_bins"] == 0, (what, st)
    elif mode == mirt.QUERY_BINNED:
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] in (1, 2) and st["cube_bins"] >= 8 and st["shells"] == SHELLS, (what, st)


def extent_of(tris):
    return float(np.abs(np.asarray(tris).reshape(-1, 15)[:, :9]).max())


# ---- scenes, ray counts, modes, forms ----------------------------------------------------------------------------------------------

def batch_of(oracle, name):
    """Scene `name` uploaded; NBATCH of make_batch's starts with the odd kinds planted, along OBLIQUE: the oracle's fresh-record
    results, limits of the eight kinds and both expectations."""
    tris, a, b = scene_of(name)
    mirt.scene_upload(tris)
    if name not in _batches:
        starts, planted = plant_odd_starts(make_batch(NBATCH, a, b)["start"], extent_of(tris))
        hits = oracle_intersect(oracle, tris, mirt.make_rays(starts, OBLIQUE))
        limits, kind = limits_for(hits)
        v = starts, planted, hits, limits, kind, expected(hits, limits), expected(hits, None)
        for x in v:
            x.setflags(write=False)
        _batches[name] = v
    return (tris,) + _batches[name]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", ["one", "soup65", "cornell", "soup2000"])
def test_equals_the_reference(oracle, name, n):
    tris, starts, planted, hits, limits, kind, want, want_null = batch_of(oracle, name)
    if n == NBATCH and name != "one":
        assert (hits["index"] >= 0).mean() > 0.05 and want[kind == 3].sum() > 10, "the batch hardly hits anything"
    for mname, mode in MODES:
        for form in ("host", "device"):
            what = "%s, %d rays, %s, %s form" % (name, n, mname, form)
            got, st = closest(form, OBLIQUE, starts[:n], mode)
            mode_is(st, mode, what)
            same_hits(got, hits[:n], what)
            got, st = occluded(form, OBLIQUE, starts[:n], limits[:n], mode, what)
            mode_is(st, mode, what)
            assert np.array_equal(got, want[:n]), "%s: %d bytes differ (first at ray %d)" % (what, int((got != want[:n]).sum()), int(np.flatnonzero(got != want[:n])[0]))
            got, st = occluded(form, OBLIQUE, starts[:n], None, mode, what + ", no limits")
            assert np.array_equal(got, want_null[:n]), "%s, NULL limits: %d bytes differ" % (what, int((got != want_null[:n]).sum()))


# ---- directions -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell", "soup2000"])
def test_directions(oracle, name):
    """The 26 axis, diagonal and corner directions, the oblique one and the two ends of the magnitude window, 257 starts each."""
    tris, a, b = scene_of(name)
    mirt.scene_upload(tris)
    starts, _ = plant_odd_starts(make_batch(257, a, b, seed=19)["start"], extent_of(tris))
    for k, d in enumerate(directions()):
        if (name, k) not in _sweeps:
            _sweeps[name, k] = oracle_intersect(oracle, tris, mirt.make_rays(starts, d))
        hits = _sweeps[name, k]
        limits, kind = limits_for(hits)
        for mname, mode in BOTH:
            what = "%s, direction %r, %s" % (name, d.tolist(), mname)
            got, st = closest("device", d, starts, mode)
            assert st["mode_used"] in (mirt.QUERY_BRUTE, mode), (what, st)      # (an edge-on scene may give the grid up)
            same_hits(got, hits, what)
            got, st = occluded("device", d, starts, limits, mode, what)
            assert np.array_equal(got, expected(hits, limits)), what


def test_a_direction_outside_the_window_is_brute_force(oracle):
    tris, starts, planted, hits, limits, kind, want, want_null = batch_of(oracle, "soup65")
    for d in (np.array([0, 0, 2.0 ** 20], np.float32), np.array([2.0 ** -40, 0, 0], np.float32), np.array([0, 0, 0], np.float32), np.array([1, NAN, 0], np.float32)):
        ref = oracle_intersect(oracle, tris, mirt.make_rays(starts[:300], d))
        got, st = closest("device", d, starts[:300], mirt.QUERY_BINNED)
        assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0, (d, st)
        same_hits(got, ref, repr(d))


# ---- incoming records -----------------------------------------------------------------------------------------------------------------

def test_incoming_records(oracle):
    """The records an earlier ray left (another direction's results), and records with negative, NaN and +inf distances."""
    tris, starts, planted, hits, limits, kind, want, want_null = batch_of(oracle, "soup2000")
    n = 1200
    other = np.array([-1, 0.25, 0.5], np.float32)
    left = oracle_intersect(oracle, tris, mirt.make_rays(starts[:n], other))
    odd = left.copy()
    odd["distance"][0::7] = -1.0
    odd["distance"][1::7] = NAN
    odd["distance"][2::7] = INF
    odd["distance"][3::7] = 0.0
    odd["distance"][4::7] = hits["distance"][:n][4::7]                       # a tie with the ray's own closest hit: the record loses it
    odd["index"][4::7] = 12345
    for incoming, iname in ((left, "left by an earlier ray"), (odd, "odd distances")):
        ref = oracle_intersect(oracle, tris, mirt.make_rays(starts[:n], OBLIQUE), incoming)
        for mname, mode in BOTH:
            for form in ("host", "device"):
                got, st = closest(form, OBLIQUE, starts[:n], mode, incoming.copy())
                mode_is(st, mode, iname)
                same_hits(got, ref, "%s, %s, %s form" % (iname, mname, form))
    kept = (odd["distance"] < 0) | np.isnan(odd["distance"])
    assert ref[kept].tobytes() == odd[kept].tobytes() and (ref["index"][2::7] >= 0).sum() > 20


# ---- an edge-on scene -----------------------------------------------------------------------------------------------------------------

def edge_on_scene(d):
    """Cornell's box and eight soup triangles turned to within 2^-22 rad of edge-on to d."""
    rng = np.random.default_rng(23)
    dh = np.asarray(d, np.float64) / np.linalg.norm(d)
    v = []
    for k in range(8):
        e1 = rng.uniform(-0.3, 0.3, 3)
        nperp = np.cross(e1, dh)
        nperp /= np.linalg.norm(nperp)
        theta = 2.0 ** -22 * (1, -1, 0.5, -0.25, 0, 1, -1, 0.125)[k]
        e2 = rng.uniform(-0.5, 0.5) * e1 + 0.25 * dh + theta * 0.25 * nperp
        v0 = rng.uniform(-0.5, 0.5, 3)
        v.append([v0, v0 + e1, v0 + e2])
    return np.concatenate([mirt.scene_cornell(), silhouette.finish(v)])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_edge_on_scene(oracle, axis):
    """dir in the planes of Cornell's walls, exactly and tilted by one ulp either way: BINNED equals BRUTE equals the oracle."""
    base = np.zeros(3, np.float32)
    base[axis] = -1.0
    tilted = []
    for c in ((axis + 1) % 3, (axis + 2) % 3):
        for to in (INF, -INF):
            e = base.copy()
            e[c] = np.nextafter(np.float32(0), to)
            tilted.append(e)
    up = base.copy()
    up[axis] = np.nextafter(np.float32(-1), np.float32(0))
    rng = np.random.default_rng(29)
    for d in [base] + tilted + [up]:
        tris = edge_on_scene(d)
        mirt.scene_upload(tris)
        # starts all over the box, and starts IN the planes of the walls (coordinates +-1 exactly) and of the edge-on triangles
        starts = rng.uniform(-0.99, 0.99, (320, 3)).astype(np.float32)
        for k in range(0, 160):
            starts[k][(axis + 1 + k % 2) % 3] = (1.0, -1.0)[(k // 2) % 2]
        on_tri = tris[-8:, 0:3] + 0.3 * (tris[-8:, 3:6] - tris[-8:, 0:3]) + 0.2 * (tris[-8:, 6:9] - tris[-8:, 0:3])
        starts[160:168] = on_tri - 0.4 * d / np.float32(np.abs(d).max())
        ref = oracle_intersect(oracle, tris, mirt.make_rays(starts, d))
        brute, st = closest("device", d, starts, mirt.QUERY_BRUTE)
        binned, st = closest("device", d, starts, mirt.QUERY_BINNED)
        assert st["mode_used"] == mirt.QUERY_BINNED, st                    # (38 triangles: the every-ray list never outgrows its floor of 64)
        same_hits(brute, ref, "brute, %r" % d.tolist())
        same_hits(binned, ref, "binned, %r" % d.tolist())
        limits, _ = limits_for(ref)
        for mode in (mirt.QUERY_BRUTE, mirt.QUERY_BINNED):
            got, _ = occluded("device", d, starts, limits, mode)
            assert np.array_equal(got, expected(ref, limits)), (d, mode)


# ---- silhouette probes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,targets,d", [("soup2000", range(24), OBLIQUE), ("needles", range(0, 150, 6), np.array([-0.6, 1.0, 0.35], np.float32)),
                                            ("walls", range(24), np.array([0.2, 0.3, -1.0], np.float32)),
                                            ("soup2000 @ far", range(24), OBLIQUE), ("needles @ far", range(0, 150, 6), np.array([-0.6, 1.0, 0.35], np.float32))])
def test_silhouette_probes(oracle, name, targets, d):
    """Starts within 2^-20 .. 2^-8 of projected edges, vertices and the grid's cell borders, twins to either side.  The "@ far"
    scenes lie at (300, 200, -100), where a start's ulp is about 2^-15 of the scene: the smallest delta is below what a start
    resolves there, the larger two are not.  The soup's grid holds there (50 of 2000 triangles on the every-ray list); of the
    needles 149 of 150 go on it -- their margins, sized by |S| and |v0|, are wider than they are --, the grid gives up and BINNED
    runs the brute-force kernels (tests/test_along_host.py has both counts from the header)."""
    tris = silhouette.scene_of(oracle, name)[0]
    mirt.scene_upload(tris)
    info = mirt.scene_info()
    grid = grid_of(d, info["bbox_lo"], info["bbox_hi"], len(tris))
    starts = silhouette_starts(tris, d, targets, grid)
    assert 500 < len(starts) < 9000, len(starts)
    i, j = cell_of(grid, starts)
    assert (i >= 0).mean() > 0.9 and len(np.unique(i * grid["B"] + j)) > 10
    ref = oracle_intersect(oracle, tris, mirt.make_rays(starts, d))
    assert 0.2 < (ref["index"] >= 0).mean() < 1.0
    got, st = closest("device", d, starts, mirt.QUERY_BINNED)
    if name == "needles @ far":
        assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0, st
    else:
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_bins"] == grid["B"], st
    same_hits(got, ref, name)
    limits, _ = limits_for(ref)
    got, _ = occluded("device", d, starts, limits, mirt.QUERY_BINNED)
    assert np.array_equal(got, expected(ref, limits))


# ---- the structure is kept ---------------------------------------------------------------------------------------------------------------

def test_keeping_the_structure(oracle):
    tris, starts, planted, hits, limits, kind, want, want_null = batch_of(oracle, "soup2000")
    mirt.scene_upload(tris)                                                 # (a new scene version: nothing is held)
    n = 600
    got, st = closest("host", OBLIQUE, starts[:n], mirt.QUERY_BINNED)
    assert st["cube_source"] == 1 and st["cube_bins"] == 32 and st["shells"] == SHELLS, st
    same_hits(got, hits[:n], "built")
    for form in ("host", "device"):
        got, st = closest(form, OBLIQUE, starts[:n], mirt.QUERY_BINNED)
        assert st["cube_source"] == 2, st
        same_hits(got, hits[:n], "kept")
    got, st = occluded("device", OBLIQUE, starts[:n], limits[:n], mirt.QUERY_BINNED)
    assert st["cube_source"] == 2 and np.array_equal(got, want[:n]), st       # one structure serves both kinds
    got, st = closest("device", OBLIQUE, starts[:50], mirt.QUERY_AUTO)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2, st
    # a new direction
    d2 = np.array([0.37, -0.52, 0.8125], np.float32)
    ref2 = oracle_intersect(oracle, tris, mirt.make_rays(starts[:n], d2))
    got, st = closest("device", d2, starts[:n], mirt.QUERY_BINNED)
    assert st["cube_source"] == 1, st
    same_hits(got, ref2, "a new direction")
    got, st = closest("device", OBLIQUE, starts[:n], mirt.QUERY_BINNED)
    assert st["cube_source"] == 1, st                                         # one structure is kept
    # a kept binning pass of a standing view survives a call in between, and the frame's statistics stay its own
    view = mirt.make_view((0, 0, -2.5), oracle.rot_from_yaw(0.1, 1.0), 120.0, 160, 120)
    frames = [mirt.raytrace(view, LIGHTS[:1], mode=mirt.RT_BINNED) for _ in range(4)][2:]
    assert frames[1]["stats"]["mode_used"] == mirt.RT_BINNED and frames[1]["stats"]["bins_reused"] == 1, frames[1]["stats"]
    stats0, light, fan, occ = mirt.stats(), mirt.query_stats(), mirt.fan_stats(), mirt.occlusion_stats()
    got, st = closest("device", d2, starts[:n], mirt.QUERY_BINNED)
    assert st["cube_source"] == 1, st
    same_hits(got, ref2, "between two frames")
    assert (mirt.stats(), mirt.query_stats(), mirt.fan_stats(), mirt.occlusion_stats()) == (stats0, light, fan, occ)
    after = mirt.raytrace(view, LIGHTS[:1], mode=mirt.RT_BINNED)
    assert after["stats"]["bins_reused"] == 1, after["stats"]
    assert np.array_equal(after["xrgb"], frames[1]["xrgb"])
    # the scene moves
    eye = np.eye(3, dtype=np.float32).ravel()
    mirt.scene_transform(0, len(tris), eye, (0.0625, 0.0, 0.0))
    moved = oracle_intersect(oracle, mirt.scene_download(), mirt.make_rays(starts[:n], d2))
    got, st = closest("device", d2, starts[:n], mirt.QUERY_BINNED)
    assert st["cube_source"] == 1, st
    same_hits(got, moved, "after mirt_scene_transform")
    assert moved.tobytes() != ref2.tobytes()
    # a fresh library state
    mirt.shutdown()
    mirt.init(0)
    mirt.scene_upload(tris)
    got, st = closest("device", OBLIQUE, starts[:n], mirt.QUERY_BINNED)
    assert st["cube_source"] == 1, st
    same_hits(got, hits[:n], "after mirt_shutdown / mirt_init")


# ---- several frames in flight -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flight", [2, 4])
def test_frames_in_flight(oracle, flight):
    tris, starts, planted, hits, limits, kind, want, want_null = batch_of(oracle, "soup2000")
    mirt.scene_upload(tris)                                                 # (nothing is held: the first call builds, the others wait for it)
    n = len(starts)
    d_starts, d_lim = to_device(starts), to_device(limits)
    d_hits = [to_device(mirt.fresh_hits(n)) for _ in range(3)]
    outs = [DeviceArray((n + GUARD,), np.uint8, 0xAA) for _ in range(3)]
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        mirt.set_frames_in_flight(flight)
        for k in range(3):
            mirt.intersect_along_device(OBLIQUE, d_starts.ptr, n, d_hits[k].ptr)
            mirt.occluded_along_device(OBLIQUE, d_starts.ptr, n, d_lim.ptr if k % 2 == 0 else None, outs[k].ptr)
        mirt.sync()
        for k in range(3):
            same_hits(np.frombuffer(d_hits[k].read().tobytes(), mirt.HIT_DTYPE), hits, "call %d of six on %d streams" % (2 * k, flight))
            assert np.array_equal(checked(outs[k].read(), n, "call %d" % k), want if k % 2 == 0 else want_null), k
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
        mirt.set_frames_in_flight(1)
        for x in [d_starts, d_lim] + d_hits + outs:
            x.free()


# ---- rows offered, and the statistics ------------------------------------------------------------------------------------------------------

def test_rows_offered(oracle):
    """With profiling on, on soup2000 in BINNED mode: candidates <= rays * n // 8 -- a walk that offers every row to every ray does
    not pass (tests/test_along_host.py shows that the inputs leave the bound room) -- and the planted starts, no others, sweep."""
    tris, starts, planted, hits, limits, kind, want, want_null = batch_of(oracle, "soup2000")
    n, rays = len(tris), len(starts)
    mirt.set_profiling(True)
    try:
        got, st = closest("device", OBLIQUE, starts, mirt.QUERY_BINNED)
        same_hits(got, hits, "profiled")
        print(st)
        assert st["mode_used"] == mirt.QUERY_BINNED and st["shadow_rays"] == rays, st
        assert st["fallback_records"] == int(planted.sum()) > 50, (st, int(planted.sum()))
        assert 0 < st["tests"] <= st["candidates"] <= rays * n // 8, st
        assert st["candidates"] >= int(planted.sum()) * n                      # the sweeps count every row
        got, so = occluded("device", OBLIQUE, starts, limits, mirt.QUERY_BINNED)
        print(so)
        assert np.array_equal(got, want)
        assert so["shadow_rays"] == rays and so["tests"] <= so["candidates"] <= st["candidates"], (so, st)
    finally:
        mirt.set_profiling(False)
    got, st = closest("device", OBLIQUE, starts, mirt.QUERY_BINNED)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["shadow_rays"] == st["candidates"] == st["tests"] == st["fallback_records"] == 0, st


# ---- arguments -----------------------------------------------------------------------------------------------------------------------------

def test_argument_validation():
    lib = mirt.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    mirt.scene_upload(mirt.scene_cornell())
    d = np.array([0, 0, 1], np.float32)
    origins = np.zeros((4, 3), np.float32)
    hits = mirt.fresh_hits(4)
    out = np.full(4 + GUARD, 0xAA, np.uint8)
    for f in (lib.mirt_intersect_along, lib.mirt_intersect_along_device):
        assert f(p(d), p(origins), -1, p(hits)) == INVALID and f(p(d), None, 4, p(hits)) == INVALID and f(None, p(origins), 4, p(hits)) == INVALID
        assert f(None, None, 0, None) == 0 and f(p(d), p(origins), 0, p(hits)) == 0
    for f in (lib.mirt_occluded_along, lib.mirt_occluded_along_device):
        assert f(p(d), p(origins), -1, None, p(out)) == INVALID and f(p(d), p(origins), 4, None, None) == INVALID
        assert f(None, None, 0, None, None) == 0
    assert hits.tobytes() == mirt.fresh_hits(4).tobytes() and (out == 0xAA).all()
    assert lib.mirt_get_along_stats(None) == INVALID
    assert mirt.intersect_along(d, origins[:0]).shape == (0,) and mirt.occluded_along(d, origins[:0]).shape == (0,)


def test_no_scene():
    mirt.shutdown()
    mirt.init(0)
    with pytest.raises(mirt.MirtError, match="no scene uploaded"):
        mirt.intersect_along([0, 0, 1], np.zeros((2, 3), np.float32))
    with pytest.raises(mirt.MirtError, match="no scene uploaded"):
        mirt.occluded_along([0, 0, 1], np.zeros((2, 3), np.float32))
    st = mirt.along_stats()
    assert st["mode_used"] == 0 and st["cube_source"] == 0
