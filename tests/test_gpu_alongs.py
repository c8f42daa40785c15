"""Ray queries along several directions in one call on the GPU: mirt_intersect_alongs* (k_alongs_closest) and mirt_occluded_alongs*
(k_alongs_occluded) through groups of single-direction grids, and by brute force over the rays written out.

Expected records are the CPU oracle's ClosestIntersection per ray on the rays {origins[i], dirs[dir_of[i]]}
(query_helpers.oracle_intersect), compared bit for bit (same_hits); expected bytes are the reference's two steps on fresh-record
results, (index >= 0) & (distance < limit) (query_helpers.expected).  Occlusion buffers start as 0xAA with 64 guard bytes behind
them, record buffers carry four records of guard.  Directions are dealt to rays so that the lanes of a wave mix them; a (scene, K)
batch and its oracle records are computed once and shared by the ray counts, forms and modes compared with them."""
import ctypes as C

import numpy as np
import pytest

import mirt
import silhouette
from along_helpers import OBLIQUE, SHELLS, cell_of, directions, grid_of, plant_odd_starts, silhouette_starts
from devbuf import DeviceArray, to_device
from query_helpers import INF, NAN, expected, limits_for, make_batch, oracle_intersect, same_hits, scene_of

pytestmark = pytest.mark.gpu

GUARD = 64
INVALID = -3
NBATCH = 4097 + 300
COUNTS = (1, 257, 4096, NBATCH)
BOTH = (("brute", mirt.QUERY_BRUTE), ("binned", mirt.QUERY_BINNED))
_batches, _scenes = {}, {}


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_query_mode(mirt.QUERY_AUTO)
    mirt.set_profiling(False)
    mirt.set_frames_in_flight(1)
    mirt.shutdown()


# ---- directions, scenes, batches -----------------------------------------------------------------------------------------------------

def direction_list(K):
    """K directions out of along_helpers.directions(): the 29 in turn, each later round scaled by another dyadic factor (other bits,
    inside the window: 2^18 x 1.5 < 2^19); from K = 3 on the last one repeats the first bit for bit -- a direction may appear twice."""
    base = directions()
    out = [(base[k % len(base)] * np.float32(1.0 + 0.25 * (k // len(base)))).astype(np.float32) for k in range(K)]
    if K >= 3:
        out[-1] = out[0].copy()
    return np.ascontiguousarray(out, np.float32)


def deal(n, K):
    """dir_of for n rays: neighbours take different directions, and the deal shifts from wave to wave."""
    i = np.arange(n)
    return ((i * 7 + i // 64) % K).astype(np.int32)


def soup33000():
    if "soup33000" not in _scenes:
        _scenes["soup33000"] = mirt.scene_soup(77, 33000, 0.05)
        _scenes["soup33000"].setflags(write=False)
    return _scenes["soup33000"]


def extent_of(tris):
    return float(np.abs(np.asarray(tris).reshape(-1, 15)[:, :9]).max())


def rays_of(starts, dirs, of):
    return mirt.make_rays(starts, dirs[of])


def batch_of(oracle, name, K, nbatch=NBATCH):
    """Scene `name` uploaded; nbatch of make_batch's starts with the odd kinds planted, K directions dealt to them: the oracle's
    fresh-record results, limits of the eight kinds and both expectations."""
    tris, a, b = (soup33000(), 1.5, 1.0) if name == "soup33000" else scene_of(name)
    mirt.scene_upload(tris)
    if (name, K) not in _batches:
        starts, planted = plant_odd_starts(make_batch(nbatch, a, b)["start"], extent_of(tris))
        dirs, of = direction_list(K), deal(nbatch, K)
        hits = oracle_intersect(oracle, tris, rays_of(starts, dirs, of))
        limits, kind = limits_for(hits)
        v = dirs, of, starts, planted, hits, limits, kind, expected(hits, limits), expected(hits, None)
        for x in v:
            x.setflags(write=False)
        _batches[name, K] = v
    return (tris,) + _batches[name, K]


# ---- calls ---------------------------------------------------------------------------------------------------------------------------

def checked(buf, n, what):
    assert buf.shape == (n + GUARD,) and (buf[n:] == 0xAA).all(), "%s: wrote beyond %d rays" % (what, n)
    assert (buf[:n] <= 1).all(), "%s: %d bytes are neither 0 nor 1" % (what, int((buf[:n] > 1).sum()))
    return buf[:n]


def closest(form, dirs, of, starts, mode, hits=None):
    """(records, statistics) of one closest-hit call in `mode`; form: "host" or "device"."""
    n = len(starts)
    mirt.set_query_mode(mode)
    try:
        if form == "host":
            return mirt.intersect_alongs(dirs, of, starts, hits), mirt.along_stats()
        incoming = mirt.fresh_hits(n) if hits is None else hits
        d_starts, d_hits = to_device(starts), to_device(np.concatenate([incoming, mirt.fresh_hits(4)]))     # (four records of guard)
        d_of = None if of is None else to_device(np.ascontiguousarray(of, np.int32))
        try:
            mirt.intersect_alongs_device(dirs, None if d_of is None else d_of.ptr, d_starts.ptr, n, d_hits.ptr)
            st = mirt.along_stats()
            mirt.sync()
            back = np.frombuffer(d_hits.read().tobytes(), mirt.HIT_DTYPE)
            assert back[n:].tobytes() == mirt.fresh_hits(4).tobytes(), "wrote beyond %d records" % n
            return back[:n].copy(), st
        finally:
            d_starts.free(); d_hits.free()
            if d_of is not None:
                d_of.free()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


def occluded(form, dirs, of, starts, limits, mode, what=""):
    n = len(starts)
    mirt.set_query_mode(mode)
    try:
        if form == "host":
            buf = np.full(n + GUARD, 0xAA, np.uint8)
            mirt.occluded_alongs(dirs, of, starts, limits, buf[:n])
            return checked(buf, n, what), mirt.along_stats()
        d_starts, d_lim = to_device(starts), None if limits is None else to_device(limits)
        d_of = None if of is None else to_device(np.ascontiguousarray(of, np.int32))
        with DeviceArray((n + GUARD,), np.uint8, 0xAA) as d_out:
            try:
                mirt.occluded_alongs_device(dirs, None if d_of is None else d_of.ptr, d_starts.ptr, n, None if d_lim is None else d_lim.ptr, d_out.ptr)
                st = mirt.along_stats()
                return checked(d_out.read(), n, what), st
            finally:
                d_starts.free()
                for x in (d_lim, d_of):
                    if x is not None:
                        x.free()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


def mode_is(st, mode, what):
    if mode == mirt.QUERY_BRUTE:
        assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0 and st["cube_bins"] == 0, (what, st)
    else:
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] in (1, 2) and st["cube_bins"] >= 8 and st["shells"] == SHELLS, (what, st)


def all_calls_equal(batch, n, what, forms=("host", "device")):
    tris, dirs, of, starts, planted, hits, limits, kind, want, want_null = batch
    for mname, mode in BOTH:
        for form in forms:
            w = "%s, %d rays, %s, %s form" % (what, n, mname, form)
            got, st = closest(form, dirs, of[:n], starts[:n], mode)
            mode_is(st, mode, w)
            same_hits(got, hits[:n], w)
            got, st = occluded(form, dirs, of[:n], starts[:n], limits[:n], mode, w)
            mode_is(st, mode, w)
            assert np.array_equal(got, want[:n]), "%s: %d bytes differ (first at ray %d)" % (w, int((got != want[:n]).sum()), int(np.flatnonzero(got != want[:n])[0]))
            got, st = occluded(form, dirs, of[:n], starts[:n], None, mode, w + ", no limits")
            assert np.array_equal(got, want_null[:n]), "%s, NULL limits: %d bytes differ" % (w, int((got != want_null[:n]).sum()))


# ---- equals the oracle ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 2, 5, 32, 33, 70])
@pytest.mark.parametrize("name", ["cornell", "soup2000"])
def test_equals_the_oracle(oracle, name, K):
    """1, 2, 5 directions; a full group of 32; 33 and 70: two and three passes.  Ray counts 1, 257, 4096 and 4397."""
    batch = batch_of(oracle, name, K)
    hits, kind, want = batch[5], batch[7], batch[8]
    assert (hits["index"] >= 0).mean() > 0.05 and want[kind == 3].sum() > 10, "the batch hardly hits anything"
    for n in COUNTS:
        all_calls_equal(batch, n, "%s, K = %d" % (name, K))


@pytest.mark.parametrize("name,K", [("one", 1), ("one", 5), ("soup65", 2), ("soup65", 33)])
def test_small_scenes(oracle, name, K):
    batch = batch_of(oracle, name, K)
    for n in (1, 257, NBATCH):
        all_calls_equal(batch, n, "%s, K = %d" % (name, K), forms=("device",) if n != 257 else ("host", "device"))


@pytest.mark.parametrize("K", [15, 16, 17])
def test_a_grid_of_256_cells_a_side_holds_15_directions(oracle, K):
    """33 000 triangles: B = 256, a group holds 15 directions -- one pass, one and a direction, one and two."""
    batch = batch_of(oracle, "soup33000", K, 257)
    assert (batch[5]["index"] >= 0).mean() > 0.05
    all_calls_equal(batch, 257, "soup33000, K = %d" % K)
    tris, dirs, of, starts = batch[:4]
    _, st = closest("device", dirs, of, starts, mirt.QUERY_BINNED)
    assert st["cube_bins"] == 256 and st["cube_source"] == 2, st


# ---- equals the single call -------------------------------------------------------------------------------------------------------------

def test_equals_the_single_call(oracle):
    """Each direction's subset of the rays equals mirt_intersect_along / mirt_occluded_along on that subset."""
    tris, dirs, of, starts, planted, hits, limits, kind, want, want_null = batch_of(oracle, "soup2000", 5)
    got, st = closest("device", dirs, of, starts, mirt.QUERY_BINNED)
    occ, _ = occluded("device", dirs, of, starts, limits, mirt.QUERY_BINNED)
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        for k in range(5):
            sub = np.flatnonzero(of == k)
            assert len(sub) > 500
            single = mirt.intersect_along(dirs[k], starts[sub])
            assert mirt.along_stats()["mode_used"] == mirt.QUERY_BINNED
            same_hits(got[sub], single, "direction %d" % k)
            assert np.array_equal(occ[sub], mirt.occluded_along(dirs[k], starts[sub], limits[sub])), k
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


def test_one_direction_is_the_single_walk(oracle):
    """K = 1 with profiling on: the rows offered and tested are the single call's, so the two are one walk over one structure.
    Inside a (cell, shell) list the rows' order is whatever the sort's LDS atomics made it (csrc/bin_bucket_sort.hip: not
    deterministic, nor the same for two builds), and `tests` of a walk whose bound moves depends on it; `candidates` of a closest-hit
    walk does not (the list's end moves shell by shell).  So the counters are compared where they are functions of the structure
    alone: `candidates` from fresh records; both from records that already hold the answers (the bound never moves: a tie leaves
    the distance as it is); both for occlusion with every limit AT the closest distance (`<` never ends a walk early)."""
    tris, dirs, of, starts, planted, hits, limits, kind, want, want_null = batch_of(oracle, "soup2000", 1)
    at = np.where(hits["index"] >= 0, hits["distance"], np.float32(1.0)).astype(np.float32)
    mirt.set_profiling(True)
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        def closest_pair(incoming):
            a = mirt.intersect_alongs(dirs, None, starts, incoming)
            sa = mirt.along_stats()
            b = mirt.intersect_along(dirs[0], starts, incoming)
            sb = mirt.along_stats()
            assert a.tobytes() == b.tobytes()
            assert sa["mode_used"] == sb["mode_used"] == mirt.QUERY_BINNED and sa["cube_bins"] == sb["cube_bins"], (sa, sb)
            print(sa, sb)
            return sa, sb
        sa, sb = closest_pair(None)
        assert sa["shadow_rays"] == sb["shadow_rays"] == len(starts) and sa["candidates"] == sb["candidates"] > 0, (sa, sb)
        assert sa["fallback_records"] == sb["fallback_records"] == int(planted.sum())
        sa, sb = closest_pair(hits.copy())
        assert sa["candidates"] == sb["candidates"] > 0 and sa["tests"] == sb["tests"] > 0, (sa, sb)
        assert sa["tests"] < sa["candidates"]
        a = mirt.occluded_alongs(dirs, None, starts, at)
        sa = mirt.along_stats()
        b = mirt.occluded_along(dirs[0], starts, at)
        sb = mirt.along_stats()
        print(sa, sb)
        assert np.array_equal(a, b) and not a.any()
        assert sa["candidates"] == sb["candidates"] > 0 and sa["tests"] == sb["tests"] > 0, (sa, sb)
    finally:
        mirt.set_profiling(False)
        mirt.set_query_mode(mirt.QUERY_AUTO)


# ---- incoming records, limits, odd starts ------------------------------------------------------------------------------------------------

def test_incoming_records(oracle):
    """The records an earlier ray left (another direction's results), and records with negative, NaN, +inf and zero distances, and a
    tie with the ray's own closest hit (every kind test_gpu_along.py::test_incoming_records plants)."""
    tris, dirs, of, starts, planted, hits, limits, kind, want, want_null = batch_of(oracle, "soup2000", 5)
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
        ref = oracle_intersect(oracle, tris, rays_of(starts[:n], dirs, of[:n]), incoming)
        for mname, mode in BOTH:
            for form in ("host", "device"):
                got, st = closest(form, dirs, of[:n], starts[:n], mode, incoming.copy())
                mode_is(st, mode, iname)
                same_hits(got, ref, "%s, %s, %s form" % (iname, mname, form))
    kept = (odd["distance"] < 0) | np.isnan(odd["distance"])
    assert ref[kept].tobytes() == odd[kept].tobytes() and (ref["index"][2::7] >= 0).sum() > 20


def test_limits(oracle):
    """At the closest distance, one float above it, one float below it, and NULL, for the rays that hit."""
    tris, dirs, of, starts, planted, hits, limits, kind, want, want_null = batch_of(oracle, "soup2000", 5)
    hit = np.flatnonzero(hits["index"] >= 0)[:1500]
    d = hits["distance"][hit]
    assert len(hit) > 500
    for mname, mode in BOTH:
        for lim, byte in ((d, 0), (np.nextafter(d, INF), 1), (np.nextafter(d, np.float32(0)), 0), (None, 1)):
            got, _ = occluded("device", dirs, of[hit], starts[hit], lim, mode)
            assert (got == byte).all(), (mname, byte, int((got != byte).sum()))


def test_odd_starts_sweep(oracle):
    """plant_odd_starts' rays (1e9, NaN, infinite, beyond the structure's reach) sweep the scene, no others, and equal the oracle."""
    tris, dirs, of, starts, planted, hits, limits, kind, want, want_null = batch_of(oracle, "soup2000", 33)
    mirt.set_profiling(True)
    try:
        got, st = closest("device", dirs, of, starts, mirt.QUERY_BINNED)
        same_hits(got, hits, "profiled")
        print(st)
        assert st["mode_used"] == mirt.QUERY_BINNED and st["shadow_rays"] == len(starts), st        # (summed over the two passes)
        assert st["fallback_records"] == int(planted.sum()) > 50, (st, int(planted.sum()))
        assert st["candidates"] >= int(planted.sum()) * len(tris) and 0 < st["tests"] <= st["candidates"], st
        occ, so = occluded("device", dirs, of, starts, limits, mirt.QUERY_BINNED)
        assert np.array_equal(occ, want) and so["shadow_rays"] == len(starts), so
    finally:
        mirt.set_profiling(False)
    same_hits(got[planted], hits[planted], "the planted starts")


# ---- indices outside the list --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [5, 33])
def test_indices_outside_the_list(oracle, K):
    """-1, K and 2^30: the host form refuses with nothing written; the device form leaves the record unwritten and writes byte 0,
    under both modes, and the guards around the buffers stay intact."""
    tris, dirs, of, starts, planted, hits, limits, kind, want, want_null = batch_of(oracle, "soup2000", K)
    n = 700
    idx = of[:n].copy()
    stray = np.zeros(n, bool)
    for j, bad in enumerate((-1, K, 2 ** 30)):
        idx[3 + j::37] = bad
        stray[3 + j::37] = True
    incoming = mirt.fresh_hits(n)
    incoming["distance"][::2] = INF                                        # (records any hit would replace)
    incoming["index"][::2] = 777
    ref = oracle_intersect(oracle, tris, rays_of(starts[:n], dirs, of[:n]), incoming)
    ref[stray] = incoming[stray]
    want_b = np.where(stray, 0, want[:n]).astype(np.uint8)
    for mname, mode in BOTH:
        got, st = closest("device", dirs, idx, starts[:n], mode, incoming.copy())
        mode_is(st, mode, mname)
        same_hits(got, ref, "%s: records" % mname)
        occ, st = occluded("device", dirs, idx, starts[:n], limits[:n], mode, mname)
        assert np.array_equal(occ, want_b), (mname, int((occ != want_b).sum()))
        occ, st = occluded("device", dirs, idx, starts[:n], None, mode, mname)
        assert np.array_equal(occ, np.where(stray, 0, want_null[:n])), mname
        mirt.set_query_mode(mode)
        try:
            rec = incoming.copy()
            with pytest.raises(mirt.MirtError, match=r"dir_of\[3\] = -1 is outside \[0, %d\)" % K):
                mirt.intersect_alongs(dirs, idx, starts[:n], rec)
            lib = mirt.load()
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            buf = np.full(n + GUARD, 0xAA, np.uint8)
            s32 = np.ascontiguousarray(starts[:n], np.float32)
            assert lib.mirt_intersect_alongs(p(dirs), K, p(idx), p(s32), n, p(rec)) == INVALID and rec.tobytes() == incoming.tobytes()
            assert lib.mirt_occluded_alongs(p(dirs), K, p(idx), p(s32), n, None, p(buf)) == INVALID and (buf == 0xAA).all()
        finally:
            mirt.set_query_mode(mirt.QUERY_AUTO)


# ---- directions no grid is built for ----------------------------------------------------------------------------------------------------

def edge_on_scene(d, count):
    """Cornell's box and `count` soup triangles turned to within 2^-22 rad of edge-on to d (test_gpu_along.py::edge_on_scene with
    more of them: beyond the every-ray list's floor of 64 rows, so that the direction is given up)."""
    rng = np.random.default_rng(23)
    dh = np.asarray(d, np.float64) / np.linalg.norm(d)
    v = []
    for k in range(count):
        e1 = rng.uniform(-0.3, 0.3, 3)
        nperp = np.cross(e1, dh)
        nperp /= np.linalg.norm(nperp)
        theta = 2.0 ** -22 * (1, -1, 0.5, -0.25, 0, 1, -1, 0.125)[k % 8]
        e2 = rng.uniform(-0.5, 0.5) * e1 + 0.25 * dh + theta * 0.25 * nperp
        v0 = rng.uniform(-0.5, 0.5, 3)
        v.append([v0, v0 + e1, v0 + e2])
    return np.concatenate([mirt.scene_cornell(), silhouette.finish(v)])


def brute_and_builds_nothing(oracle, tris, dirs, what):
    """BINNED is asked for: the whole call is BRUTE and equals the oracle, and so is the second call, which builds nothing."""
    rng = np.random.default_rng(31)
    n = 600
    starts = rng.uniform(-0.95, 0.95, (n, 3)).astype(np.float32)
    of = deal(n, len(dirs))
    ref = oracle_intersect(oracle, tris, rays_of(starts, dirs, of))
    assert (ref["index"] >= 0).mean() > 0.3
    limits, _ = limits_for(ref)
    for call in range(2):
        got, st = closest("device", dirs, of, starts, mirt.QUERY_BINNED)
        assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0 and st["cube_bins"] == 0, (what, call, st)
        same_hits(got, ref, "%s, call %d" % (what, call))
        occ, st = occluded("host", dirs, of, starts, limits, mirt.QUERY_BINNED)
        assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0, (what, call, st)
        assert np.array_equal(occ, expected(ref, limits)), (what, call)
    # (a list without the unfit direction bins)
    fit = np.ascontiguousarray(dirs[:2])
    _, st = closest("device", fit, of % 2, starts, mirt.QUERY_BINNED)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 1, (what, st)


def test_a_direction_outside_the_window(oracle):
    tris = scene_of("soup2000")[0]
    mirt.scene_upload(tris)
    dirs = np.array([OBLIQUE, [0.2, 0.3, -1.0], [0, 0, 2.0 ** 20], [1, 0, 0]], np.float32)
    brute_and_builds_nothing(oracle, tris, dirs, "a direction of magnitude 2^20")


def test_an_edge_on_scene(oracle):
    """An axis direction with 100 triangles edge-on to it among 130: its every-ray list outgrows max(n / 8, 64)."""
    axis = np.array([0, -1, 0], np.float32)
    tris = edge_on_scene(axis, 100)
    mirt.scene_upload(tris)
    dirs = np.array([OBLIQUE, [0.2, 0.3, -1.0], axis], np.float32)
    brute_and_builds_nothing(oracle, tris, dirs, "an edge-on scene")
    # the single call gives this direction up too: one rule
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        mirt.intersect_along(axis, np.zeros((4, 3), np.float32))
        assert mirt.along_stats()["mode_used"] == mirt.QUERY_BRUTE
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


# ---- silhouette probes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,targets", [("soup2000", range(10)), ("needles", range(0, 150, 15))])
def test_silhouette_probes(oracle, name, targets):
    """Starts within 2^-20 .. 2^-8 of projected edges, vertices and the grids' cell borders, twins to either side, for three
    directions at once; every direction's probes are offered to all three."""
    tris = silhouette.scene_of(oracle, name)[0]
    mirt.scene_upload(tris)
    info = mirt.scene_info()
    dirs = np.array([OBLIQUE, [-0.6, 1.0, 0.35], [0.2, 0.3, -1.0]], np.float32)
    parts = []
    for d in dirs:
        grid = grid_of(d, info["bbox_lo"], info["bbox_hi"], len(tris))
        s = silhouette_starts(tris, d, targets, grid)
        i, j = cell_of(grid, s)
        assert (i >= 0).mean() > 0.9
        parts.append(s)
    own = np.concatenate([np.full(len(s), k, np.int32) for k, s in enumerate(parts)])
    starts = np.concatenate(parts)
    rng = np.random.default_rng(37)
    perm = rng.permutation(len(starts))
    starts, own = np.ascontiguousarray(starts[perm]), own[perm]
    assert 600 < len(starts) < 9000, len(starts)
    for shift in (0, 1):                                                    # its own direction, and its neighbour's
        of = ((own + shift) % 3).astype(np.int32)
        ref = oracle_intersect(oracle, tris, rays_of(starts, dirs, of))
        if shift == 0:
            assert 0.2 < (ref["index"] >= 0).mean() < 1.0
        got, st = closest("device", dirs, of, starts, mirt.QUERY_BINNED)
        assert st["mode_used"] == mirt.QUERY_BINNED, st
        same_hits(got, ref, "%s, shift %d" % (name, shift))
        limits, _ = limits_for(ref)
        occ, _ = occluded("device", dirs, of, starts, limits, mirt.QUERY_BINNED)
        assert np.array_equal(occ, expected(ref, limits))


# ---- the groups are kept ----------------------------------------------------------------------------------------------------------------

def test_keeping_the_groups(oracle):
    tris, dirs, of, starts, planted, hits, limits, kind, want, want_null = batch_of(oracle, "soup2000", 70)
    mirt.scene_upload(tris)                                                 # (a new scene version: nothing is held)
    n = 900
    got, st = closest("device", dirs, of[:n], starts[:n], mirt.QUERY_BINNED)
    assert st["cube_source"] == 1 and st["cube_bins"] == 32 and st["shells"] == SHELLS, st
    same_hits(got, hits[:n], "built")
    for form in ("host", "device"):
        got, st = closest(form, dirs, of[:n], starts[:n], mirt.QUERY_BINNED)
        assert st["cube_source"] == 2, st                                   # three passes, three groups, all held
        same_hits(got, hits[:n], "kept")
    occ, st = occluded("device", dirs, of[:n], starts[:n], limits[:n], mirt.QUERY_BINNED)
    assert st["cube_source"] == 2 and np.array_equal(occ, want[:n]), st       # the two kinds share the groups
    got, st = closest("device", dirs, of[:50], starts[:50], mirt.QUERY_AUTO)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2, st    # AUTO: every group is held
    # a single-direction call in between neither evicts nor is evicted
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        single = mirt.intersect_along(OBLIQUE, starts[:n])
        assert mirt.along_stats()["cube_source"] == 1
        got, st = closest("device", dirs, of[:n], starts[:n], mirt.QUERY_BINNED)
        assert st["cube_source"] == 2, st
        mirt.set_query_mode(mirt.QUERY_BINNED)
        again = mirt.intersect_along(OBLIQUE, starts[:n])
        assert mirt.along_stats()["cube_source"] == 2 and again.tobytes() == single.tobytes()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
    # a reordered list rebuilds (the key is the directions in order); only the passes that changed
    swapped = dirs.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    of2 = np.where(of == 1, 2, np.where(of == 2, 1, of)).astype(np.int32)
    got, st = closest("device", swapped, of2[:n], starts[:n], mirt.QUERY_BINNED)
    assert st["cube_source"] == 1, st
    same_hits(got, hits[:n], "reordered")
    got, st = closest("device", swapped, of2[:n], starts[:n], mirt.QUERY_BINNED)
    assert st["cube_source"] == 2, st
    # the scene moves
    eye = np.eye(3, dtype=np.float32).ravel()
    mirt.scene_transform(0, len(tris), eye, (0.0625, 0.0, 0.0))
    moved = oracle_intersect(oracle, mirt.scene_download(), rays_of(starts[:n], dirs, of[:n]))
    got, st = closest("device", dirs, of[:n], starts[:n], mirt.QUERY_BINNED)
    assert st["cube_source"] == 1, st
    same_hits(got, moved, "after mirt_scene_transform")
    assert moved.tobytes() != hits[:n].tobytes()
    # a fresh library state
    mirt.shutdown()
    mirt.init(0)
    mirt.scene_upload(tris)
    got, st = closest("device", dirs, of[:n], starts[:n], mirt.QUERY_BINNED)
    assert st["cube_source"] == 1, st
    same_hits(got, hits[:n], "after mirt_shutdown / mirt_init")


# ---- several frames in flight -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flight", [2, 4])
def test_frames_in_flight(oracle, flight):
    """Device forms alternating over two direction lists (5 directions, and 33: two passes), closest hits and occlusion."""
    lists = [batch_of(oracle, "soup2000", 5), batch_of(oracle, "soup2000", 33)]
    mirt.scene_upload(lists[0][0])                                          # (nothing is held: the first calls build, the others wait)
    n = 2000
    starts = lists[0][3]
    d_starts = to_device(starts[:n])
    d_of = [to_device(np.ascontiguousarray(b[2][:n], np.int32)) for b in lists]
    d_lim = [to_device(b[6][:n]) for b in lists]
    d_hits = [to_device(mirt.fresh_hits(n)) for _ in range(6)]
    outs = [DeviceArray((n + GUARD,), np.uint8, 0xAA) for _ in range(6)]
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        mirt.set_frames_in_flight(flight)
        for k in range(6):
            b = lists[k % 2]
            mirt.intersect_alongs_device(b[1], d_of[k % 2].ptr, d_starts.ptr, n, d_hits[k].ptr)
            mirt.occluded_alongs_device(b[1], d_of[k % 2].ptr, d_starts.ptr, n, d_lim[k % 2].ptr if k % 3 else None, outs[k].ptr)
        mirt.sync()
        for k in range(6):
            b = lists[k % 2]
            same_hits(np.frombuffer(d_hits[k].read().tobytes(), mirt.HIT_DTYPE), b[5][:n], "call %d of twelve on %d streams" % (2 * k, flight))
            assert np.array_equal(checked(outs[k].read(), n, "call %d" % k), (b[8] if k % 3 else b[9])[:n]), k
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
        mirt.set_frames_in_flight(1)
        for x in [d_starts] + d_of + d_lim + d_hits + outs:
            x.free()


# ---- arguments, no scene ---------------------------------------------------------------------------------------------------------------

def test_argument_validation():
    lib = mirt.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    mirt.scene_upload(mirt.scene_cornell())
    dirs = np.array([[0, 0, 1], [0, 1, 0]], np.float32)
    of = np.array([0, 1, 1, 0], np.int32)
    origins = np.zeros((4, 3), np.float32)
    hits = mirt.fresh_hits(4)
    out = np.full(4 + GUARD, 0xAA, np.uint8)
    for f in (lib.mirt_intersect_alongs, lib.mirt_intersect_alongs_device):
        assert f(p(dirs), -1, p(of), p(origins), 4, p(hits)) == INVALID and f(p(dirs), 2, p(of), p(origins), -1, p(hits)) == INVALID
        assert f(p(dirs), 2, p(of), None, 4, p(hits)) == INVALID and f(None, 2, p(of), p(origins), 4, p(hits)) == INVALID
        assert f(p(dirs), 0, p(of), p(origins), 4, p(hits)) == INVALID and f(p(dirs), 2, None, p(origins), 4, p(hits)) == INVALID
        assert f(None, 0, None, None, 0, None) == 0 and f(p(dirs), 2, p(of), p(origins), 0, p(hits)) == 0
    for f in (lib.mirt_occluded_alongs, lib.mirt_occluded_alongs_device):
        assert f(p(dirs), 2, p(of), p(origins), -1, None, p(out)) == INVALID and f(p(dirs), 2, p(of), p(origins), 4, None, None) == INVALID
        assert f(p(dirs), 2, None, p(origins), 4, None, p(out)) == INVALID
        assert f(None, 0, None, None, 0, None, None) == 0
    assert hits.tobytes() == mirt.fresh_hits(4).tobytes() and (out == 0xAA).all()
    assert mirt.intersect_alongs(dirs, of[:0], origins[:0]).shape == (0,) and mirt.occluded_alongs(dirs, of[:0], origins[:0]).shape == (0,)
    # one direction needs no indices
    one = mirt.intersect_alongs(dirs[:1], None, origins)
    assert one.tobytes() == mirt.intersect_along(dirs[0], origins).tobytes()


def test_no_scene():
    mirt.shutdown()
    mirt.init(0)
    dirs = np.array([[0, 0, 1], [0, 1, 0]], np.float32)
    with pytest.raises(mirt.MirtError, match="no scene uploaded"):
        mirt.intersect_alongs(dirs, [0, 1], np.zeros((2, 3), np.float32))
    with pytest.raises(mirt.MirtError, match="no scene uploaded"):
        mirt.occluded_alongs(dirs, [0, 1], np.zeros((2, 3), np.float32))
    st = mirt.along_stats()
    assert st["mode_used"] == 0 and st["cube_source"] == 0
