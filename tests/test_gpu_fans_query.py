"""Origin fans from many origins in one call on the GPU: mirt_intersect_fans* -- every ray through its bin of ITS origin's positions
in a cube of up to 32 origins (k_query_fans_binned), in passes when the call has more, or written out and swept by
mirt_intersect's kernels (k_query_fans_expand) -- against mirt_intersect on the expanded rays {origins[origin_of[i]], dirs[i]} and
against the CPU oracle's ClosestIntersection.

Every comparison is bit-exact over all 20 bytes of every record (same_hits of query_helpers.py).  The reference of a batch is
computed once and shared by the modes and forms that are compared with it."""
import ctypes as C

import numpy as np
import pytest

import mirt
from devbuf import hip_fill, to_device
from query_helpers import INSIDE, LIGHTS, OUTSIDE, oracle_intersect, same_hits, seam_directions
from query_helpers import fan_scene_of as scene_of

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
ORACLE_RAYS = 256
NRAYS = 6000
INVALID = -3
MODES = (("brute", mirt.QUERY_BRUTE), ("auto", mirt.QUERY_AUTO), ("binned", mirt.QUERY_BINNED))      # (AUTO before a cube is held)
BOTH = (MODES[0], MODES[2])
_batches = {}


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_query_mode(mirt.QUERY_AUTO)
    mirt.set_profiling(False)
    mirt.set_frames_in_flight(1)
    mirt.shutdown()


# ---- origins, batches, calls ---------------------------------------------------------------------------------------------------

def origins_for(tris, K, seed=3):
    """K origins: inside the scene's box, outside it and on a vertex of triangle 0 first (K = 1: inside; K = 2: inside, vertex), then
    alternately inside U[-0.4, 0.4]^3 and outside, at 2 .. 3 from the centre."""
    rng = np.random.default_rng(seed)
    first = [INSIDE, np.array(tris[0, 0:3], np.float32), OUTSIDE]
    out = [first[k] for k in range(min(K, 3))]
    for k in range(3, K):
        if k % 2:
            out.append(rng.uniform(-0.4, 0.4, 3))
        else:
            v = rng.normal(size=3)
            out.append(v / np.linalg.norm(v) * rng.uniform(2.0, 3.0))
    return np.ascontiguousarray(np.array(out, np.float32).reshape(K, 3))


def make_batch(origins, b, nrays=NRAYS, seed=5):
    """(origin_of, dirs): for every origin the seam directions and their one-ulp neighbours, then directions towards U[-b, b]^3 from
    origins drawn at random; the whole batch shuffled, so that every wave mixes origins and both kinds of direction."""
    K = len(origins)
    rng = np.random.default_rng(seed)
    seams = seam_directions()
    extra = max(nrays - K * len(seams), 16 * K)
    of = np.concatenate([np.repeat(np.arange(K), len(seams)), rng.integers(0, K, extra)]).astype(np.int32)
    target = rng.uniform(-b, b, (extra, 3)).astype(np.float32)
    dirs = np.concatenate([np.tile(seams, (K, 1)), (target - origins[of[K * len(seams):]]).astype(np.float32)])
    order = rng.permutation(len(of))
    return np.ascontiguousarray(of[order]), np.ascontiguousarray(dirs[order].astype(np.float32))


def expanded(origins, of, dirs):
    return mirt.make_rays(origins[of], dirs)


def reference(origins, of, dirs, hits=None):
    """mirt.intersect on the expanded rays: brute force whatever the query mode."""
    return mirt.intersect(expanded(origins, of, dirs), hits)


def fans(origins, of, dirs, mode, hits=None):
    mirt.set_query_mode(mode)
    try:
        out = mirt.intersect_fans(origins, of, dirs, hits)
        return out, mirt.fan_stats()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


def fans_device(origins, of, dirs, mode, hits=None, fill=None):
    """The device form into a record buffer that held `fill` bytes before the records were copied in."""
    from devbuf import hip
    hits = mirt.fresh_hits(len(dirs)) if hits is None else hits
    d_of, d_dirs, d_hits = to_device(of), to_device(dirs), to_device(hits)
    try:
        if fill is not None:
            assert hip_fill(d_hits, fill)
            assert hip().hipMemcpy(d_hits.ptr, hits.ctypes.data_as(C.c_void_p), hits.nbytes, 1) == 0
        mirt.set_query_mode(mode)
        mirt.intersect_fans_device(origins, d_of.ptr, d_dirs.ptr, len(dirs), d_hits.ptr)
        st = mirt.fan_stats()
        return d_hits.read().view(mirt.HIT_DTYPE).reshape(-1), st
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
        for d in (d_of, d_dirs, d_hits):
            d.free()


def batch_of(name, K):
    """Scene `name` uploaded, and the shared batch of K origins with its reference."""
    tris, b = scene_of(name)
    mirt.scene_upload(tris)
    if (name, K) not in _batches:
        origins = origins_for(tris, K)
        of, dirs = make_batch(origins, b)
        want = reference(origins, of, dirs)
        want.setflags(write=False)
        _batches[name, K] = origins, of, dirs, want
    return (tris,) + _batches[name, K]


# ---- 1. equality with mirt_intersect --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 2, 5, 32, 33, 70])
@pytest.mark.parametrize("name", ["cornell", "soup2000"])
def test_equals_intersect(oracle, name, K):
    tris, origins, of, dirs, want = batch_of(name, K)
    what = "%s, %d origins" % (name, K)
    assert len(np.unique(of)) == K
    assert K == 1 or all(len(np.unique(of[w:w + 64])) > 1 for w in range(0, len(of) - 64, 64)), "a wave with one origin only"
    same_hits(want[:ORACLE_RAYS], oracle_intersect(oracle, tris, expanded(origins, of, dirs)[:ORACLE_RAYS]), what + ": reference vs oracle")
    if name == "soup2000":
        assert 0.05 <= (want["index"] >= 0).mean() <= 0.98
    for mname, mode in MODES:
        got, st = fans(origins, of, dirs, mode)
        same_hits(got, want, "%s, %s, host form" % (what, mname))
        if mode == mirt.QUERY_BRUTE:
            assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0 and st["cube_bins"] == 0, st
        elif mode == mirt.QUERY_BINNED:
            assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] in (1, 2) and st["cube_bins"] in (64, 128, 256) and st["shells"] >= 1, st
        else:
            # AUTO with no cube held (batch_of uploaded the scene anew): the single fan's rule -- 30 triangles never bin, 2000 always do
            assert st["mode_used"] == (mirt.QUERY_BINNED if name == "soup2000" else mirt.QUERY_BRUTE), st
        got, st2 = fans_device(origins, of, dirs, mode, fill=0x5a)
        same_hits(got, want, "%s, %s, device form" % (what, mname))
        assert st2["mode_used"] == st["mode_used"]
    same_hits(got[:ORACLE_RAYS], oracle_intersect(oracle, tris, expanded(origins, of, dirs)[:ORACLE_RAYS]), what + ": vs oracle")


# ---- 2. incoming records ------------------------------------------------------------------------------------------------------------

def test_incoming_records(oracle):
    tris, origins, of, dirs, fresh = batch_of("soup2000", 5)
    hit = fresh["index"] >= 0
    rec = mirt.fresh_hits(len(dirs))
    kind = np.arange(len(dirs)) % 8
    own = (kind != 0) & (kind != 1)                                          # 0: fresh
    rec["position"][own] = (9, 9, 9)
    rec["index"][own] = 7
    rec[kind == 1] = fresh[kind == 1]                                        # 1: what an earlier call left
    rec["distance"][kind == 2] = fresh["distance"][kind == 2]               # the ray's own hit distance: the record loses the tie
    rec["distance"][kind == 3] = np.nextafter(fresh["distance"][kind == 3], np.float32(0))       # just below: stays, all 20 bytes
    rec["distance"][kind == 4] = -1
    rec["distance"].view(np.uint32)[kind == 5] = 0x7fc12345                 # NaN with a payload
    rec["distance"][kind == 6] = np.float32("inf")
    rec["distance"][kind == 7] = 1.0                                        # a record of the caller's own somewhere in the scene
    rec["index"][kind == 7] = 123456
    want = reference(origins, of, dirs, rec)
    same_hits(want[:ORACLE_RAYS], oracle_intersect(oracle, tris, expanded(origins, of, dirs)[:ORACLE_RAYS], rec[:ORACLE_RAYS]), "reference vs oracle")
    for mname, mode in BOTH:
        for form in (fans, lambda *a: fans_device(*a, fill=0xa5)):
            got, _ = form(origins, of, dirs, mode, rec)
            same_hits(got, want, "incoming records, " + mname)
            same_hits(got[hit & (kind == 2)], fresh[hit & (kind == 2)], "equal: replaced")
            same_hits(got[kind == 1], fresh[kind == 1], "an earlier call's records")
            for k in (3, 4, 5):
                # (from the vertex origin triangle 0 is met at distance 0, and nothing lies "just below" that: those records tie)
                keep = (kind == k) & ~((k == 3) & (fresh["distance"] == 0))
                assert got[keep].tobytes() == rec[keep].tobytes(), k
            assert ((kind == 3) & (fresh["distance"] == 0)).sum() < (kind == 3).sum() / 2
            same_hits(got[hit & (kind == 6)], fresh[hit & (kind == 6)], "inf: replaced")
            assert got[~hit & (kind == 6)].tobytes() == rec[~hit & (kind == 6)].tobytes()
            assert (got["index"][kind == 7] == 123456).any() and (got["index"][kind == 7] != 123456).any()
    assert hit[kind == 2].sum() > 100 and hit[kind == 6].sum() > 100


# ---- 3. per-ray fallback ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [5, 33])
def test_per_ray_fallback(oracle, K):
    tris, origins, of, dirs, _ = batch_of("soup2000", K)
    odd_dirs = dirs.copy()
    ordinary = np.flatnonzero((np.abs(dirs).max(axis=1) > 1e-3) & (np.abs(dirs).max(axis=1) < 1e3) & (np.abs(dirs).min(axis=1) > 0))
    odd = np.concatenate([w + np.array([3, 17, 40]) for w in range(0, len(dirs) - 64, 64)])       # three in every wave
    odd = np.intersect1d(odd, ordinary)
    odd = np.union1d(odd, np.intersect1d(np.flatnonzero(of == K - 1), ordinary)[:8])             # (K = 33: some in the second pass)
    assert len(odd) > 100 and (of[odd] == K - 1).any() and (of[odd] < K - 1).any()
    for k, i in enumerate(odd):
        kind = k % 5
        unit = dirs[i] / np.abs(dirs[i]).max()                              # largest component exactly +-1
        if kind == 0:
            odd_dirs[i] = 0
        elif kind == 1:
            odd_dirs[i][k % 3] = np.float32("nan")
        elif kind == 2:
            odd_dirs[i][k % 3] = np.float32("inf") * (1 if k % 2 else -1)
        elif kind == 3:
            odd_dirs[i] = unit * np.float32(2.0 ** -33)                    # just below the window
        else:
            odd_dirs[i] = unit * np.float32(2.0 ** 19)                     # its upper end, outside
    assert np.abs(odd_dirs[odd[3::5]]).max(axis=1).tolist() == [2.0 ** -33] * len(odd[3::5])
    want = reference(origins, of, odd_dirs)
    first = np.sort(odd)[:ORACLE_RAYS]
    same_hits(want[first], oracle_intersect(oracle, tris, expanded(origins, of, odd_dirs)[first]), "reference vs oracle")
    assert (want["index"][odd[3::5]] >= 0).any() and (want["index"][odd[4::5]] >= 0).any()       # tiny and huge ones do find hits
    mirt.set_profiling(True)
    try:
        got, st = fans(origins, of, odd_dirs, mirt.QUERY_BINNED)
        same_hits(got, want, "directions outside the window, binned")
        assert st["mode_used"] == mirt.QUERY_BINNED and st["fallback_records"] == len(odd), (st, len(odd))
        assert st["shadow_rays"] == len(dirs) and 0 < st["tests"] <= st["candidates"], st
        got, st = fans(origins, of, dirs, mirt.QUERY_BINNED)
        assert st["fallback_records"] == 0 and st["shadow_rays"] == len(dirs), st
    finally:
        mirt.set_profiling(False)
    same_hits(fans(origins, of, odd_dirs, mirt.QUERY_BRUTE)[0], want, "directions outside the window, brute")
    _, st = fans(origins, of, odd_dirs, mirt.QUERY_BINNED)                 # without profiling the counters stay zero
    assert st["fallback_records"] == 0 and st["shadow_rays"] == 0 and st["candidates"] == 0


# ---- 4. indices outside the list ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [5, 33])
def test_out_of_range_indices(K):
    tris, origins, of, dirs, want = batch_of("soup2000", K)
    bad_of = of.copy()
    bad = np.concatenate([w + np.array([1, 30, 63]) for w in range(0, len(of) - 64, 64)])
    bad_of[bad[0::3]] = -1
    bad_of[bad[1::3]] = K
    bad_of[bad[2::3]] = 2 ** 30
    bad_of[bad[0]] = -2 ** 31
    rec = mirt.fresh_hits(len(dirs))
    rec["position"] = (7, 7, 7)
    rec["index"] = 99
    good = np.ones(len(of), bool)
    good[bad] = False
    want = reference(origins, of, dirs, rec)
    for mname, mode in BOTH:
        got, st = fans_device(origins, bad_of, dirs, mode, rec, fill=0xc3)
        assert st["mode_used"] == mode
        assert got[bad].tobytes() == rec[bad].tobytes(), "%s: a ray with an index outside the list wrote its record" % mname
        same_hits(got[good], want[good], "the rays around them, " + mname)
    # the host form looks first and writes nothing
    lib = mirt.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for i in (bad[0], bad[1], bad[2], bad[3]):
        one = of.copy()
        one[i] = bad_of[i]
        hits = rec.copy()
        assert lib.mirt_intersect_fans(p(origins), K, p(one), p(dirs), len(dirs), p(hits)) == INVALID
        assert b"origin_of[%d]" % i in lib.mirt_last_error()
        assert hits.tobytes() == rec.tobytes()


# ---- 5. an origin the frame path would not bin ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["1e9", "nan", "inf"])
def test_unbinnable_origin(oracle, what):
    tris, origins, of, dirs, _ = batch_of("soup2000", 5)
    origins = origins.copy()
    origins[3] = {"1e9": (1e9, 0, 0), "nan": (0.1, np.nan, 0.2), "inf": (0, 0, -np.inf)}[what]
    want = reference(origins, of, dirs)
    same_hits(want[:ORACLE_RAYS], oracle_intersect(oracle, tris, expanded(origins, of, dirs)[:ORACLE_RAYS]), "reference vs oracle")
    assert (want["index"][of != 3] >= 0).sum() > 1000
    for mname, mode in MODES:
        got, st = fans(origins, of, dirs, mode)
        assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0, (mname, st)
        same_hits(got, want, "origin %s among ordinary ones, %s" % (what, mname))


# ---- 6. one origin, no indices -------------------------------------------------------------------------------------------------------

def test_single_origin_without_indices():
    tris, origins, of, dirs, want = batch_of("soup2000", 1)
    for mname, mode in MODES:
        got, st = fans(origins, None, dirs, mode)
        same_hits(got, want, "origin_of NULL, " + mname)
        mirt.set_query_mode(mode)
        try:
            same_hits(got, mirt.intersect_from(origins[0], dirs), "vs intersect_from, " + mname)
            assert mirt.fan_stats()["mode_used"] == st["mode_used"]
        finally:
            mirt.set_query_mode(mirt.QUERY_AUTO)
    d_dirs, d_hits = to_device(dirs), to_device(mirt.fresh_hits(len(dirs)))
    mirt.intersect_fans_device(origins, None, d_dirs.ptr, len(dirs), d_hits.ptr)
    same_hits(d_hits.read().view(mirt.HIT_DTYPE).reshape(-1), want, "device form, origin_of NULL")
    d_dirs.free(), d_hits.free()


def test_single_fan_and_one_origin_fans_are_one_walk():
    """k_query_fan_binned and k_query_fans_binned are two entries to one walk: for one origin mirt.intersect_from and
    mirt.intersect_fans without indices return the same bytes and, with profiling on, count the same rays, rows stepped over and
    swept rays on the same grid -- with ordinary directions, and with 64 of them replaced by directions the bins do not cover
    (zero, a NaN component, scaled by 2^20), whose rays sweep the origin's table.

    `tests`, the rows tested, is NOT compared.  The two calls walk two cubes (g.qrows.fan and g.qrows.fans), each built by its
    call, and a build does not fix the order of the rows inside a depth shell; a row is tested when its `near` is not beyond the
    record's distance at that moment, which depends on which rows of the shell came before it.  Measured on this scene from
    this origin, 6000 directions towards U[-1, 1]^3, four builds of either cube by one library: 8480 / 8485 / 8477 / 8483 for the single fan, 8486 / 8480 / 8476
    / 8477 for the many-origin call.  `candidates` does not depend on that order: a row of shell s has near in s and its hit is
    no nearer than near, so a replacement never moves the list's end in front of the shell being walked, and every lane steps
    over whole shells up to the one its final distance falls into (9123 in all of those builds)."""
    import silhouette as sil
    tris, origins, of, dirs, want = batch_of("soup2000", 1)
    swept = dirs.copy()
    ordinary = np.flatnonzero((np.abs(dirs).max(axis=1) >= 0.5) & (np.abs(dirs).max(axis=1) < 1e3))
    odd = np.random.default_rng(13).permutation(ordinary)[:64]
    swept[odd[0::3]] = 0
    swept[odd[1::3], 1] = np.float32("nan")
    swept[odd[2::3]] = dirs[odd[2::3]] * np.float32(2.0 ** 20)
    assert not sil.outside_the_fan_window(dirs).any() and int(sil.outside_the_fan_window(swept).sum()) == 64
    mirt.set_profiling(True)
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        for what, d, nswept in (("ordinary directions", dirs, 0), ("64 swept directions", swept, 64)):
            one = mirt.intersect_from(origins[0], d)
            st1 = mirt.fan_stats()
            many = mirt.intersect_fans(origins, None, d)
            stn = mirt.fan_stats()
            assert one.tobytes() == many.tobytes(), what
            assert st1["mode_used"] == stn["mode_used"] == mirt.QUERY_BINNED, (what, st1, stn)
            for key in ("shadow_rays", "candidates", "fallback_records", "cube_bins", "shells"):
                assert st1[key] == stn[key], (what, key, st1, stn)
            assert st1["shadow_rays"] == len(d) and st1["fallback_records"] == nswept and 0 < st1["tests"] <= st1["candidates"], (what, st1)
            assert 0 < stn["tests"] <= stn["candidates"], (what, stn)
            if nswept == 0:
                same_hits(one, want, what)
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
        mirt.set_profiling(False)


# ---- 7. caches -------------------------------------------------------------------------------------------------------------------------

def test_caches(oracle):
    tris, origins, of, dirs, want = batch_of("soup2000", 5)
    mirt.scene_upload(tris)                                                 # (a new scene version: nothing is held)
    got, st = fans(origins, of, dirs, mirt.QUERY_BINNED)
    assert st["cube_source"] == 1, st
    got, st = fans(origins, of, dirs, mirt.QUERY_BINNED)
    assert st["cube_source"] == 2, st
    same_hits(got, want, "kept cube")
    got, st = fans(origins, of[:64], dirs[:64], mirt.QUERY_AUTO)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2, st
    same_hits(got, want[:64], "auto, cube held")
    # the order of the origins is part of the key
    got, st = fans(origins[::-1], (4 - of).astype(np.int32), dirs, mirt.QUERY_BINNED)
    assert st["cube_source"] == 1, st
    same_hits(got, want, "origins in reverse order")
    # the scene moves: the cube is built again, and the results follow the scene
    eye = np.eye(3, dtype=np.float32).ravel()
    mirt.scene_transform(0, len(tris), eye, (0.0625, 0.0, 0.0))
    got, st = fans(origins[::-1], (4 - of).astype(np.int32), dirs, mirt.QUERY_BINNED)
    assert st["cube_source"] == 1, st
    moved = reference(origins, of, dirs)
    same_hits(got, moved, "after scene_transform")
    assert not np.array_equal(moved["index"], want["index"])
    mirt.scene_upload(tris)

    # a single-origin fan before and after: its cube is kept, the many-origin call evicts nothing of it (nor the reverse)
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        one = mirt.intersect_from(INSIDE, dirs)
        assert mirt.fan_stats()["cube_source"] == 1
        got = mirt.intersect_fans(origins, of, dirs)
        assert mirt.fan_stats()["cube_source"] == 1
        same_hits(got, want, "between two single fans")
        assert mirt.intersect_from(INSIDE, dirs).tobytes() == one.tobytes()
        assert mirt.fan_stats()["cube_source"] == 2
        mirt.intersect_fans(origins, of, dirs)
        assert mirt.fan_stats()["cube_source"] == 2

        # the shadow maps of the scene's own lights: DirectLight's cube is read, not rebuilt, and left as it was
        recs = want[want["index"] >= 0]
        lit = mirt.direct_light(recs, LIGHTS)
        qs = mirt.query_stats()
        assert qs["mode_used"] == mirt.QUERY_BINNED and qs["cube_source"] == 1, qs
        lpos = np.ascontiguousarray(LIGHTS[:, :3])
        lof = (of % 2).astype(np.int32)
        got = mirt.intersect_fans(lpos, lof, dirs)
        st = mirt.fan_stats()
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 4 and st["cube_bins"] == qs["cube_bins"] and st["shells"] == qs["shells"], st
        same_hits(got, reference(lpos, lof, dirs), "through DirectLight's cube")
        assert mirt.query_stats() == qs
        again = mirt.direct_light(recs, LIGHTS)
        assert mirt.query_stats()["cube_source"] == 2
        assert np.array_equal(again.view(np.uint32), lit.view(np.uint32))
        mirt.intersect_fans(origins, of, dirs)
        assert mirt.fan_stats()["cube_source"] == 2                          # ... and the call's own cube is still held

        # between two binned frames of a standing view the kept camera pass survives the call
        view = mirt.make_view((0, 0, -2.5), oracle.rot_from_yaw(0.1, 1.0), 120.0, 160, 120)
        frames = [mirt.raytrace(view, LIGHTS[:1], mode=mirt.RT_BINNED) for _ in range(4)]
        frames = frames[2:]
        assert frames[1]["stats"]["mode_used"] == mirt.RT_BINNED and frames[1]["stats"]["bins_reused"] == 1, frames[1]["stats"]
        stats0 = mirt.stats()
        got = mirt.intersect_fans(origins + np.float32(0.03125), of, dirs)
        assert mirt.fan_stats()["cube_source"] == 1
        assert mirt.stats() == stats0 and mirt.query_stats()["cube_source"] == 2      # the call touches neither
        after = mirt.raytrace(view, LIGHTS[:1], mode=mirt.RT_BINNED)
        assert after["stats"]["bins_reused"] == 1, after["stats"]
        assert np.array_equal(after["xrgb"], frames[1]["xrgb"])
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


def test_auto_rule():
    """AUTO: the single fan's rule and more than MIRT_QUERY_WAVE_RAYS (4096) rays -- below that the brute path answers a wave per ray
    and was measured ahead of every build (profiles/ray_query_bench.txt, fans) --, or the cubes held."""
    tris, origins, of, dirs, want = batch_of("soup2000", 5)
    assert len(dirs) > 4096
    got, st = fans(origins, of[:4096], dirs[:4096], mirt.QUERY_AUTO)
    assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0, st
    same_hits(got, want[:4096], "auto, 4096 rays")
    got, st = fans(origins, of[:4097], dirs[:4097], mirt.QUERY_AUTO)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 1, st
    same_hits(got, want[:4097], "auto, 4097 rays")
    got, st = fans(origins, of[:64], dirs[:64], mirt.QUERY_AUTO)            # the cube is held now
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2, st
    same_hits(got, want[:64], "auto, 64 rays, cube held")
    # 33 origins: both ranges' cubes are held afterwards (a cube per pass), so a small call is "held" too and builds nothing
    tris, origins, of, dirs, want = batch_of("soup2000", 33)
    got, st = fans(origins, of, dirs, mirt.QUERY_AUTO)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 1, st
    got, st = fans(origins, of[:64], dirs[:64], mirt.QUERY_AUTO)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2, st
    same_hits(got, want[:64], "auto, 33 origins, 64 rays, cubes held")
    got, st = fans(origins, of, dirs, mirt.QUERY_BINNED)
    assert st["cube_source"] == 2, st
    same_hits(got, want, "33 origins again, cubes held")


# ---- 8. frames in flight ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_flight", [1, 2, 3, 4])
def test_frames_in_flight(in_flight):
    calls = [batch_of("soup2000", K)[1:] for K in (33, 5, 2, 32)[:in_flight]]
    bufs = []
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        mirt.set_frames_in_flight(in_flight)
        for rnd in range(2):                                                # twice: the second round meets cubes other streams left
            for origins, of, dirs, want in calls:
                d = to_device(of), to_device(dirs), to_device(mirt.fresh_hits(len(dirs)))
                bufs.append((d, want))
                mirt.intersect_fans_device(origins, d[0].ptr, d[1].ptr, len(dirs), d[2].ptr)
        mirt.sync()
        for i, (d, want) in enumerate(bufs):
            same_hits(d[2].read().view(mirt.HIT_DTYPE).reshape(-1), want, "call %d with %d in flight" % (i, in_flight))
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
        mirt.set_frames_in_flight(1)
        for d, _ in bufs:
            for x in d:
                x.free()


# ---- 9. silhouettes and bin borders, three origins in one call ----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["shell", "walls", "soup150", "shell @ far", "needles @ far"])
def test_silhouette_probes_from_three_origins(oracle, name):
    import silhouette as sil
    tris, targets, crossings, scale = sil.scene_of(oracle, name)
    mirt.scene_upload(tris)
    named = sil.origins_of(tris, scale, sil.offset_of(name))
    origins = np.ascontiguousarray(np.array(list(named.values()), np.float32))
    p = [sil.probes(tris, O, targets, crossings) for O in origins]
    assert all(len(q) > 3000 for q in p)
    of = np.concatenate([np.full(len(q), k, np.int32) for k, q in enumerate(p)])
    dirs = np.concatenate([q["dir"] for q in p]).astype(np.float32)
    order = np.random.default_rng(1).permutation(len(of))
    of, dirs = np.ascontiguousarray(of[order]), np.ascontiguousarray(dirs[order])
    want = reference(origins, of, dirs)
    assert 0.2 <= (want["index"] >= 0).mean() <= 0.999
    mirt.set_profiling(True)
    try:
        got, st = fans(origins, of, dirs, mirt.QUERY_BINNED)
    finally:
        mirt.set_profiling(False)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["shadow_rays"] == len(dirs), st
    assert st["fallback_records"] == int(sil.outside_the_fan_window(dirs).sum()), st
    bad = np.flatnonzero((got.view(np.uint8).reshape(-1, 20) != want.view(np.uint8).reshape(-1, 20)).any(axis=1))
    for q in bad[:6]:                                                       # (the first failures in full, as test_gpu_silhouette_probes.py)
        k = of[q]
        src = order[q] - sum(len(x) for x in p[:k])
        print("ray %d from origin %d: got %r, want %r\n  %s" % (q, k, got[q].tolist(), want[q].tolist(), sil.describe(p[k][src], tris, origins[k])))
    same_hits(got, want, "%s: binned vs brute force, three origins at once" % name)
    same_hits(fans(origins, of, dirs, mirt.QUERY_BINNED)[0], want, "%s: the plain instantiation" % name)
    same_hits(fans(origins, of, dirs, mirt.QUERY_BRUTE)[0], want, "%s: the brute path" % name)


# ---- 10. arguments ------------------------------------------------------------------------------------------------------------------

def test_argument_validation():
    lib = mirt.load()
    origins = np.zeros((2, 3), np.float32)
    of = np.array([0, 1, 1, 0], np.int32)
    dirs, hits = np.ones((4, 3), np.float32), mirt.fresh_hits(4)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    mirt.scene_upload(mirt.scene_cornell())
    for f in (lib.mirt_intersect_fans, lib.mirt_intersect_fans_device):
        # (the device form is given host pointers here: every one of these calls returns before anything touches the device)
        assert f(p(origins), -1, p(of), p(dirs), 4, p(hits)) == INVALID and b"origin count -1 is negative" in lib.mirt_last_error()
        assert f(p(origins), 2, p(of), p(dirs), -1, p(hits)) == INVALID and b"direction count -1 is negative" in lib.mirt_last_error()
        assert f(p(origins), 2, p(of), None, 4, p(hits)) == INVALID and f(p(origins), 2, p(of), p(dirs), 4, None) == INVALID
        assert b"direction arrays must not be NULL" in lib.mirt_last_error()
        assert f(None, 2, p(of), p(dirs), 4, p(hits)) == INVALID and b"origins must not be NULL" in lib.mirt_last_error()
        assert f(p(origins), 0, p(of), p(dirs), 4, p(hits)) == INVALID and f(None, 0, None, p(dirs), 4, p(hits)) == INVALID
        assert b"no origin" in lib.mirt_last_error()
        assert f(p(origins), 2, None, p(dirs), 4, p(hits)) == INVALID and f(p(origins), 2, None, None, 0, None) == INVALID
        assert b"origin_of may be NULL only for a single origin" in lib.mirt_last_error()
        # nrays == 0 succeeds and does nothing, NULL arrays and an empty origin list included
        assert f(p(origins), 2, p(of), None, 0, None) == 0 and f(None, 0, None, None, 0, None) == 0 and f(p(origins), 1, None, None, 0, None) == 0
    assert hits.tobytes() == mirt.fresh_hits(4).tobytes()
    assert mirt.intersect_fans(origins, np.zeros(0, np.int32), np.zeros((0, 3), np.float32)).shape == (0,)


def test_no_scene():
    mirt.shutdown()
    mirt.init(0)
    origins = np.zeros((2, 3), np.float32)
    with pytest.raises(mirt.MirtError, match="no scene uploaded"):
        mirt.intersect_fans(origins, np.array([0, 1], np.int32), np.ones((2, 3), np.float32))
    lib = mirt.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    # the argument checks come before the scene's: an index outside the list, a NULL origin_of for two origins
    assert lib.mirt_intersect_fans(p(origins), 2, p(np.array([0, 2], np.int32)), p(np.ones((2, 3), np.float32)), 2, p(mirt.fresh_hits(2))) == INVALID
    assert lib.mirt_intersect_fans_device(p(origins), 2, None, p(origins), 2, p(origins)) == INVALID
    assert lib.mirt_intersect_fans_device(None, 0, None, None, 0, None) == 0
    st = mirt.fan_stats()
    assert st["mode_used"] == 0 and st["cube_source"] == 0
