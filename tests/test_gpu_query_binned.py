"""DirectLight queries through the light-cube bins (mirt_set_query_mode, k_query_direct_light_binned): the binned walk against the
brute-force kernel and the CPU oracle's DirectLight, bit for bit and for every record; that the bins are really walked; the
queries' cube cache and the frame path's cube; streams; and what MIRT_QUERY_AUTO chooses.

Scenes, ray batches and comparison helpers are those of test_gpu_ray_query.py (query_helpers.py).  The records are closest hits of mirt.intersect
plus records of the caller's own kind: misses, an index one past the scene, positions the cube's ray family does not cover (3e19,
NaN, inf, the light itself), positions behind an occluder, and positions at L + t d for d along the axes, the face diagonals and
the cube diagonals -- the face ties and bin borders of cube_bin_of.  Lights sit on dyadic coordinates so that those ties are exact."""
import ctypes as C

import numpy as np
import pytest

import mirt
import query_helpers as rq
from devbuf import hip_fill, to_device

pytestmark = pytest.mark.gpu

# the first light lies inside every scene's box ([-1, 1]^3), so its records surround it
LIGHTS = np.array([[0, -0.5, -0.75, 1, 1, 1, 14], [0.5, 0.25, -0.875, 1, 0.5, 0.25, 6], [-0.625, -0.25, 0.125, 0.25, 1, 0.5, 9]], np.float32)
SCENES = ("soup2000", "cornell", "cornell x 2", "one")
NRAYS = 2048
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_query_mode(mirt.QUERY_AUTO)
    mirt.set_profiling(False)
    mirt.set_soft_shadows(1)
    mirt.set_frames_in_flight(1)
    mirt.shutdown()


def scene(name):
    if name == "cornell x 2":
        return np.concatenate([mirt.scene_cornell(), mirt.scene_cornell()]), 0.9, 3.0
    return rq.scene_of(name)


def directions():
    """Axes, face diagonals (+-1, +-1, 0) in the three planes, cube diagonals, and steps that land on bin borders of every grid."""
    d = []
    for ax in range(3):
        for s in (1, -1):
            v = [0, 0, 0]; v[ax] = s
            d.append(v)
    for a, b in ((0, 1), (1, 2), (0, 2)):
        for sa in (1, -1):
            for sb in (1, -1):
                v = [0, 0, 0]; v[a], v[b] = sa, sb
                d.append(v)
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                d.append([sx, sy, sz])
    for ax in range(3):                                      # u or v = +-1/2, +-1/4, 0: a bin border on grids of 64, 128 and 256
        for s in (1, -1):
            for u, v in ((0.5, 0.25), (-0.25, 0.5), (0.0, -0.5), (1.0, 0.5), (-1.0, -1.0)):
                w = [0.0, 0.0, 0.0]; w[ax], w[(ax + 1) % 3], w[(ax + 2) % 3] = s, u, v
                d.append(w)
    return np.array(d, np.float32)


def build_records(tris, hits, lights):
    """The closest-hit records `hits` plus the caller's own kinds.  Returns (records, number that fall back to the full table):
    the records whose index lies inside the scene and whose position is not finite, 3e19, or a light's position."""
    n = len(tris)
    rng = np.random.default_rng(3)
    L = np.asarray(lights, np.float32).reshape(-1, 7)[:, 0:3]
    base = hits.copy()
    hit_ids = np.flatnonzero(base["index"] >= 0)
    base["index"][5::97] = n                                 # one past the end, among the hits and the misses
    parts = [base]
    # behind an occluder: past the hit point as seen from each light (the triangle the record names shadows it)
    for k in range(len(L)):
        src = base[rng.choice(hit_ids, 160)]
        src = src[(src["index"] >= 0) & (src["index"] < n)]
        rec = src.copy()
        rec["position"] = (L[k] + np.float32(1.625) * (src["position"] - L[k])).astype(np.float32)
        parts.append(rec)
    # L + t d
    dirs = directions()
    for k in range(len(L)):
        for t in (np.float32(0.5), np.float32(1.0), np.float32(0.0078125)):
            rec = mirt.fresh_hits(len(dirs))
            rec["position"] = L[k] + t * dirs
            rec["index"] = rng.integers(0, n, len(dirs))
            rec["distance"] = 1.0
            parts.append(rec)
    # what the cube's ray family does not cover
    odd = base[rng.choice(hit_ids, 96)].copy()
    odd = odd[(odd["index"] >= 0) & (odd["index"] < n)]
    for i in range(len(odd)):
        kind = i % 6
        if kind == 0:
            odd["position"][i] = np.float32(3e19)
        elif kind == 1:
            odd["position"][i][i % 3] = np.float32(3e19)
        elif kind == 2:
            odd["position"][i][i % 3] = np.float32("nan")
        elif kind == 3:
            odd["position"][i][i % 3] = np.float32("inf") * (1 if i % 2 else -1)
        elif kind == 4:
            odd["position"][i] = np.float32("nan")
        else:
            odd["position"][i] = L[i % len(L)]
    parts.append(odd)
    recs = np.concatenate(parts)
    recs = recs[rng.permutation(len(recs))]                  # scattered, so that waves hold every kind
    return np.ascontiguousarray(recs), len(odd)


def faces_of(recs, Lk, n):
    """The cube face (0 .. 5, as cube_bin_of numbers them) of each record's shadow ray for the light at Lk; -1 where there is none."""
    d = (Lk - recs["position"]).astype(np.float32)
    ok = np.isfinite(d).all(axis=1) & (np.abs(d).max(axis=1) > 0) & (np.abs(d).max(axis=1) < 1e18) & (recs["index"] >= 0) & (recs["index"] < n)
    a = np.abs(d)
    k = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    sgn = d[np.arange(len(d)), k]
    return np.where(ok, 2 * k + (sgn < 0), -1)


def shadow_states(oracle, tris, recs, Lk):
    """Per record with a face: whether the oracle's ClosestIntersection from the light towards it ends before 0.99 r (:310-313)."""
    n = len(tris)
    face = faces_of(recs, Lk, n)
    occluded = np.zeros(len(recs), bool)
    for i in np.flatnonzero(face >= 0):
        d = (Lk - recs["position"][i]).astype(np.float32)
        r = np.float32(np.sqrt(np.float32((d * d).sum())))
        rdir = (d / r).astype(np.float32)
        _, _, dist, ix = oracle.closest_intersection(tris, Lk, -rdir)
        occluded[i] = ix >= 0 and dist < r * np.float32(0.99)
    return face, occluded


def check_coverage(oracle, tris, recs, lights):
    """All six faces, and at least 100 occluded and 100 lit records per light -- from the oracle and numpy alone."""
    counts = []
    for l in np.asarray(lights, np.float32).reshape(-1, 7):
        face, occ = shadow_states(oracle, tris, recs, l[0:3])
        assert set(face[face >= 0].tolist()) == set(range(6)), sorted(set(face.tolist()))
        n_occ, n_lit = int(occ.sum()), int(((face >= 0) & ~occ).sum())
        counts.append((n_occ, n_lit))
        assert n_occ >= 100 and n_lit >= 100, counts
    return counts


def case(oracle, name):
    """Scene, records and the oracle's results for 1, 2 and 3 lights and 2 lights x 4 soft-shadow samples: computed once."""
    if name not in _cache:
        tris, a, b = scene(name)
        rays = rq.make_batch(NRAYS, a, b)
        mirt.scene_upload(tris)
        hits = mirt.intersect(rays)
        rq.same_hits(hits[:256], rq.oracle_intersect(oracle, tris, rays[:256]), name)
        recs, nodd = build_records(tris, hits, LIGHTS)
        assert 1024 <= len(recs) <= 4096
        jit = rq.jitter(oracle, LIGHTS[:2], 4)
        want = {nl: rq.oracle_direct_light(oracle, tris, recs, LIGHTS[:nl]) for nl in (1, 2, 3)}
        want["soft"] = rq.oracle_direct_light(oracle, tris, recs, LIGHTS[:2], samples=4, jitter=jit)
        for v in want.values():
            v.setflags(write=False)
        _cache[name] = (tris, recs, nodd, jit, want)
    return _cache[name]


def light_query(recs, lights, mode):
    mirt.set_query_mode(mode)
    try:
        out = mirt.direct_light(recs, lights)
        return out, mirt.query_stats()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


# ---- binned == brute == oracle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_binned_equals_brute_equals_oracle(oracle, name):
    tris, recs, nodd, jit, want = case(oracle, name)
    n = len(tris)
    print(name, "records", len(recs), "(occluded, lit) per light", check_coverage(oracle, tris, recs, LIGHTS))
    mirt.scene_upload(tris)
    outside = (recs["index"] < 0) | (recs["index"] >= n)
    assert outside.sum() > 20 and (recs["index"] == n).any() and (recs["index"] < 0).any()
    for nl in (1, 2, 3):
        brute, sb = light_query(recs, LIGHTS[:nl], mirt.QUERY_BRUTE)
        binned, st = light_query(recs, LIGHTS[:nl], mirt.QUERY_BINNED)
        assert sb["mode_used"] == mirt.QUERY_BRUTE and sb["cube_source"] == 0
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] in (1, 2) and st["cube_bins"] in (64, 128, 256) and st["shells"] >= 1
        rq.same_bits(binned, brute, "%s, %d lights: binned vs brute" % (name, nl))
        rq.same_bits(binned, want[nl], "%s, %d lights: binned vs oracle" % (name, nl))
        assert not binned[outside].any() and binned.any()
    mirt.set_soft_shadows(4, jit)
    try:
        brute, _ = light_query(recs, LIGHTS[:2], mirt.QUERY_BRUTE)
        binned, st = light_query(recs, LIGHTS[:2], mirt.QUERY_BINNED)
    finally:
        mirt.set_soft_shadows(1)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 1      # the jittered positions: a cube of their own
    rq.same_bits(binned, brute, name + ", soft shadows: binned vs brute")
    rq.same_bits(binned, want["soft"], name + ", soft shadows: binned vs oracle")


# ---- the bins are used ------------------------------------------------------------------------------------------------------

def test_the_bins_are_used(oracle):
    tris, recs, nodd, jit, want = case(oracle, "soup2000")
    n = len(tris)
    mirt.scene_upload(tris)
    mirt.set_profiling(True)
    try:
        binned, st = light_query(recs, LIGHTS, mirt.QUERY_BINNED)
        brute, sb = light_query(recs, LIGHTS, mirt.QUERY_BRUTE)
    finally:
        mirt.set_profiling(False)
    print(st)
    valid = int(((recs["index"] >= 0) & (recs["index"] < n)).sum())
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 1
    assert st["shadow_rays"] == valid * len(LIGHTS)
    assert 0 < st["candidates"] < st["shadow_rays"] * n
    assert 0 < st["tests"] <= st["candidates"]
    assert nodd > 50 and st["fallback_records"] == nodd
    assert sb["mode_used"] == mirt.QUERY_BRUTE and sb["candidates"] == 0 and sb["cube_bins"] == 0
    rq.same_bits(binned, want[3], "profiled kernel vs oracle")
    rq.same_bits(brute, want[3], "brute vs oracle")
    # without profiling the counters stay zero
    _, st = light_query(recs, LIGHTS, mirt.QUERY_BINNED)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2 and st["candidates"] == 0 and st["shadow_rays"] == 0
    lib = mirt.load()
    assert lib.mirt_set_query_mode(3) == -3 and lib.mirt_set_query_mode(-1) == -3 and lib.mirt_get_query_stats(None) == -3


def test_fallback_sweep_counters(oracle):
    """The whole-table sweep of the records the bins do not cover adds the table's n rows to `candidates` per swept (record,
    position) and the rows a live lane tests to `tests`.  70 records (more than one wave) that name a triangle of the 65-triangle
    soup and whose position has a NaN x: rDir is NaN for either light, a NaN direction accepts nothing, so every row of both
    tables is tested."""
    tris, _, _ = rq.scene_of("soup65")
    mirt.scene_upload(tris)
    n, nrec, lights = len(tris), 70, LIGHTS[:2]
    assert n == 65
    recs = mirt.fresh_hits(nrec)
    recs["position"] = np.random.default_rng(5).uniform(-1, 1, (nrec, 3)).astype(np.float32)
    recs["position"][:, 0] = np.float32("nan")
    recs["index"] = np.arange(nrec) % n
    recs["distance"] = 1.0
    want = rq.oracle_direct_light(oracle, tris, recs, lights)
    mirt.set_profiling(True)
    try:
        got, st = light_query(recs, lights, mirt.QUERY_BINNED)
    finally:
        mirt.set_profiling(False)
    print(st)
    rq.same_bits(got, want, "NaN records vs oracle")
    assert st["mode_used"] == mirt.QUERY_BINNED, st
    assert st["shadow_rays"] == nrec * len(lights) and st["fallback_records"] == nrec, st
    assert st["candidates"] == st["tests"] == nrec * len(lights) * n, st


# ---- the cache ----------------------------------------------------------------------------------------------------------------

def test_cube_cache(oracle):
    from devbuf import DeviceArray
    tris, recs, nodd, jit, want = case(oracle, "soup2000")
    mirt.scene_upload(tris)
    out, st = light_query(recs, LIGHTS[:2], mirt.QUERY_BINNED)
    assert st["cube_source"] == 1
    rq.same_bits(out, want[2], "built")
    out, st = light_query(recs, LIGHTS[:2], mirt.QUERY_BINNED)
    assert st["cube_source"] == 2
    rq.same_bits(out, want[2], "kept")
    out, st = light_query(recs, LIGHTS[:2], mirt.QUERY_AUTO)            # a cube is held: AUTO uses it
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2
    moved = LIGHTS[:2].copy()
    moved[1, 0] += np.float32(0.125)
    out, st = light_query(recs, moved, mirt.QUERY_BINNED)
    assert st["cube_source"] == 1
    rq.same_bits(out, rq.oracle_direct_light(oracle, tris, recs, moved), "moved light")
    # a new scene forgets the cube, and the results follow the new scene
    tris2 = mirt.scene_soup(42, 2000, 0.2)
    mirt.scene_upload(tris2)
    out, st = light_query(recs, moved, mirt.QUERY_BINNED)
    assert st["cube_source"] == 1
    rq.same_bits(out, rq.oracle_direct_light(oracle, tris2, recs, moved), "new scene")
    assert not np.array_equal(out, rq.oracle_direct_light(oracle, tris, recs, moved))
    # the frame path's cube: binned frames under standing lights settle into the shared cube, and a query with those lights reads it
    W, H = 160, 120
    view = mirt.make_view((0, 0, -2.5), oracle.rot_from_yaw(0.1, 1.0), 120.0, W, H)
    x = DeviceArray((H, W), np.uint32, 0)
    try:
        frames = []
        for i in range(7):
            assert hip_fill(x, 0x11)
            mirt.raytrace_device(view, LIGHTS[:2], (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, x.ptr, W * 4)
            mirt.sync()
            frames.append(x.read())
        assert all(np.array_equal(f, frames[0]) for f in frames)
        frame_stats = mirt.stats()
        out, st = light_query(recs, LIGHTS[:2], mirt.QUERY_BINNED)
        assert st["cube_source"] == 3 and st["mode_used"] == mirt.QUERY_BINNED
        rq.same_bits(out, rq.oracle_direct_light(oracle, tris2, recs, LIGHTS[:2]), "the frame path's cube")
        out, st = light_query(recs, LIGHTS[:2], mirt.QUERY_AUTO)
        assert st["cube_source"] == 3
        assert mirt.stats() == frame_stats
        assert hip_fill(x, 0x11)
        mirt.raytrace_device(view, LIGHTS[:2], (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, x.ptr, W * 4)
        mirt.sync()
        assert np.array_equal(x.read(), frames[-1]), "the frame after the query changed"
        assert mirt.stats()["bins_reused"] == 1
    finally:
        x.free()


# ---- streams ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_flight", [1, 2, 3, 4])
def test_device_queries_between_frames_in_flight(oracle, in_flight):
    from devbuf import DeviceArray
    tris, recs, nodd, jit, want = case(oracle, "soup2000")
    mirt.scene_upload(tris)
    W, H = 160, 120
    view = mirt.make_view((0, 0, -2.5), oracle.rot_from_yaw(0.1, 1.0), 120.0, W, H)
    light_sets = [LIGHTS[:1], LIGHTS[:2], LIGHTS, LIGHTS[:2], LIGHTS[:1], LIGHTS]
    sync_want = {len(l): light_query(recs, l, mirt.QUERY_BINNED)[0] for l in light_sets}
    for nl, w in sync_want.items():
        rq.same_bits(w, want[nl], "synchronous, %d lights" % nl)
    want_frame = mirt.raytrace(view, LIGHTS[:1], mode=mirt.RT_BRUTE)["xrgb"]
    d_hits = to_device(recs)
    outs, planes = [], []
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        mirt.set_frames_in_flight(in_flight)
        for l in light_sets:
            d_rgb, x = DeviceArray((len(recs), 3), np.float32, 0x11), DeviceArray((H, W), np.uint32, 0)
            outs.append(d_rgb); planes.append(x)
            mirt.raytrace_device(view, LIGHTS[:1], (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, x.ptr, W * 4)
            mirt.direct_light_device(d_hits.ptr, len(recs), l, d_rgb.ptr)
        mirt.sync()
        for i, l in enumerate(light_sets):
            rq.same_bits(outs[i].read(), sync_want[len(l)], "query %d of %d in flight" % (i, in_flight))
            assert np.array_equal(planes[i].read()[1:-1, 1:-1], want_frame[1:-1, 1:-1]), "frame %d" % i
        # a standing view: every stream holds its pass by now; queries between its frames leave the passes alone
        x = planes[0]
        for i in range(2 * in_flight):
            assert hip_fill(x, 0x11)
            mirt.raytrace_device(view, LIGHTS[:1], (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, x.ptr, W * 4)
            st = mirt.stats()
            assert st["mode_used"] == mirt.RT_BINNED and st["bins_reused"] == 1, (i, st)
            assert np.array_equal(x.read()[1:-1, 1:-1], want_frame[1:-1, 1:-1]), "standing frame %d" % i
            mirt.direct_light_device(d_hits.ptr, len(recs), light_sets[i % len(light_sets)], outs[0].ptr)
            assert mirt.query_stats()["mode_used"] == mirt.QUERY_BINNED
            rq.same_bits(outs[0].read(), sync_want[len(light_sets[i % len(light_sets)])], "standing query %d" % i)
            assert mirt.stats() == st
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
        mirt.set_frames_in_flight(1)
        for d in outs + planes + [d_hits]:
            d.free()


# ---- AUTO ---------------------------------------------------------------------------------------------------------------------

def test_auto_follows_the_frame_paths_rule(oracle):
    tris, recs, nodd, jit, want = case(oracle, "soup2000")
    mirt.scene_upload(tris)                                   # (a new scene version: no cube is held)
    small = recs[:1024]
    out, st = light_query(small, LIGHTS[:1], mirt.QUERY_AUTO)  # 1024 x 1 x 2000 = 2e6: brute force, as before
    assert st["mode_used"] == mirt.QUERY_BRUTE and st["cube_source"] == 0
    rq.same_bits(out, want[1][:1024], "small call")
    big = np.concatenate([recs] * 3)                           # > 6667 records x 3 x 2000 >= 4e7
    assert len(big) * 3 * len(tris) >= 40000000
    out, st = light_query(big, LIGHTS, mirt.QUERY_AUTO)
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 1
    rq.same_bits(out, np.concatenate([want[3]] * 3), "large call")
    out, st = light_query(small, LIGHTS, mirt.QUERY_AUTO)      # the cube is held now: the small call uses it
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2
    rq.same_bits(out, want[3][:1024], "small call, cube held")
    # a light outside the filter's range: the frame path would not bin, nor does a query under BINNED
    far = LIGHTS[:1].copy()
    far[0, 0] = np.float32(3e8)
    out, st = light_query(small, far, mirt.QUERY_BINNED)
    assert st["mode_used"] == mirt.QUERY_BRUTE
    rq.same_bits(out, rq.oracle_direct_light(oracle, tris, small, far), "light out of range")


# ---- the three users of a stream's light scratch set, in turn -------------------------------------------------------------

_evict = {}


def _evict_case(oracle):
    """Scene, view, 256 closest-hit records of the frame's primary rays, and the brute-force frame and colours: computed once."""
    if not _evict:
        from devbuf import DeviceArray
        tris = mirt.scene_soup(17, 2500, 0.08)
        W, H, cam, focal = 160, 96, (0.0, 0.0, -2.5), 120.0
        rot = oracle.rot_from_yaw(0.1, 1.0)
        view = mirt.make_view(cam, rot, focal, W, H)
        L0, L1 = LIGHTS[0:1], LIGHTS[1:2]
        mirt.scene_upload(tris)
        hits = mirt.intersect(rq.primary_rays(oracle, cam, rot, focal, W, H))
        hit_ids = np.flatnonzero(hits["index"] >= 0)
        assert len(hit_ids) >= 256
        recs = np.ascontiguousarray(hits[hit_ids[:: len(hit_ids) // 256][:256]])
        with DeviceArray((H, W), np.uint32, 0x11) as x:
            mirt.raytrace_device(view, L0, (0.2, 0.2, 0.2), mirt.RT_BRUTE, 0, H, 0, x.ptr, W * 4)
            want_frame = x.read()
        want_rgb, sb = light_query(recs, L1, mirt.QUERY_BRUTE)
        assert sb["mode_used"] == mirt.QUERY_BRUTE and want_rgb.any()
        want_frame.setflags(write=False)
        want_rgb.setflags(write=False)
        _evict.update(tris=tris, view=view, W=W, H=H, L0=L0, L1=L1, recs=recs, want_frame=want_frame, want_rgb=want_rgb)
    return _evict


@pytest.mark.parametrize("in_flight", [1, 2])
def test_frames_and_queries_take_the_light_scratch_in_turn(oracle, in_flight):
    """A stream's light scratch set has three users that evict one another: a frame's moving-light pass, the frame path's shared
    cube build and a query's cube build.  Frames under L0 and DirectLight queries under L1 take them in turn; every frame equals
    the brute-force frame and both queries the brute-force colours, bit for bit.  One frame in flight with a sync after each call,
    and two in flight with one sync at the end.  (A kept pass belongs to a stream: with two in flight the frame that comes back to
    the first frame's stream is the third, so step 2 renders `in_flight` frames and the last of them must have kept its pass.)"""
    from devbuf import DeviceArray
    c = _evict_case(oracle)
    W, H, view, L0, L1, recs = c["W"], c["H"], c["view"], c["L0"], c["L1"], c["recs"]
    mirt.scene_upload(c["tris"])                              # (a new scene version: no pass, no cube is held)
    d_hits = to_device(recs)
    planes, outs = [], []

    def frame():
        x = DeviceArray((H, W), np.uint32, 0x11)
        planes.append(x)
        mirt.raytrace_device(view, L0, (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, x.ptr, W * 4)
        if in_flight == 1:
            mirt.sync()

    def query():
        d_rgb = DeviceArray((len(recs), 3), np.float32, 0x11)
        outs.append(d_rgb)
        mirt.direct_light_device(d_hits.ptr, len(recs), L1, d_rgb.ptr)
        st = mirt.query_stats()
        if in_flight == 1:
            mirt.sync()
        return st

    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        mirt.set_frames_in_flight(in_flight)
        frame()                                               # 1. new lights: the frame's own pass
        assert mirt.stats()["mode_used"] == mirt.RT_BINNED
        for _ in range(in_flight):                            # 2. the same frame again, back on the first frame's stream
            frame()
        assert mirt.stats()["bins_reused"] == 1
        st = query()                                          # 3. L1's cube is built in the same scratch set
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 1
        for _ in range(5):                                    # 4. the lights settle into the shared cube
            frame()
        st = query()                                          # 5. L1's cube is held
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2
        mirt.sync()
        for i, x in enumerate(planes):
            assert np.array_equal(x.read(), c["want_frame"]), "frame %d of %d in flight" % (i, in_flight)
        for i, d in enumerate(outs):
            rq.same_bits(d.read(), c["want_rgb"], "query %d of %d in flight" % (i, in_flight))
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
        mirt.set_frames_in_flight(1)
        for d in planes + outs + [d_hits]:
            d.free()
