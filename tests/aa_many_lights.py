"""Supersampled frames past 32 light positions: the frames, light sets and the per-pixel replay that test_aa_many_lights_host.py
(oracle alone) and test_gpu_aa_many_lights.py share.  A plain module like supersampling.py.

The library shades each record a pixel carries once (lights/aa_versions.hpp): a "version" begins at a hit sub-ray whose
ClosestIntersection call replaced the carried record, and is shaded once per hit sub-ray until the next version begins.  replay()
is Draw()'s sub-ray loop (raytracer.cpp:557-602) over the oracle's ClosestIntersection, counting the hit sub-rays and the versions
of every pixel; the frames are the ones of test_gpu_many_lights.py, the lights its recipe (lights_of, query_helpers.jitter)."""
import numpy as np

import query_helpers as rq

FLT_MAX = np.finfo(np.float32).max
INDIRECT = (0.2, 0.2, 0.2)

# name: scene, camera, yaw, W, H (focal = H / 2), lights x samples, supersampling
FRAMES = {
    "cornell_aa2": dict(scene="cornell", cam=(0.0, 0.0, -2.0), yaw=0.1, W=64, H=48, sets=(3, 16), aa=2),
    "cornell_aa3": dict(scene="cornell", cam=(0.0, 0.0, -2.0), yaw=0.1, W=64, H=48, sets=(3, 16), aa=3),
    "cornell_aa8": dict(scene="cornell", cam=(0.0, 0.0, -2.0), yaw=0.1, W=32, H=24, sets=(3, 11), aa=8),
    "soup_aa3": dict(scene="soup", cam=(0.1, 0.0, -2.2), yaw=0.15, W=80, H=56, sets=(3, 11), aa=3),
}
_cache = {}


def lights_of(n, seed=5):
    """n lights on dyadic coordinates inside the scenes' box; colours and powers differ (test_gpu_many_lights.lights_of)."""
    rng = np.random.default_rng(seed)
    L = np.zeros((n, 7), np.float32)
    L[:, 0:3] = np.round(rng.uniform(-0.75, 0.75, (n, 3)) * 64) / 64
    L[:, 3:6] = rng.choice(np.array([0.25, 0.5, 0.75, 1.0], np.float32), (n, 3))
    L[:, 6] = rng.integers(3, 15, n)
    L[0] = rq.LIGHTS[0]
    return L


def scene_of(oracle, name):
    key = ("scene", name)
    if key not in _cache:
        t = oracle.cornell() if name == "cornell" else oracle.soup(33, 700, 0.12)
        t.setflags(write=False)
        _cache[key] = t
    return _cache[key]


def light_set(oracle, nl, samples):
    key = ("lights", nl, samples)
    if key not in _cache:
        L = lights_of(nl)
        _cache[key] = (L, rq.jitter(oracle, L, samples, seed=9))
    return _cache[key]


def replay(oracle, tris, cam, rot, focal, W, H, aa, y0=0, y1=None):
    """Draw()'s sub-ray loop per pixel over oracle.closest_intersection: every sub-ray's call on a fresh record, merged into the
    record the pixel carries.  Returns dict(hits, versions: (H, W) counts of hit sub-rays and of versions; index, dist, pos: the
    final records as the oracle's frame stores them)."""
    y1 = H if y1 is None else y1
    rot = np.ascontiguousarray(rot, np.float32)
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 15)
    cam = np.asarray(cam, np.float32)
    f32 = np.float32
    halfW, halfH = f32(W) / f32(2), f32(H) / f32(2)
    step = f32(1) / f32(aa - 1)
    hits, versions = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    index, dist, pos = np.full((H, W), -1, np.int32), np.zeros((H, W), np.float32), np.zeros((H, W, 3), np.float32)
    d, out = np.zeros(3, np.float32), np.zeros(3, np.float32)
    for y in range(y0, y1):
        for x in range(W):
            p, dd, ix = np.zeros(3, np.float32), FLT_MAX, -1        # Update()'s reset (:335-339)
            ysub = f32(y) - f32(0.5)
            for z in range(aa):
                xsub = f32(x) - f32(0.5)
                for z2 in range(aa):
                    d[0], d[1], d[2] = xsub - halfW, ysub - halfH, f32(focal)
                    oracle.lib.mirt_oracle_mat3_mul_vec(rot, d, out)
                    # the call on a fresh record, merged as the sequential `>=` sweep on the carried one would leave it (:243): the
                    # sub-ray's closest hit takes the record when it is at least as close -- that the final records below are the
                    # oracle's frame's is checked by test_aa_many_lights_host.py
                    any_, p2, d2, i2 = oracle.closest_intersection(tris, cam, out)
                    if any_:
                        hits[y, x] += 1
                        replaced = i2 >= 0 and dd >= d2
                        if replaced:
                            p, dd, ix = p2, d2, i2
                        if replaced or versions[y, x] == 0:
                            versions[y, x] += 1
                        xsub = f32(xsub + step)                      # (:593) only after a hit
                ysub = f32(ysub + step)                              # (:596)
            index[y, x], dist[y, x], pos[y, x] = ix, dd, p
    return dict(hits=hits, versions=versions, index=index, dist=dist, pos=pos)


def frame(oracle, name):
    """The oracle's frame of FRAMES[name] and its replay, computed once, shared and left unchanged: dict(tris, L, jit, samples, aa,
    W, H, cam, rot, focal, ref: oracle.raytrace's planes and nshadow, rep: replay's)."""
    key = ("frame", name)
    if key not in _cache:
        F = FRAMES[name]
        tris = scene_of(oracle, F["scene"])
        nl, samples = F["sets"]
        L, jit = light_set(oracle, nl, samples)
        rot = oracle.rot_from_yaw(F["yaw"], 1.0)
        W, H, aa = F["W"], F["H"], F["aa"]
        ref = oracle.raytrace(tris, F["cam"], rot, H / 2.0, W, H, L, samples=samples, jitter=jit, aa=aa, threads=16)
        rep = replay(oracle, tris, F["cam"], rot, H / 2.0, W, H, aa)
        for part in (ref, rep):
            for v in part.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _cache[key] = dict(tris=tris, L=L, jit=jit, samples=samples, npos=nl * samples, aa=aa, W=W, H=H, cam=F["cam"], rot=rot, focal=H / 2.0,
                           ref=ref, rep=rep)
    return _cache[key]


def totals(rep, y0=0, y1=None):
    """(hit sub-rays, versions) of rows [y0, y1) of a replay: what mirt.supersample_stats() reports for a frame of that band."""
    return int(rep["hits"][y0:y1].sum()), int(rep["versions"][y0:y1].sum())
