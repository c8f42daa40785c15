"""What the ray-query tests on the GPU (test_gpu_ray_query.py, test_gpu_query_binned.py, test_gpu_fan_query.py,
test_gpu_fans_query.py, test_gpu_occluded.py) and the call-sequence fuzzer fuzz_queries.py share: the CPU oracle's
ClosestIntersection and DirectLight per ray or record, the bit-exact comparisons, the occlusion limits and odd rays, and the
scenes, ray batches and directions they are made on.  Test plumbing only; device buffers: devbuf.py."""
import ctypes as C

import numpy as np

import mirt

# two lights on dyadic coordinates, the first inside every scene's box ([-1, 1]^3): the fans' tests and their frames
LIGHTS = np.array([[0, -0.5, -0.75, 1, 1, 1, 14], [0.5, 0.25, -0.875, 1, 0.5, 0.25, 6]], np.float32)
INSIDE = np.array([0.125, -0.0625, 0.1875], np.float32)
OUTSIDE = np.array([2.5, 0.75, -1.5], np.float32)
FLT_MAX = np.finfo(np.float32).max
INF, NAN = np.float32("inf"), np.float32("nan")
NKINDS = 8                                           # the kinds of limit limits_for cycles through
_fan_scenes = {}


# ---- the oracle, and bit-exact comparisons ---------------------------------------------------------------------------------------

def oracle_intersect(oracle, tris, rays, hits=None):
    """One oracle ClosestIntersection call per ray on its in/out record."""
    out = mirt.fresh_hits(len(rays)) if hits is None else hits.copy()
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 15)
    for i in range(len(rays)):
        _, p, d, ix = oracle.closest_intersection(tris, rays["start"][i], rays["dir"][i], pos=out["position"][i],
                                                  distance=float(out["distance"][i]), index=int(out["index"][i]))
        # a NaN distance that came back unchanged keeps the caller's bits (float -> C float -> float may quieten a payload)
        if not (np.isnan(d) and np.isnan(out["distance"][i])):
            out["distance"][i] = d
        out["position"][i], out["index"][i] = p, ix
    return out


def oracle_direct_light(oracle, tris, hits, lights, samples=1, jitter=None):
    out = np.zeros((len(hits), 3), np.float32)
    for i, h in enumerate(hits):
        if 0 <= h["index"] < len(tris):                      # outside: the reference indexes out of bounds; the library yields 0
            out[i] = oracle.direct_light(tris, h["position"], float(h["distance"]), int(h["index"]), lights, samples=samples, jitter=jitter)
    return out


def jitter(oracle, lights, samples, seed=1):
    C.CDLL(None).srand(seed)
    return np.concatenate([oracle.jitter(l[0:3], samples) for l in np.asarray(lights, np.float32).reshape(-1, 7)])


def same_hits(got, want, what=""):
    assert np.array_equal(got["index"], want["index"]), "%s: index differs for %d rays" % (what, int((got["index"] != want["index"]).sum()))
    assert np.array_equal(got["distance"].view(np.uint32), want["distance"].view(np.uint32)), "%s: distance not bit-identical" % what
    assert np.array_equal(got["position"].view(np.uint32), want["position"].view(np.uint32)), "%s: position not bit-identical" % what
    assert got.tobytes() == want.tobytes(), what


def same_bits(got, want, what=""):
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), "%s: not bit-identical" % what


# ---- scenes and rays -------------------------------------------------------------------------------------------------------------

def scene_of(name):
    """(triangles, a, b) for make_batch: starts in U[-a, a]^3, targets in U[-b, b]^3."""
    if name == "cornell":
        return mirt.scene_cornell(), 0.9, 3.0
    if name == "soup2000":
        return mirt.scene_soup(41, 2000, 0.2), 1.5, 1.0
    if name == "soup65":
        return mirt.scene_soup(5, 65, 0.5), 1.5, 1.0
    if name == "one":
        return mirt.scene_soup(9, 1, 0.8), 1.5, 0.3
    raise KeyError(name)


def make_batch(n, a, b, seed=7):
    """start ~ U[-a, a]^3, dir = target - start, target ~ U[-b, b]^3."""
    rng = np.random.default_rng(seed)
    start = rng.uniform(-a, a, (n, 3)).astype(np.float32)
    target = rng.uniform(-b, b, (n, 3)).astype(np.float32)
    return mirt.make_rays(start, (target - start).astype(np.float32))


def primary_rays(oracle, cam, rot, focal, W, H):
    """The primary rays of Draw() (raytracer.cpp:579-580): d = (x - W/2, y - H/2, focalLength), dir = cameraRot * d."""
    rays = np.zeros(W * H, mirt.RAY_DTYPE)
    rays["start"] = np.asarray(cam, np.float32)
    rot = np.ascontiguousarray(rot, np.float32)
    out = np.zeros(3, np.float32)
    for y in range(H):
        for x in range(W):
            d = np.array([np.float32(x) - np.float32(W) / np.float32(2), np.float32(y) - np.float32(H) / np.float32(2), np.float32(focal)], np.float32)
            oracle.lib.mirt_oracle_mat3_mul_vec(rot, d, out)
            rays["dir"][y * W + x] = out
    return rays


# ---- occlusion: expectations, limits and rays outside the filter's range -------------------------------------------------------------

def expected(hits, limits):
    """The reference's two steps on the oracle's (or the library's bit-identical) fresh-record results."""
    lim = np.full(len(hits), INF, np.float32) if limits is None else limits
    with np.errstate(invalid="ignore"):
        return ((hits["index"] >= 0) & (hits["distance"] < lim)).astype(np.uint8)


def limits_for(hits):
    """Per ray, cycling: +inf, FLT_MAX, d, the float above d, the float below d, 0, -1, NaN -- d the ray's own closest distance
    where it hit, else 1."""
    d = np.where(hits["index"] >= 0, hits["distance"], np.float32(1.0)).astype(np.float32)
    kind = np.arange(len(hits)) % NKINDS
    lim = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, kind == 6],
                    [INF, FLT_MAX, d, np.nextafter(d, INF), np.nextafter(d, np.float32(0)), np.float32(0), np.float32(-1)], NAN)
    return np.ascontiguousarray(lim.astype(np.float32)), kind


def odd_rays(rays):
    """A handful of rays outside the filter's range in every batch of 257 or more (every 41st ray from the 6th on): a start at
    1e9, a direction component of 1e7, a zero direction, a NaN in the start, a NaN in the direction."""
    rays = rays.copy()
    for k, i in enumerate(range(5, len(rays), 41)):
        kind = k % 5
        if kind == 0:
            rays["start"][i][k % 3] = 1e9
        elif kind == 1:
            rays["dir"][i][k % 3] = 1e7
        elif kind == 2:
            rays["dir"][i] = 0
        elif kind == 3:
            rays["start"][i][k % 3] = NAN
        else:
            rays["dir"][i][k % 3] = NAN
    return rays


# ---- origin fans: scenes and directions ------------------------------------------------------------------------------------------

def fan_scene_of(name):
    """(triangles, b), computed once: the scenes of scene_of and cornell + soup2000; directions aim at U[-b, b]^3."""
    if name not in _fan_scenes:
        if name == "cornell+soup2000":
            v = np.concatenate([mirt.scene_cornell(), mirt.scene_soup(41, 2000, 0.2)]), 1.0
        elif name == "cornell x 2":
            v = np.concatenate([mirt.scene_cornell(), mirt.scene_cornell()]), 3.0
        else:
            tris, _, b = scene_of(name)
            v = tris, b
        v[0].setflags(write=False)
        _fan_scenes[name] = v
    return _fan_scenes[name]


def seam_directions():
    """The 26 axis, face-diagonal and corner directions, and each with one component moved one ulp up or down (a zero component
    to the smallest subnormal of either sign): on, and to either side of, every face seam and face centre of cube_bin_of."""
    base = [np.array([x, y, z], np.float32) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if x or y or z]
    out = []
    for d in base:
        out.append(d)
        for c in range(3):
            for to in (np.float32("inf"), np.float32("-inf")):
                e = d.copy()
                e[c] = np.nextafter(d[c], to)
                out.append(e)
    return np.array(out, np.float32)
