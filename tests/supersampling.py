"""Supersampled frames at 2 to 8 samples: scenes, guards and the frame comparison for test_supersampling_host.py (oracle alone),
test_aa_reach.py (set-up arithmetic alone) and test_gpu_supersampling.py.  A plain module like silhouette.py.

The reference walks a pixel's sub-rays with x1 = x - 0.5f; x1 += 1.0f / (realSamples - 1) after every HIT, and y1 likewise per
sub-row (raytracer.cpp:566-596): a chain of rounded float sums.  At 4, 6, 7 and 8 samples it ends a few ulp beyond x + 0.5 for many
coordinates; ref_cases.sliver_scene builds the triangles only such a sub-ray sees.  The guards here say when a case exercises what
it is meant to: a sliver lies beyond the half pixel, the oracle's supersampled frame shows it and the plain frame does not; a sparse
soup leaves sub-rays without a hit in a fair share of the pixels."""
import numpy as np

from ref_cases import aa_overshoot, overshooting, sliver_gaps, sliver_scene

FLT_MAX = np.finfo(np.float32).max
TOL = 1e-4                                          # BASELINE.json north_star, as tests/test_gpu_parity.py

# ---- a. sub-rays past the half pixel ----------------------------------------------------------------------------------------------
SLIVER_W, SLIVER_H, SLIVER_FOCAL = 96, 72, 48.0
SLIVER_CAM = (0.0, 0.0, 0.0)
SLIVER_LIGHT = np.array([[0.0, 0.0, 0.2, 1.0, 1.0, 1.0, 14.0]], np.float32)
SLIVER_SAMPLES = (4, 6, 7, 8)
CONTROL_SAMPLES = 5                                 # no coordinate overshoots: its slivers stand where those of 4 samples stand
SLIVER_YAW = 0.3                                    # the second pose of test_aa_reach.py (set-up arithmetic only)

_cache = {}


def identity():
    r = np.zeros(9, np.float32)
    r[0] = r[4] = r[8] = 1
    return r


def sliver_case(oracle, samples, n=None, yaw=0.0):
    """The sliver scene of the 96 x 72 frame at `samples`, padded to n triangles with a soup far behind the backdrop (hidden from
    every ray, but in the view: every kernel has to reject it ray by ray or bin by bin).  Returns dict(tris, cols, rows, rot)."""
    key = ("sliver", samples, n, yaw)
    if key not in _cache:
        rot = oracle.rot_from_yaw(yaw, 1.0) if yaw else identity()
        at = 4 if samples == CONTROL_SAMPLES else samples
        tris, cols, rows = sliver_scene(samples, SLIVER_W, SLIVER_H, SLIVER_FOCAL, SLIVER_CAM, rot,
                                        overshooting(SLIVER_W, at), overshooting(SLIVER_H, at))
        if n is not None:
            pad = oracle.soup(700 + n, n - len(tris), 0.3)
            R = np.asarray(rot, np.float64).reshape(3, 3).T
            for k in range(3):                                      # along the view's axis, 6 away: depth 5 to 7 behind the backdrop's 2
                pad[:, 3 * k:3 * k + 3] = (pad[:, 3 * k:3 * k + 3].astype(np.float64) + 6.0 * R[:, 2]).astype(np.float32)
            tris = np.concatenate([tris, pad])
        tris.setflags(write=False)
        _cache[key] = dict(tris=tris, cols=cols, rows=rows, rot=rot)
    return _cache[key]


def sliver_frames(oracle, samples, n=None):
    """(supersampled, plain) oracle frames of sliver_case(samples, n): computed once, shared, left unchanged."""
    key = ("frames", samples, n)
    if key not in _cache:
        c = sliver_case(oracle, samples, n)
        a = oracle.raytrace(c["tris"], SLIVER_CAM, c["rot"], SLIVER_FOCAL, SLIVER_W, SLIVER_H, SLIVER_LIGHT, threads=16, aa=samples)
        p = oracle.raytrace(c["tris"], SLIVER_CAM, c["rot"], SLIVER_FOCAL, SLIVER_W, SLIVER_H, SLIVER_LIGHT, threads=16)
        for f in (a, p):
            for v in f.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _cache[key] = (a, p)
    return _cache[key]


def sliver_guards(case, frame, plain):
    """Per sliver: (coordinate, axis, lowest gap of its edge beyond c + 0.5 in float64 on the float32 vertices, pixels of its column
    or row the supersampled oracle frame gives it, pixels of the whole plain frame it owns)."""
    gaps = sliver_gaps(case["tris"], case["cols"], case["rows"], SLIVER_W, SLIVER_H, SLIVER_FOCAL, SLIVER_CAM, case["rot"])
    out = []
    for k, c in enumerate(case["cols"] + case["rows"]):
        axis = 0 if k < len(case["cols"]) else 1
        line = frame["index"][:, c] if axis == 0 else frame["index"][c, :]
        out.append((c, axis, gaps[k][0], int((line == 2 + k).sum()), int((plain["index"] == 2 + k).sum())))
    return out


def assert_sliver_guards(case, frame, plain, samples):
    """The case is not empty: both lists hold a last-of-16 coordinate, every sliver lies beyond the half pixel and is invisible to
    the plain frame; where the chain overshoots the supersampled frame gives it at least 20 pixels of its column or row -- and at the
    control's 5 samples none."""
    assert any(c % 16 == 15 for c in case["cols"]) and any(c % 16 == 15 for c in case["rows"]), (case["cols"], case["rows"])
    g = sliver_guards(case, frame, plain)
    assert len(g) >= 4
    for c, axis, gap, owned, owned_plain in g:
        what = "%s %d at %d samples" % ("row" if axis else "column", c, samples)
        assert gap > 0.0, "%s: the sliver starts %.3g pixels beyond the half pixel" % (what, gap)
        assert owned_plain == 0, "%s: the plain frame sees the sliver in %d pixels" % (what, owned_plain)
        if samples == CONTROL_SAMPLES:
            assert owned == 0, "%s: the control sees the sliver in %d pixels" % (what, owned)
        else:
            assert gap < float(aa_overshoot(c, samples, (SLIVER_H if axis else SLIVER_W) / 2.0)), what
            assert owned >= 20, "%s: the oracle gives the sliver %d pixels" % (what, owned)


def sliver_bands(case):
    """Three bands of the sliver frame: the first ends ON a row that carries a row sliver (its last row y1 - 1 overshoots), the third
    starts at a row that is no multiple of 8."""
    r = case["rows"][0]
    return [(0, r + 1), (r + 1, 45), (45, SLIVER_H)]


# ---- b. every sample count on every kernel ---------------------------------------------------------------------------------------
SOUP_W, SOUP_H, SOUP_FOCAL, SOUP_YAW = 96, 64, 64.0, 0.15
SOUP_CAM = (0.0, 0.0, -2.0)
TWO_LIGHTS = np.array([[0, -0.5, -0.7, 1, 1, 1, 14], [0.4, 0.3, -0.9, 0.6, 0.9, 0.3, 7]], np.float32)
# path: (mode name, triangles, lights, soup seed, triangle size).  The counts are the selection boundaries of capi/rt_frame.cpp:
# n <= 64 the tile kernel; 16 + 48 * n * (2 + lights) <= 48 KiB the LDS-resident kernel (255 with two lights, 341 with one); beyond
# it the chunked brute-force kernel.  Sizes: chosen so that sparse_share() lies between 0.2 and 0.8 at every sample count.
SOUP_PATHS = {
    "tile30": ("auto", 30, 1, 330, 1.0),
    "tile64": ("auto", 64, 2, 364, 0.7),
    "small65": ("brute", 65, 1, 365, 0.7),
    "small255": ("brute", 255, 2, 555, 0.36),
    "brute256": ("brute", 256, 2, 556, 0.36),
    "brute342": ("brute", 342, 1, 642, 0.3),
    "binned1200": ("binned", 1200, 1, 1500, 0.2),
    # RT_AUTO bins from 4e7 pixel-triangles on: this frame stays below it, so this is the chunked brute-force kernel once more,
    # chosen by RT_AUTO.  (A frame that RT_AUTO bins costs the oracle 4e7 * samples^2: AUTO_BINS below, at 2 and 3 samples.)
    "brute1200_auto": ("auto", 1200, 1, 1500, 0.2),
}
# RT_AUTO choosing the bins: 96 * 64 * 6600 = 4.06e7 pixel-triangles, 3.6e8 tests for the oracle at 3 samples
AUTO_BINS = ("auto", 6600, 1, 6900, 0.09)
AUTO_BINS_SAMPLES = (2, 3)


def _spec(path):
    return AUTO_BINS if path == "auto_bins" else SOUP_PATHS[path]


def soup_case(oracle, path):
    mode, n, nl, seed, size = _spec(path)
    key = ("soup", _spec(path)[1:])
    if key not in _cache:
        t = oracle.soup(seed, n, size)
        t.setflags(write=False)
        _cache[key] = t
    return mode, _cache[key], TWO_LIGHTS[:nl], oracle.rot_from_yaw(SOUP_YAW, 1.0)


def soup_frame(oracle, path, aa):
    """The oracle's frame of a path's soup at `aa` samples: computed once, shared (binned1200 and brute1200_auto are one scene)."""
    mode, tris, lights, rot = soup_case(oracle, path)
    key = ("soup frame", _spec(path)[1:], aa)
    if key not in _cache:
        f = oracle.raytrace(tris, SOUP_CAM, rot, SOUP_FOCAL, SOUP_W, SOUP_H, lights, threads=16, aa=aa)
        for v in f.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = f
    return _cache[key]


def sub_ray_hits(oracle, tris, cam, rot, focal, W, H, aa):
    """How many of a pixel's aa * aa sub-rays hit something, per pixel: the oracle's frame of the scene painted white, without a
    light and with indirect light 1 -- every hit adds exactly 1 to the pixel's sum, which is divided by aa * aa."""
    white = np.array(tris, np.float32)
    white[:, 12:15] = 1.0
    f = oracle.raytrace(white, cam, rot, focal, W, H, np.zeros((0, 7), np.float32), indirect=(1.0, 1.0, 1.0), threads=16, aa=aa, want=("rgb",))
    return np.rint(f["rgb"][:, :, 0].astype(np.float64) * (aa * aa)).astype(np.int64)


def sparse_share(oracle, tris, cam, rot, focal, W, H, aa):
    """Share of the pixels in which at least one sub-ray missed: they end without a hit (index -1), or with a record carried over a
    sub-ray that found nothing while x1 stood still."""
    return float((sub_ray_hits(oracle, tris, cam, rot, focal, W, H, aa) < aa * aa).mean())


def soup_share(oracle, path, aa):
    """sparse_share() of a path's soup at `aa` samples: computed once, shared like soup_frame()."""
    mode, tris, lights, rot = soup_case(oracle, path)
    key = ("soup share", _spec(path)[1:], aa)
    if key not in _cache:
        _cache[key] = sparse_share(oracle, tris, SOUP_CAM, rot, SOUP_FOCAL, SOUP_W, SOUP_H, aa)
    return _cache[key]


# ---- the comparison -----------------------------------------------------------------------------------------------------------------

def compare_frames(got, ref, W, H, aa):
    """_rt_compare's assertions (tests/test_gpu_parity.py) between a rendered frame and the oracle's: closest-hit index, distance and
    position planes, float colour bits, XRGB words and both ray counts -- got["stats"] is required; a frame rendered in bands
    brings the sums of its bands' counts."""
    assert np.array_equal(got["index"], ref["index"]), "closest-hit index differs in %d pixels" % int((got["index"] != ref["index"]).sum())
    assert np.array_equal(got["dist"].view(np.uint32), ref["dist"].view(np.uint32)), "closest-hit distance not bit-identical"
    assert np.array_equal(got["pos"].view(np.uint32), ref["pos"].view(np.uint32)), "closest-hit position not bit-identical"
    assert np.max(np.abs(got["rgb"] - ref["rgb"])) <= TOL
    assert np.array_equal(got["rgb"].view(np.uint32), ref["rgb"].view(np.uint32)), "float colours not bit-identical"
    assert np.array_equal(got["xrgb"], ref["xrgb"])
    assert got["stats"]["primary_rays"] == W * H * aa * aa
    assert got["stats"]["shadow_rays"] == ref["nshadow"]
