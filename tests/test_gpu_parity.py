"""Parity tests proper: the HIP path, called through the C-ABI (libmirt.so), against the CPU oracle and the
reference's recorded outputs.  Bar (BASELINE.json north_star): closest-hit triangle index bit-exact, colours
within 1e-4 per channel -- in practice the kernels reproduce the float colours bit for bit, which the tests
also assert (it is what makes the 8-bit frame identical).
"""
import numpy as np
import pytest

import mirt
from mirt_oracle import DEFAULT_LIGHT

pytestmark = pytest.mark.gpu

TOL = 1e-4   # per-channel colour tolerance stated by north_star


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)          # raises MirtError (fails loudly) when libmirt.so or the GPU is missing
    yield
    mirt.shutdown()


def _rt_compare(oracle, tris, cam, rot, focal, W, H, lights, mode=mirt.RT_BRUTE, threads=16, samples=1, jitter=None, aa=1):
    ref = oracle.raytrace(tris, cam, rot, focal, W, H, lights, threads=threads, samples=samples, jitter=jitter, aa=aa)
    mirt.scene_upload(tris)
    mirt.set_soft_shadows(samples, jitter)
    mirt.set_antialiasing(aa)
    try:
        got = mirt.raytrace(mirt.make_view(cam, rot, focal, W, H), lights, mode=mode, want_intersection=True)
    finally:
        mirt.set_soft_shadows(1)
        mirt.set_antialiasing(1)
    assert np.array_equal(got["index"], ref["index"]), "closest-hit index differs in %d pixels" % int((got["index"] != ref["index"]).sum())
    # the rest of struct Intersection (raytracer.cpp:91-98): closest distance (FLT_MAX on a miss) and hit position, bit for bit
    assert np.array_equal(got["dist"].view(np.uint32), ref["dist"].view(np.uint32)), "closest-hit distance not bit-identical"
    assert np.array_equal(got["pos"].view(np.uint32), ref["pos"].view(np.uint32)), "closest-hit position not bit-identical"
    assert np.max(np.abs(got["rgb"] - ref["rgb"])) <= TOL
    assert np.array_equal(got["rgb"].view(np.uint32), ref["rgb"].view(np.uint32)), "float colours not bit-identical"
    assert np.array_equal(got["xrgb"], ref["xrgb"])
    assert got["stats"]["primary_rays"] == W * H * aa * aa
    assert got["stats"]["shadow_rays"] == ref["nshadow"]
    return got, ref


def test_rt_cornell_500_matches_reference_hashes(oracle, golden):
    """Config 1/2 at the reference's own size: the GPU frame reproduces the hashes recorded from the reference."""
    g = golden["raytracer"]
    tris = mirt.scene_cornell()
    rot = oracle.rot_from_yaw(0.0, 1.0)
    mirt.scene_upload(tris)
    view = mirt.make_view(g["cam_pos"], rot, g["focal"], 500, 500)
    lit = mirt.raytrace(view, np.array([g["light"]], np.float32), mode=mirt.RT_BRUTE)
    assert "%016x" % oracle.fnv(lit["index"]) == g["index_fnv"]
    assert "%016x" % oracle.fnv(lit["rgb"]) == g["with_light"]["rgb_fnv"]
    assert "%016x" % oracle.fnv(lit["xrgb"]) == g["with_light"]["screen_fnv"]
    unlit = mirt.raytrace(view, np.zeros((0, 7), np.float32), mode=mirt.RT_BRUTE)
    assert "%016x" % oracle.fnv(unlit["index"]) == g["index_fnv"]
    assert "%016x" % oracle.fnv(unlit["rgb"]) == g["no_light"]["rgb_fnv"]
    assert "%016x" % oracle.fnv(unlit["xrgb"]) == g["no_light"]["screen_fnv"]
    assert lit["stats"]["shadow_rays"] == 250000 and unlit["stats"]["shadow_rays"] == 0


def test_rt_cornell_1080p(oracle):
    """BASELINE config 2: Cornell box, 1920x1080, primary + shadow."""
    _rt_compare(oracle, mirt.scene_cornell(), (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 540.0, 1920, 1080, DEFAULT_LIGHT)


@pytest.mark.parametrize("yaw", [0.3, -1.1])
def test_rt_cornell_rotated_camera(oracle, yaw):
    _rt_compare(oracle, mirt.scene_cornell(), (0.2, -0.1, -2.5), oracle.rot_from_yaw(yaw, 1.0), 300.0, 640, 360, DEFAULT_LIGHT)


def test_rt_three_lights_double_count_quirk(oracle):
    """result2 += result without resetting result (raytracer.cpp:319-322) must be reproduced."""
    lights = np.array([[0, -0.5, -0.7, 1, 1, 1, 14], [0.5, 0.3, -0.9, 1, 0.5, 0.2, 6], [-0.6, -0.2, 0.1, 0.3, 0.9, 0.4, 9]], np.float32)
    _rt_compare(oracle, mirt.scene_cornell(), (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 128.0, 256, 256, lights)


@pytest.mark.parametrize("n,W,H", [(1, 64, 64), (37, 200, 120), (1500, 320, 200), (5000, 256, 144)])
def test_rt_soup_brute(oracle, n, W, H):
    """Random soups (ragged sizes: n not a multiple of the LDS chunk, W not a multiple of 64)."""
    tris = mirt.scene_soup(11 + n, n, 0.25 if n < 100 else 0.08)
    _rt_compare(oracle, tris, (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), H / 2.0, W, H, DEFAULT_LIGHT)


@pytest.mark.parametrize("n,W,H,s", [(700, 320, 200, 0.15), (5000, 333, 207, 0.08), (20000, 640, 360, 0.05)])
def test_rt_soup_binned(oracle, n, W, H, s):
    """Binned mode (screen-tile + light-cube candidate lists) must reproduce brute force bit for bit."""
    tris = mirt.scene_soup(31 + n, n, s)
    got, _ = _rt_compare(oracle, tris, (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), H / 2.0, W, H, DEFAULT_LIGHT, mode=mirt.RT_BINNED)
    assert got["stats"]["mode_used"] == mirt.RT_BINNED


def test_rt_binned_camera_inside_soup_rotated_two_lights(oracle):
    """Triangles beside and behind the camera and all around both lights (every cube face in use)."""
    tris = mirt.scene_soup(77, 6000, 0.12)
    lights = np.array([[0, -0.5, -0.7, 1, 1, 1, 14], [0.4, 0.3, 0.2, 0.6, 0.9, 0.3, 5]], np.float32)
    _rt_compare(oracle, tris, (0.1, -0.2, -0.3), oracle.rot_from_yaw(0.7, 1.0), 150.0, 400, 300, lights, mode=mirt.RT_BINNED)


def test_rt_binned_cornell(oracle):
    """Large triangles spanning many bins, exact-distance ties on shared edges (tie rule restated order-free)."""
    got, _ = _rt_compare(oracle, mirt.scene_cornell(), (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 250.0, 500, 500, DEFAULT_LIGHT, mode=mirt.RT_BINNED)
    assert got["stats"]["mode_used"] == mirt.RT_BINNED


def test_rt_binned_band(oracle):
    """A band that does not start on a tile boundary."""
    import ctypes as C
    tris = mirt.scene_soup(5, 3000, 0.1)
    mirt.scene_upload(tris)
    W, H = 200, 120
    view = mirt.make_view((0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 60.0, W, H)
    full = mirt.raytrace(view, DEFAULT_LIGHT, mode=mirt.RT_BRUTE)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), W * H * 4) == 0
    assert hip.hipMemset(d, 0, W * H * 4) == 0
    for (y0, y1) in [(0, 45), (45, 83), (83, 120)]:
        mirt.raytrace_device(view, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_BINNED, y0, y1, 0, d, W * 4)
    mirt.sync()
    out = np.zeros((H, W), np.uint32)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), d, W * H * 4, 2) == 0
    hip.hipFree(d)
    assert np.array_equal(out, full["xrgb"])


@pytest.mark.parametrize("mode", [mirt.RT_BRUTE, mirt.RT_AUTO])
def test_rt_wave_per_ray_min_t(oracle, mode):
    """Few rays, many triangles: one wave per ray, lanes over triangles, closest hit by the wavefront min-t key
    (distance bits << 32 | ~index): the `>=` tie rule and every colour must still match bit for bit."""
    tris = np.concatenate([mirt.scene_soup(41, 3000, 0.2), mirt.scene_cornell()])      # Cornell adds exact ties
    lights = np.array([[0, -0.5, -0.7, 1, 1, 1, 14], [0.3, 0.2, -0.9, 0.5, 0.7, 1.0, 8]], np.float32)
    _rt_compare(oracle, tris, (0, 0, -2), oracle.rot_from_yaw(0.1, 1.0), 24.0, 48, 40, lights, mode=mode)


# ---- soft shadows (parity unpinned: no recorded reference output) ----------------

def _jitter(oracle, lights, samples, seed=1):
    import ctypes
    ctypes.CDLL(None).srand(seed)                     # the reference never seeds: glibc's default state is srand(1)
    return np.concatenate([oracle.jitter(l[0:3], samples) for l in np.asarray(lights, np.float32).reshape(-1, 7)])


def test_rt_soft_shadows_cornell_16_samples(oracle):
    """SOFT_SHADOWS_SAMPLES = 16 jittered positions for the reference's light (raytracer.cpp:40-41,186-190,272-287)."""
    jit = _jitter(oracle, DEFAULT_LIGHT, 16)
    got, _ = _rt_compare(oracle, mirt.scene_cornell(), (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 150.0, 300, 300,
                         DEFAULT_LIGHT, mode=mirt.RT_AUTO, samples=16, jitter=jit)
    assert got["stats"]["shadow_rays"] == 16 * 300 * 300


@pytest.mark.parametrize("mode,n", [(mirt.RT_BRUTE, 90), (mirt.RT_BRUTE, 3000), (mirt.RT_BINNED, 3000)])
def test_rt_soft_shadows_two_lights(oracle, mode, n):
    """Two lights x 4 samples: result += D per sample, result2 += result per LIGHT (raytracer.cpp:319-322)."""
    lights = np.array([[0, -0.5, -0.7, 1, 1, 1, 14], [0.4, 0.3, -0.9, 0.6, 0.9, 0.3, 7]], np.float32)
    jit = _jitter(oracle, lights, 4)
    tris = mirt.scene_soup(17, n, 0.25 if n < 100 else 0.1)
    _rt_compare(oracle, tris, (0, 0, -2), oracle.rot_from_yaw(-0.2, 1.0), 110.0, 240, 200, lights, mode=mode, samples=4, jitter=jit)


# ---- supersampling (parity unpinned: no recorded reference output) ----------------

def test_rt_supersampling_cornell(oracle):
    """AA_SAMPLES = 3: nine sub-rays per pixel with the reference's carried closest-hit record and hit-only x1 advance
    (raytracer.cpp:549-599).  Cornell box: the tile-mask kernel, rectangles widened by the sub-pixel reach."""
    got, ref = _rt_compare(oracle, mirt.scene_cornell(), (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 100.0, 200, 200,
                           DEFAULT_LIGHT, mode=mirt.RT_AUTO, aa=3)
    plain = oracle.raytrace(mirt.scene_cornell(), (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 100.0, 200, 200, DEFAULT_LIGHT)
    assert not np.array_equal(ref["rgb"], plain["rgb"])                  # it does change the image


@pytest.mark.parametrize("mode,n,aa", [(mirt.RT_BRUTE, 90, 3), (mirt.RT_BRUTE, 1500, 2), (mirt.RT_BINNED, 2500, 3), (mirt.RT_AUTO, 30, 4)])
def test_rt_supersampling_all_kernels(oracle, mode, n, aa):
    """Sparse soups leave many sub-rays without a hit, which exercises the `x1 advances only after a hit` quirk and
    the carried record (a sub-ray that hits something farther still shades the nearest hit found so far)."""
    tris = mirt.scene_soup(55 + n, n, 0.25 if n < 100 else 0.08)
    lights = np.array([[0, -0.5, -0.7, 1, 1, 1, 14], [0.4, 0.3, -0.9, 0.6, 0.9, 0.3, 7]], np.float32)
    _rt_compare(oracle, tris, (0, 0, -2), oracle.rot_from_yaw(0.15, 1.0), 70.0, 150, 110, lights, mode=mode, aa=aa)


def test_rt_supersampling_with_soft_shadows(oracle):
    jit = _jitter(oracle, DEFAULT_LIGHT, 4)
    _rt_compare(oracle, mirt.scene_cornell(), (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 60.0, 120, 120, DEFAULT_LIGHT,
                mode=mirt.RT_AUTO, samples=4, jitter=jit, aa=3)


def test_rt_soft_shadows_limits():
    with pytest.raises(mirt.MirtError):
        mirt.set_soft_shadows(16, np.zeros((8, 3), np.float32))          # fewer positions than samples
    mirt.set_soft_shadows(16, np.zeros((32, 3), np.float32))
    try:
        mirt.scene_upload(mirt.scene_cornell())
        view = mirt.make_view((0, 0, -2), np.eye(3, dtype=np.float32).ravel(), 16.0, 32, 32)
        with pytest.raises(mirt.MirtError, match="exceed"):
            mirt.raytrace(view, np.tile(DEFAULT_LIGHT, (3, 1)))          # 3 lights x 16 samples > 32 positions
    finally:
        mirt.set_soft_shadows(1)


def test_rt_miss_everywhere(oracle):
    """Camera looking away: no hit anywhere -> index -1, black, zero shadow rays."""
    tris = mirt.scene_cornell()
    got, _ = _rt_compare(oracle, tris, (0, 0, -2), oracle.rot_from_yaw(np.pi, 1.0), 100.0, 128, 96, DEFAULT_LIGHT)
    assert (got["index"] == -1).all() and not got["xrgb"].any()


def test_rt_border_left_untouched(oracle):
    tris = mirt.scene_cornell()
    mirt.scene_upload(tris)
    W = H = 96
    canvas = np.full((H, W + 5), 0xABCDEF01, np.uint32)          # pitch wider than the row
    view = mirt.make_view((0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 48.0, W, H)
    mirt.raytrace(view, DEFAULT_LIGHT, xrgb=canvas[:, :W], want_rgb=False, want_index=False)
    assert (canvas[0] == 0xABCDEF01).all() and (canvas[-1] == 0xABCDEF01).all()
    assert (canvas[:, 0] == 0xABCDEF01).all() and (canvas[:, W - 1:] == 0xABCDEF01).all()
    ref = oracle.raytrace(tris, (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 48.0, W, H, DEFAULT_LIGHT)
    assert np.array_equal(canvas[1:-1, 1:W - 1], ref["xrgb"][1:-1, 1:-1])


def test_rt_degenerate_inputs(oracle):
    """Zero-area and edge-on triangles divide by zero in the reference (NaN/Inf always reject)."""
    tris = mirt.scene_soup(5, 64, 0.3)
    tris[3, 3:6] = tris[3, 0:3]                      # v1 == v0  -> zero area
    tris[7, 6:9] = tris[7, 3:6]                      # v2 == v1
    tris[9, 0:9] = np.tile(tris[9, 0:3], 3)          # a point
    _rt_compare(oracle, tris, (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 80.0, 160, 160, DEFAULT_LIGHT)


def test_rt_huge_coordinates_take_exact_path(oracle):
    """Operands beyond the pre-reject filter's proven range switch the kernel to the exact-only path."""
    tris = mirt.scene_soup(6, 40, 0.3)
    tris[5, 0:9] *= 1.0e12
    _rt_compare(oracle, tris, (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 64.0, 128, 128, DEFAULT_LIGHT)


def test_rt_band_rendering_matches_full_frame(oracle):
    """Rows [y0,y1) rendered as separate bands (what each GPU does when the frame is sharded) are byte-identical."""
    import ctypes as C
    tris = mirt.scene_soup(3, 300, 0.2)
    mirt.scene_upload(tris)
    W, H = 200, 120
    view = mirt.make_view((0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 60.0, W, H)
    full = mirt.raytrace(view, DEFAULT_LIGHT)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), W * H * 4) == 0
    assert hip.hipMemset(d, 0, W * H * 4) == 0
    for (y0, y1) in [(0, 50), (50, 51), (51, 120)]:
        mirt.raytrace_device(view, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_BRUTE, y0, y1, 0, d, W * 4)
    mirt.sync()
    out = np.zeros((H, W), np.uint32)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), d, W * H * 4, 2) == 0
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipFree(d)
    assert np.array_equal(out, full["xrgb"])


# ---- rasteriser --------------------------------------------------------------------------------------

def _raster_compare(oracle, tris, cam, rot, focal, W, H, lights, cull_flags=3):
    view = mirt.make_view(cam, rot, focal, W, H)
    culled = mirt.cull(tris, view, cull_flags)
    assert np.array_equal(culled, oracle.cull(tris, cam, rot, focal, W, H, cull_flags))
    ref = oracle.rasterise(tris, culled, cam, rot, focal, W, H, lights)
    mirt.scene_upload(tris, culled)
    got = mirt.rasterise(view, lights)
    assert np.array_equal(got["index"], ref["index"]), "owner triangle differs in %d pixels" % int((got["index"] != ref["index"]).sum())
    assert np.array_equal(got["depth"].view(np.uint32), ref["depth"].view(np.uint32))
    assert np.max(np.abs(got["rgb"] - ref["rgb"])) <= TOL
    assert np.array_equal(got["rgb"].view(np.uint32), ref["rgb"].view(np.uint32))
    assert np.array_equal(got["xrgb"], ref["xrgb"])
    return got, ref


def test_raster_cornell_500_matches_reference_hashes(oracle, golden):
    g = golden["rasteriser"]
    tris = mirt.scene_cornell()
    rot = oracle.rot_from_yaw(0.0, g["rot11"])
    got, _ = _raster_compare(oracle, tris, g["cam_pos"], rot, g["focal"], 500, 500, np.array([g["light"]], np.float32))
    assert int((got["depth"] > 0).sum()) == g["covered"]
    assert "%016x" % oracle.fnv(got["depth"]) == g["depth_fnv"]
    assert "%016x" % oracle.fnv(got["rgb"]) == g["rgb_fnv"]


def test_raster_cornell_4k(oracle):
    """BASELINE config 4: Cornell box, 3840x2160, camera (0,0,-3), cameraRot[1][1] = 1.01, focal = H."""
    _raster_compare(oracle, mirt.scene_cornell(), (0, 0, -3), oracle.rot_from_yaw(0.0, 1.01), 2160.0, 3840, 2160, DEFAULT_LIGHT)


@pytest.mark.parametrize("yaw,cam", [(0.4, (0.3, 0.1, -2.6)), (-0.7, (-0.5, 0.2, -2.2))])
def test_raster_cornell_rotated(oracle, yaw, cam):
    _raster_compare(oracle, mirt.scene_cornell(), cam, oracle.rot_from_yaw(yaw, 1.01), 400.0, 640, 400, DEFAULT_LIGHT)


@pytest.mark.parametrize("n,W,H", [(1, 64, 64), (300, 320, 200), (4000, 400, 300)])
def test_raster_soup(oracle, n, W, H):
    """Soups in front of the camera (camera outside the cube): partially off-screen spans, depth ties."""
    tris = mirt.scene_soup(21 + n, n, 0.3 if n < 10 else 0.1)
    _raster_compare(oracle, tris, (0, 0, -3.5), oracle.rot_from_yaw(0.0, 1.01), float(H), W, H, DEFAULT_LIGHT, cull_flags=0)


def test_staging_planes_grow_together(oracle):
    """Regression: a staging plane first requested by a small frame (depth, here) must be as large as the planes
    that larger frames already grew; render big RT -> tiny raster -> medium raster."""
    tris = mirt.scene_soup(3, 50, 0.3)
    rot = oracle.rot_from_yaw(0.0, 1.0)
    _rt_compare(oracle, tris, (0, 0, -2), rot, 180.0, 640, 360, DEFAULT_LIGHT)
    rotr = oracle.rot_from_yaw(0.0, 1.01)
    _raster_compare(oracle, tris, (0, 0, -3.5), rotr, 32.0, 32, 32, DEFAULT_LIGHT, cull_flags=0)
    _raster_compare(oracle, tris, (0, 0, -3.5), rotr, 200.0, 320, 200, DEFAULT_LIGHT, cull_flags=0)


def test_raster_everything_culled(oracle):
    tris = mirt.scene_cornell()
    view = mirt.make_view((0, 0, -3), oracle.rot_from_yaw(0.0, 1.01), 100.0, 128, 128)
    mirt.scene_upload(tris, np.ones(30, np.uint8))
    got = mirt.rasterise(view, DEFAULT_LIGHT)
    assert not got["xrgb"].any() and (got["index"] == -1).all() and not got["depth"].any()



# ---- operands outside the range of the shared-reciprocal divisions / the unscaled square root (csrc/mirt_math2.hpp) ----
# The kernels then take the general operations (wave-uniform branch); the frame must stay bit-identical either way.
ODD_LIGHTS = {
    "zero-and-negative-colour": np.array([[0.0, -0.5, -0.7, 0.0, 1.0, -0.4, 14.0]], np.float32),           # lightColor components 0 and < 0
    "huge-and-tiny-colour": np.array([[0.0, -0.5, -0.7, 3.0e11, 1.0e-14, 1.0, 14.0]], np.float32),         # 4.2e12 > 2^40, 1.4e-13 < 2^-40
    "light-on-the-back-wall": np.array([[0.1, 0.2, 1.0 - 2.0e-7, 1.0, 1.0, 1.0, 14.0]], np.float32),        # r^2 < 2^-42 for the pixels around it
    "light-far-away": np.array([[2.0e5, -3.0e5, -4.0e5, 1.0, 1.0, 1.0, 3.0e12]], np.float32),               # r^2 > 2^36
    "two-lights-one-odd": np.array([[0.0, -0.5, -0.7, 1.0, 1.0, 1.0, 14.0], [0.3, 0.3, -0.2, 0.0, 2.0, 0.0, 5.0]], np.float32),
}


@pytest.mark.parametrize("light", sorted(ODD_LIGHTS))
def test_rt_odd_lights_take_the_general_arithmetic(oracle, light):
    """Tile kernel (Cornell box) and binned trace kernel (soup) with lights whose colour or distance is outside the fast range."""
    L = ODD_LIGHTS[light]
    _rt_compare(oracle, mirt.scene_cornell(), (0, 0, -3), oracle.rot_from_yaw(0.0, 1.0), 200.0, 200, 200, L, mode=mirt.RT_AUTO)
    _rt_compare(oracle, mirt.scene_soup(21, 3000, 0.1), (0.1, 0, -2.2), oracle.rot_from_yaw(0.2, 1.0), 160.0, 320, 200, L, mode=mirt.RT_BINNED)


@pytest.mark.parametrize("light", sorted(ODD_LIGHTS))
def test_raster_odd_lights_take_the_general_arithmetic(oracle, light):
    """Small-scene rasteriser kernel (Cornell box) and the key-buffer path (soup) with the same lights."""
    L = ODD_LIGHTS[light]
    _raster_compare(oracle, mirt.scene_cornell(), (0, 0, -3), oracle.rot_from_yaw(0.0, 1.01), 300.0, 300, 300, L)
    _raster_compare(oracle, mirt.scene_soup(22, 400, 0.2), (0, 0.1, -2.5), oracle.rot_from_yaw(-0.3, 1.0), 200.0, 320, 200, L)


@pytest.mark.parametrize("scale", [1.0e-9, 3.0e-4, 3.0e5])
def test_scaled_scenes_leave_the_fast_range(oracle, scale):
    """The whole configuration scaled: at 1e-9 pos3d * zinv products, determinants and squared distances fall below 2^-40 / 2^-42,
    at 3e5 squared distances, light colours and e1e2b leave the range at the top -- spans, queued pairs and light terms take the general path."""
    tris = mirt.scene_cornell()
    tris[:, 0:9] *= np.float32(scale)
    L = np.array([[0.0, -0.5 * scale, -0.7 * scale, 1.0, 1.0, 1.0, 14.0 * scale * scale]], np.float32)
    cam = (0.0, 0.0, -3.0 * scale)
    _rt_compare(oracle, tris, cam, oracle.rot_from_yaw(0.1, 1.0), 200.0, 200, 200, L, mode=mirt.RT_AUTO)
    _raster_compare(oracle, tris, cam, oracle.rot_from_yaw(0.1, 1.01), 240.0, 240, 240, L)
    soup = mirt.scene_soup(23, 2500, 0.1)
    soup[:, 0:9] *= np.float32(scale)
    _rt_compare(oracle, soup, (0.0, 0.0, -2.0 * scale), oracle.rot_from_yaw(0.0, 1.0), 160.0, 256, 160, L, mode=mirt.RT_BINNED)


def test_errors_are_reported_not_fatal():
    with pytest.raises(mirt.MirtError):
        mirt.scene_upload(np.zeros((0, 15), np.float32))
    view = mirt.make_view((0, 0, -2), np.eye(3, dtype=np.float32).ravel(), 10.0, 0, 10)
    with pytest.raises(mirt.MirtError):
        mirt.raytrace(view, DEFAULT_LIGHT)


def test_packed_division_equals_the_compilers():
    """div2 (csrc/mirt_math2.hpp: two IEEE divisions sharing packed multiply-adds) against `/` on the device, 2^28 random bit
    patterns + special values, compared as bits (tools/div2check.hip, built by __graft_entry__.build())."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "div2check")
    assert os.path.exists(exe), "tools/div2check not built (python -c 'import __graft_entry__ as g; g.build()')"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 mismatching" in r.stdout, r.stdout + r.stderr


def test_shared_denominator_division_equals_the_compilers():
    """div3p / div3 (csrc/mirt_math2.hpp: three IEEE divisions by one denominator sharing the refined reciprocal while every operand
    is in the middle of the exponent range, the general division otherwise) against `/` on the device: 2^28 in-range triples, random
    bit patterns, special values, waves with one odd lane -- compared as bits (tools/div3check.hip)."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "div3check")
    assert os.path.exists(exe), "tools/div3check not built (python -c 'import __graft_entry__ as g; g.build()')"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "in range (2^28 triples): 0, random bits: 0, special values: 0, one odd lane per wave: 0" in r.stdout, r.stdout + r.stderr


def test_profiling_events_per_stream():
    """mirt_set_profiling: per-kernel GPU times of the last call (mirt_get_stats) and, with two frames in flight, of the call
    before it (mirt_get_previous_kernel_ms: the events of a frame survive the frame that follows it on the other stream)."""
    from devbuf import DeviceArray
    tris = np.concatenate([mirt.scene_cornell(), mirt.scene_soup(5, 3000, 0.08)])
    mirt.scene_upload(tris)
    W, H = 640, 360
    views = [mirt.make_view((0.01 * i, 0, -2.2), mirt.rot_from_yaw(0.0, 1.0), 180.0, W, H) for i in range(6)]
    outs = [DeviceArray((H, W), np.uint32, 0), DeviceArray((H, W), np.uint32, 0)]
    mirt.set_profiling(True)
    try:
        mirt.raytrace_device(views[0], mirt.DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, outs[0].ptr, W * 4)
        mirt.sync()
        st = mirt.stats()
        assert st["kernel_ms"]["bin"] > 0 and st["kernel_ms"]["trace"] > 0 and st["gpu_ms"] >= st["kernel_ms"]["trace"]
        with pytest.raises(mirt.MirtError):
            mirt.previous_kernel_ms()                    # one frame in flight: the call before the last one kept nothing
        mirt.set_frames_in_flight(2)
        for i, v in enumerate(views):
            mirt.raytrace_device(v, mirt.DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, outs[i & 1].ptr, W * 4)
        prev, gpu_ms = mirt.previous_kernel_ms()
        last = mirt.stats()
        assert prev["bin"] > 0 and prev["trace"] > 0 and gpu_ms >= prev["trace"]
        assert last["kernel_ms"]["trace"] > 0
        assert prev["raster_frag"] == 0 and prev["dof"] == 0
    finally:
        mirt.set_frames_in_flight(1)
        mirt.set_profiling(False)


# ---- the C++ host adapter (reference-shaped Draw()) ---------------------------------------------------

@pytest.mark.parametrize("which", ["rt", "rtsoft", "rtaa", "rtdof", "raster", "rasterdof", "rtasync", "rasterasync"])
def test_host_draw_adapter_matches_oracle(oracle, tmp_path, which):
    """cpp-raytracer-rasterizer_amd/host/demo_main runs the reference's main loop shape (Update(); Draw();) through
    mirt_draw.hpp and the C-ABI; its surface must hold exactly the words the oracle's PutPixelSDL path produces.
    (*async: eight DrawAsync() frames into two registered surfaces in turn, two in flight, the last one the reference view.)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "cpp-raytracer-rasterizer_amd", "host", "demo_main")
    assert os.path.exists(exe), "host/demo_main not built (make -C cpp-raytracer-rasterizer_amd)"
    W = H = 200
    raw, bmp = str(tmp_path / "out.xrgb"), str(tmp_path / "out.bmp")
    mirt.shutdown()                      # the child process owns the GPU context for this test
    try:
        subprocess.run([exe, which, str(W), str(H), bmp, raw], check=True, timeout=300)
    finally:
        mirt.init(0)
    got = np.fromfile(raw, np.uint32).reshape(H, W)
    tris = oracle.cornell()
    which = which.replace("async", "")
    if which == "rt":
        ref = oracle.raytrace(tris, (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), H / 2.0, W, H, DEFAULT_LIGHT)["xrgb"]
    elif which == "rtdof":
        r = oracle.raytrace(tris, (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), H / 2.0, W, H, DEFAULT_LIGHT)
        ref = oracle.dof(r["rgb"], _rt_focal_distances(r, 1.3), 8)
    elif which == "rasterdof":
        rot = oracle.rot_from_yaw(0.0, 1.01)
        culled = oracle.cull(tris, (0, 0, -3), rot, float(H), W, H, 3)
        r = oracle.rasterise(tris, culled, (0, 0, -3), rot, float(H), W, H, DEFAULT_LIGHT, want=("rgb", "fd"), focal_plane=1.9)
        ref = oracle.dof(r["rgb"], r["fd"], 8, clear_border=True)
    elif which == "rtaa":
        ref = oracle.raytrace(tris, (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), H / 2.0, W, H, DEFAULT_LIGHT, aa=3)["xrgb"]
    elif which == "rtsoft":
        # the adapter draws its jitter from rand() exactly as AddLight does (first 48 values of the default stream)
        jit = _jitter(oracle, DEFAULT_LIGHT, 16)
        ref = oracle.raytrace(tris, (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), H / 2.0, W, H, DEFAULT_LIGHT, samples=16, jitter=jit)["xrgb"]
    else:
        rot = oracle.rot_from_yaw(0.0, 1.01)
        culled = oracle.cull(tris, (0, 0, -3), rot, float(H), W, H, 3)
        ref = oracle.rasterise(tris, culled, (0, 0, -3), rot, float(H), W, H, DEFAULT_LIGHT)["xrgb"]
    assert np.array_equal(got, ref)
    assert os.path.getsize(bmp) == 54 + W * 3 * H


@pytest.mark.parametrize("cube", [128, 256])
def test_rt_binned_finer_light_cube(cube):
    """The light cube is 64/128/256 bins per face depending on the triangle count; force the finer grids on a small
    scene (MIRT_CUBE_BINS, read once per process) and require binned == brute bit for bit."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r)
import mirt
mirt.init(0)
tris = mirt.scene_soup(13, 4000, 0.1)
rot = np.zeros(9, np.float32); rot[0] = rot[4] = rot[8] = 1
view = mirt.make_view((0.1, 0.0, -0.4), rot, 120.0, 320, 200)        # camera inside the soup
lights = np.array([[0, -0.5, -0.7, 1, 1, 1, 14], [0.3, 0.3, 0.3, 1, 1, 1, 6]], np.float32)
mirt.scene_upload(tris)
a = mirt.raytrace(view, lights, mode=mirt.RT_BRUTE)
b = mirt.raytrace(view, lights, mode=mirt.RT_BINNED)
assert b["stats"]["mode_used"] == mirt.RT_BINNED
assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["rgb"].view(np.uint32), b["rgb"].view(np.uint32))
assert np.array_equal(a["xrgb"], b["xrgb"])
print("ok")
''' % os.path.join(root, "cpp-raytracer-rasterizer_amd")
    mirt.shutdown()
    try:
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIRT_CUBE_BINS=str(cube)),
                           capture_output=True, text=True, timeout=300)
    finally:
        mirt.init(0)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_rt_binned_light_cube_follows_a_moving_light():
    """Lights that moved within the last four frames get a coarse light cube binned by the frame itself; the shared fine one
    (256 bins per side from 20 k triangles) is built once the lights have stood still for four frames and stays held while
    other lights pass through; neither changes a result.  Frames with a fixed light (coarse x 4, then fine), then a light
    that moves every frame: every one == brute force bit for bit, and the executed shadow tests drop when the fine grid
    takes over."""
    tris = mirt.scene_soup(21, 24000, 0.06)
    rot = np.zeros(9, np.float32); rot[0] = rot[4] = rot[8] = 1
    view = mirt.make_view((0.0, 0.0, -1.6), rot, 150.0, 300, 180)
    mirt.scene_upload(tris)

    def both(lights):
        a = mirt.raytrace(view, lights, mode=mirt.RT_BRUTE)
        b = mirt.raytrace(view, lights, mode=mirt.RT_BINNED)
        assert b["stats"]["mode_used"] == mirt.RT_BINNED
        assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["rgb"].view(np.uint32), b["rgb"].view(np.uint32))
        assert np.array_equal(a["xrgb"], b["xrgb"])
        return b["stats"]["tests"]

    fixed = np.array([[0.1, -0.4, -0.6, 1, 1, 1, 14]], np.float32)
    mirt.set_profiling(True)                              # (the binned kernel keeps its own counts only for profiled frames)
    try:
        tests = [both(fixed) for _ in range(7)]
    finally:
        mirt.set_profiling(False)
    assert max(tests[4:]) < min(tests[:4]), tests         # (the count varies a little from run to run: early exits race)
    for i in range(4):
        moving = fixed.copy(); moving[0, 0] += 0.05 * (i + 1)
        both(moving)
    assert both(fixed) < min(tests[:4])                 # back on the first position: its shared fine cube is still held


def test_rt_binned_moving_lights_with_two_frames_in_flight():
    """Lights that move every frame are binned by the frame itself, on its own stream (no shared tables, no barrier): ten
    frames queued back to back on two streams, two lights moving (one of them every frame, one every third), then the lights
    stand still long enough for the shared fine cube to take over -- every frame == the brute-force frame of its lights."""
    from devbuf import DeviceArray
    tris = mirt.scene_soup(33, 22000, 0.07)
    rot = np.zeros(9, np.float32); rot[0] = rot[4] = rot[8] = 1
    W, H = 320, 200
    mirt.scene_upload(tris)
    views = [mirt.make_view((0.02 * i, 0.0, -1.7), rot, 160.0, W, H) for i in range(16)]

    def lights_of(i):
        j = min(i, 9)                                    # frames 9..15: the lights stand still
        return np.array([[0.1 + 0.03 * j, -0.4, -0.6, 1, 1, 1, 14], [-0.3, 0.2 + 0.05 * (j // 3), -0.2, 1, 0.8, 0.6, 6]], np.float32)

    want = []
    mirt.set_frames_in_flight(1)
    for i, v in enumerate(views):
        x = DeviceArray((H, W), np.uint32, 0x11)
        mirt.raytrace_device(v, lights_of(i), (0.2, 0.2, 0.2), mirt.RT_BRUTE, 0, H, 0, x.ptr, W * 4)
        mirt.sync()
        want.append(x.read())
    try:
        mirt.set_frames_in_flight(2)
        outs = [DeviceArray((H, W), np.uint32, 0x11) for _ in views]
        for i, v in enumerate(views):
            mirt.raytrace_device(v, lights_of(i), (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, outs[i].ptr, W * 4)
        mirt.sync()
        assert mirt.stats()["mode_used"] == mirt.RT_BINNED
        for i in range(len(views)):
            assert np.array_equal(outs[i].read(), want[i]), i
    finally:
        mirt.set_frames_in_flight(1)


@pytest.mark.parametrize("in_flight", [1, 2, 3])
def test_rt_binned_pass_is_kept_while_the_view_stands_still(in_flight):
    """The reference redraws with the camera where it was whenever a light key, a toggle or a light added / deleted sets isUpdated
    (raytracer.cpp:385-537).  A binned frame whose view, rows and scene are those of its stream's last pass starts at the trace
    kernel (mirt_stats.bins_reused); anything else -- a moved camera, another band, a light binned by the frame that moved, another
    kind of frame on the stream in between -- runs the pass.  A sequence that alternates moved / unmoved views and lights, whole
    frames and bands, with a brute-force frame thrown in between: every frame == the brute-force frame of its parameters, and
    the frames that may keep the pass do."""
    from devbuf import DeviceArray
    tris = mirt.scene_soup(41, 26000, 0.06)
    rot = np.zeros(9, np.float32); rot[0] = rot[4] = rot[8] = 1
    W, H = 320, 200
    mirt.scene_upload(tris)
    views = [mirt.make_view((0.03 * i, 0.0, -1.7), rot, 160.0, W, H) for i in range(3)]
    lights = [np.array([[0.1 + 0.05 * j, -0.4, -0.6, 1, 1, 1, 14]], np.float32) for j in range(4)]
    # (view, light, band, kind): what the stream a frame lands on saw last decides whether its pass is kept
    seq = [(0, 0, None, "binned")] * 6                      # the light settles into the shared cube; from the second frame of a stream on the pass is kept
    seq += [(0, 1, None, "binned"), (0, 1, None, "binned"), (0, 2, None, "binned"), (1, 2, None, "binned"), (1, 2, None, "binned"), (1, 2, (40, 120), "binned"),
            (1, 2, (40, 120), "binned"), (1, 2, None, "binned"), (1, 2, None, "brute"), (1, 2, None, "binned"), (1, 2, None, "binned"), (2, 3, None, "binned"),
            (2, 3, None, "binned"), (2, 3, None, "binned"), (2, 3, None, "binned"), (2, 3, None, "binned"), (2, 3, None, "binned"), (2, 3, None, "binned"), (0, 3, None, "binned")]
    want = {}
    mirt.set_frames_in_flight(1)
    for v, l, band, _ in seq:
        if (v, l) not in want:
            x = DeviceArray((H, W), np.uint32, 0x11)
            mirt.raytrace_device(views[v], lights[l], (0.2, 0.2, 0.2), mirt.RT_BRUTE, 0, H, 0, x.ptr, W * 4)
            want[(v, l)] = x.read()
            x.free()
    outs = []
    try:
        mirt.set_frames_in_flight(in_flight)
        last = [None] * in_flight                           # what each stream's last binned pass was for: (view, band, lights binned by the frame)
        reused = kept_possible = 0
        for i, (v, l, band, kind) in enumerate(seq):
            x = DeviceArray((H, W), np.uint32, 0x11)
            outs.append(x)
            y0, y1 = band if band else (0, H)
            mirt.raytrace_device(views[v], lights[l], (0.2, 0.2, 0.2), mirt.RT_BINNED if kind == "binned" else mirt.RT_BRUTE, y0, y1, 0, x.ptr, W * 4)
            st = mirt.stats()                               # (waits for the frame)
            si = i % in_flight
            if kind == "binned":
                assert st["mode_used"] == mirt.RT_BINNED
                if st["bins_reused"]:
                    reused += 1
                    assert last[si] is not None and last[si][:2] == (v, band), "frame %d kept a pass of another view or band" % i
                else:
                    assert st["selected_triangles"] > 0
                last[si] = (v, band)
            else:
                assert not st["bins_reused"]
                last[si] = None                             # the brute-force frame rebuilt the stream's origin rows
            got = x.read()
            assert np.array_equal(got[y0:y1], want[(v, l)][y0:y1]), "frame %d (view %d light %d band %s %s): %d words differ" % (
                i, v, l, band, kind, int((got[y0:y1] != want[(v, l)][y0:y1]).sum()))
        # the view stands still through most of the sequence: with one frame in flight about a dozen frames start at the trace kernel
        # (the frame that finds its light unchanged for the fourth time builds the shared cube and runs its pass again)
        assert reused >= (8 if in_flight == 1 else 2), reused
    finally:
        mirt.set_frames_in_flight(1)
        for x in outs:
            x.free()


# ---- edge cases: tiny / ragged frames and kernel-selection boundaries ----------------------------------

@pytest.mark.parametrize("W,H", [(1, 1), (2, 3), (3, 3), (7, 5), (65, 9), (130, 3)])
def test_rt_tiny_and_ragged_frames(oracle, W, H):
    """Frames smaller than a tile / a wave, widths not a multiple of anything."""
    _rt_compare(oracle, mirt.scene_cornell(), (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), max(H, 2) / 2.0, W, H, DEFAULT_LIGHT, mode=mirt.RT_AUTO)
    tris = mirt.scene_soup(8, 700, 0.2)
    _rt_compare(oracle, tris, (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), max(H, 2) / 2.0, W, H, DEFAULT_LIGHT, mode=mirt.RT_BINNED)
    _rt_compare(oracle, tris, (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), max(H, 2) / 2.0, W, H, DEFAULT_LIGHT, mode=mirt.RT_BRUTE)


@pytest.mark.parametrize("n", [2, 63, 64, 65, 333, 334, 340, 1023, 1024, 1025, 2049])
def test_rt_kernel_selection_boundaries(oracle, n):
    """n = 64/65: tile-mask kernel vs LDS-resident kernel; 333/334: LDS-resident vs chunked brute force; 1024/1025:
    one LDS chunk vs two; every choice must give the same bits."""
    tris = mirt.scene_soup(100 + n, n, 0.3 if n < 400 else 0.15)
    _rt_compare(oracle, tris, (0, 0, -2), oracle.rot_from_yaw(0.3, 1.0), 60.0, 150, 90, DEFAULT_LIGHT, mode=mirt.RT_BRUTE)


def test_rt_no_lights_and_many_lights(oracle):
    tris = mirt.scene_cornell()
    rot = oracle.rot_from_yaw(0.0, 1.0)
    _rt_compare(oracle, tris, (0, 0, -2), rot, 50.0, 100, 100, np.zeros((0, 7), np.float32), mode=mirt.RT_AUTO)
    rng = np.random.default_rng(3)
    lights = np.concatenate([rng.uniform(-0.8, 0.8, (32, 3)), rng.uniform(0.2, 1.0, (32, 3)), rng.uniform(1, 5, (32, 1))], axis=1).astype(np.float32)
    _rt_compare(oracle, tris, (0, 0, -2), rot, 40.0, 80, 64, lights, mode=mirt.RT_AUTO)                      # MIRT_MAX_LIGHTS
    _rt_compare(oracle, mirt.scene_soup(4, 2000, 0.15), (0, 0, -2), rot, 40.0, 80, 64, lights[:5], mode=mirt.RT_BINNED)


@pytest.mark.parametrize("W,H", [(1, 1), (2, 2), (5, 3), (9, 70)])
def test_raster_tiny_frames(oracle, W, H):
    _raster_compare(oracle, mirt.scene_cornell(), (0, 0, -3), oracle.rot_from_yaw(0.0, 1.01), float(H), W, H, DEFAULT_LIGHT)


def test_raster_triangles_crossing_the_camera_plane(oracle):
    """Vertices at or behind the camera give infinite / out-of-contract screen coordinates: such triangles are skipped
    by product and oracle alike, the rest must still match."""
    tris = mirt.scene_soup(12, 400, 0.6)
    _raster_compare(oracle, tris, (0.0, 0.0, -0.2), oracle.rot_from_yaw(0.2, 1.01), 120.0, 240, 160, DEFAULT_LIGHT, cull_flags=0)


def test_raster_two_lights_and_band(oracle):
    lights = np.array([[0, -0.5, -0.7, 1, 1, 1, 14], [0.5, 0.4, -1.5, 0.2, 0.9, 0.5, 9]], np.float32)
    from devbuf import DeviceArray
    W, H = 320, 300
    cam, rot = (0.1, 0, -3), oracle.rot_from_yaw(0.15, 1.01)
    _, ref = _raster_compare(oracle, mirt.scene_cornell(), cam, rot, 300.0, W, H, lights)
    # the same view (scene and cull flags as _raster_compare uploaded them) in two bands that split the frame on an odd row
    view = mirt.make_view(cam, rot, 300.0, W, H)
    for (y0, y1) in [(0, 113), (113, 300)]:
        with DeviceArray((H, W), np.uint32, 0x5A) as surf:
            mirt.rasterise_device(view, lights, (0.2, 0.2, 0.2), y0, y1, 0, surf.ptr, W * 4)
            got = surf.read()
        assert np.array_equal(got[y0:y1], ref["xrgb"][y0:y1]), "band [%d, %d): %d words differ" % (y0, y1, int((got[y0:y1] != ref["xrgb"][y0:y1]).sum()))
        assert (got[:y0] == 0x5A5A5A5A).all() and (got[y1:] == 0x5A5A5A5A).all()


# ---- depth of field (parity unpinned: no recorded reference output) ---------------

class _DeviceWords:
    """A W*H uint32 device surface, for the *_device entry points."""

    def __init__(self, W, H, fill=0):
        import ctypes as C
        self.C, self.W, self.H = C, W, H
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), W * H * 4) == 0
        init = np.full((H, W), fill, np.uint32)
        assert self.hip.hipMemcpy(self.ptr, init.ctypes.data_as(C.c_void_p), W * H * 4, 1) == 0

    def read(self):
        out = np.zeros((self.H, self.W), np.uint32)
        mirt.sync()
        assert self.hip.hipMemcpy(out.ctypes.data_as(self.C.c_void_p), self.ptr, self.W * self.H * 4, 2) == 0
        return out

    def free(self):
        self.hip.hipFree(self.ptr)


def _rt_focal_distances(ref, focal_plane):
    """focalDistances as ClosestIntersection leaves them (raytracer.cpp:249): closest distance - FOCAL_LENGTH, and the
    zero-initialised global where no primary ray hit."""
    return np.where(ref["index"] >= 0, ref["dist"] - np.float32(focal_plane), np.float32(0)).astype(np.float32)


@pytest.mark.parametrize("K,FL,scene,mode,aa", [(8, 1.3, "cornell", mirt.RT_AUTO, 1), (8, 1.3, "soup", mirt.RT_BINNED, 1),
                                                (3, 2.0, "soup", mirt.RT_BRUTE, 1), (5, 1.0, "cornell", mirt.RT_AUTO, 3),
                                                (2, 1.3, "sparse", mirt.RT_AUTO, 1)])
def test_rt_depth_of_field(oracle, K, FL, scene, mode, aa):
    """DOF_ENABLED: CalculateDOF's K x K blur weighted by |distance - FOCAL_LENGTH| (raytracer.cpp:608-646); the
    colour and index planes stay the un-blurred pixelColours / closest hits."""
    tris = {"cornell": mirt.scene_cornell(), "soup": mirt.scene_soup(9, 2500, 0.1), "sparse": mirt.scene_soup(4, 40, 0.2)}[scene]
    W, H = 230, 170
    cam, rot, focal = (0, 0, -2), oracle.rot_from_yaw(0.1, 1.0), 85.0
    ref = oracle.raytrace(tris, cam, rot, focal, W, H, DEFAULT_LIGHT, aa=aa)
    want = oracle.dof(ref["rgb"], _rt_focal_distances(ref, FL), K, xrgb=np.zeros((H, W), np.uint32))
    mirt.scene_upload(tris)
    mirt.set_antialiasing(aa)
    mirt.set_depth_of_field(K, FL)
    try:
        got = mirt.raytrace(mirt.make_view(cam, rot, focal, W, H), DEFAULT_LIGHT, mode=mode)
    finally:
        mirt.set_depth_of_field(0)
        mirt.set_antialiasing(1)
    assert np.array_equal(got["index"], ref["index"])
    assert np.array_equal(got["rgb"].view(np.uint32), ref["rgb"].view(np.uint32))
    assert np.array_equal(got["xrgb"], want), "%d blurred pixels differ" % int((got["xrgb"] != want).sum())
    assert not np.array_equal(want, ref["xrgb"])                          # the blur did something


def test_rt_depth_of_field_bands(oracle):
    """Bands under DOF need a halo of K/2 rows from the neighbouring band: every band renders its halo itself."""
    tris = mirt.scene_soup(21, 1200, 0.12)
    W, H, K, FL = 190, 131, 8, 1.3
    cam, rot, focal = (0, 0, -2), oracle.rot_from_yaw(-0.1, 1.0), 70.0
    ref = oracle.raytrace(tris, cam, rot, focal, W, H, DEFAULT_LIGHT)
    want = oracle.dof(ref["rgb"], _rt_focal_distances(ref, FL), K, xrgb=np.full((H, W), 0x55, np.uint32))
    mirt.scene_upload(tris)
    view = mirt.make_view(cam, rot, focal, W, H)
    surf = _DeviceWords(W, H, 0x55)
    mirt.set_depth_of_field(K, FL)
    try:
        for (y0, y1) in [(0, 3), (3, 47), (47, 48), (48, 128), (128, 131)]:
            mirt.raytrace_device(view, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_AUTO, y0, y1, 0, surf.ptr, W * 4)
        got = surf.read()
    finally:
        mirt.set_depth_of_field(0)
        surf.free()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("K", [8, 5])
def test_depth_of_field_into_a_band_buffer_with_its_own_pitch(oracle, K):
    """A rank of a sharded frame resolves its band into a buffer that starts at the band's first row (row_origin = y0) and may be
    wider than the frame (pitch > width): the blur's stores address that buffer (k_dof_tile<8>: range-checked against ITS extent),
    words beyond the frame's width and rows beyond the band stay what they were."""
    tris = mirt.scene_soup(33, 900, 0.12)
    W, H, FL, pitch_words = 150, 96, 1.3, 157
    cam, rot, focal = (0, 0, -2), oracle.rot_from_yaw(0.05, 1.0), 60.0
    ref = oracle.raytrace(tris, cam, rot, focal, W, H, DEFAULT_LIGHT)
    want = oracle.dof(ref["rgb"], _rt_focal_distances(ref, FL), K, xrgb=np.full((H, W), 0x66, np.uint32))
    mirt.scene_upload(tris)
    view = mirt.make_view(cam, rot, focal, W, H)
    mirt.set_depth_of_field(K, FL)
    try:
        for (y0, y1) in [(0, 40), (40, 77), (77, 96)]:
            rows = y1 - y0
            surf = _DeviceWords(pitch_words, rows + 2, 0x66)               # (two rows of slack behind the band)
            mirt.raytrace_device(view, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_AUTO, y0, y1, y0, surf.ptr, pitch_words * 4)
            got = surf.read()
            surf.free()
            assert np.array_equal(got[:rows, :W], want[y0:y1]), "band [%d, %d)" % (y0, y1)
            assert (got[:rows, W:] == 0x66).all() and (got[rows:] == 0x66).all()
    finally:
        mirt.set_depth_of_field(0)


@pytest.mark.parametrize("K,FL,W,H", [(8, 1.9, 320, 240), (3, 3.0, 97, 61)])
def test_raster_depth_of_field(oracle, K, FL, W, H):
    """Rasteriser CalculateDOF (rasteriser.cpp:494-513) over focalDistances = |pPos3d - cameraPos| - FOCAL_LENGTH of the
    fragment that owns the pixel (:563-565); the border stays the black Update() painted."""
    tris = np.concatenate([mirt.scene_cornell(), mirt.scene_soup(2, 200, 0.15)])
    cam, rot, focal = (0.1, 0, -3), oracle.rot_from_yaw(0.1, 1.01), float(H)
    view = mirt.make_view(cam, rot, focal, W, H)
    culled = mirt.cull(tris, view, 3)
    ref = oracle.rasterise(tris, culled, cam, rot, focal, W, H, DEFAULT_LIGHT, want=("rgb", "index", "xrgb", "depth", "fd"), focal_plane=FL)
    want = oracle.dof(ref["rgb"], ref["fd"], K, clear_border=True)
    mirt.scene_upload(tris, culled)
    mirt.set_depth_of_field(K, FL)
    try:
        got = mirt.rasterise(view, DEFAULT_LIGHT)
        surf = _DeviceWords(W, H, 0x77)
        for (y0, y1) in [(0, 2), (2, H // 2 + 1), (H // 2 + 1, H)]:
            mirt.rasterise_device(view, DEFAULT_LIGHT, (0.2, 0.2, 0.2), y0, y1, 0, surf.ptr, W * 4)
        banded = surf.read()
        surf.free()
    finally:
        mirt.set_depth_of_field(0)
    assert np.array_equal(got["index"], ref["index"])
    assert np.array_equal(got["depth"].view(np.uint32), ref["depth"].view(np.uint32))
    assert np.array_equal(got["rgb"].view(np.uint32), ref["rgb"].view(np.uint32))
    assert np.array_equal(got["xrgb"], want), "%d blurred pixels differ" % int((got["xrgb"] != want).sum())
    assert np.array_equal(banded, want)
    assert not np.array_equal(want, ref["xrgb"])


def test_depth_of_field_limits():
    with pytest.raises(mirt.MirtError):
        mirt.set_depth_of_field(65, 1.0)
    mirt.set_depth_of_field(1, 1.0)                                       # <= 1 switches it off


def test_depth_of_field_validates_the_callers_surface():
    """With the blur on, the caller's surface goes straight to the blur kernel: a NULL surface, a short or unaligned pitch,
    a bad band or an absurd frame must come back as errors (as they do without the blur), never reach a kernel."""
    mirt.scene_upload(mirt.scene_cornell())
    W, H = 64, 48
    rot = np.eye(3, dtype=np.float32).ravel()
    view = mirt.make_view((0, 0, -2), rot, 24.0, W, H)
    surf = _DeviceWords(W, H, 0x42)
    mirt.set_depth_of_field(8, 1.3)
    try:
        for call in (mirt.raytrace_device, None):
            def run(v, y0, y1, ptr, pitch):
                if call is not None:
                    mirt.raytrace_device(v, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_AUTO, y0, y1, 0, ptr, pitch)
                else:
                    mirt.rasterise_device(v, DEFAULT_LIGHT, (0.2, 0.2, 0.2), y0, y1, 0, ptr, pitch)
            for args in ((view, 0, H, None, W * 4), (view, 0, H, surf.ptr, W * 4 - 4), (view, 0, H, surf.ptr, W * 4 + 2),
                         (view, -1, H, surf.ptr, W * 4), (view, 0, H + 1, surf.ptr, W * 4), (view, 5, 4, surf.ptr, W * 4),
                         (mirt.make_view((0, 0, -2), rot, 24.0, 40000, H), 0, H, surf.ptr, 40000 * 4),
                         (mirt.make_view((0, 0, -2), rot, 24.0, 0, H), 0, H, surf.ptr, W * 4)):
                with pytest.raises(mirt.MirtError):
                    run(*args)
            run(view, 0, H, surf.ptr, W * 4)                               # and a valid call still renders
        mirt.sync()
        assert (surf.read()[1:-1, 1:-1] != 0x42424242).any()
    finally:
        mirt.set_depth_of_field(0)
        surf.free()


# ---- two frames in flight ---------------------------------------------------------------------------------------

def test_two_frames_in_flight(oracle):
    """mirt_set_frames_in_flight(2): consecutive device calls alternate between two streams.  Frames of two different
    views rendered back to back into two surfaces must equal the frames rendered one at a time, the statistics must be
    those of the last call, and calls that share library state (binned mode, rasteriser, depth of field) interleaved
    with them must still come out right."""
    tris = mirt.scene_cornell()
    W, H = 333, 207
    rot_a, rot_b = oracle.rot_from_yaw(0.0, 1.0), oracle.rot_from_yaw(0.4, 1.0)
    va = mirt.make_view((0, 0, -2), rot_a, 100.0, W, H)
    vb = mirt.make_view((0.2, 0.1, -2.3), rot_b, 120.0, W, H)
    mirt.scene_upload(tris)
    want_a = mirt.raytrace(va, DEFAULT_LIGHT)
    want_b = mirt.raytrace(vb, DEFAULT_LIGHT)
    culled = mirt.cull(tris, va, 3)
    mirt.scene_upload(tris, culled)
    want_r = mirt.rasterise(va, DEFAULT_LIGHT)["xrgb"]
    mirt.scene_upload(tris)
    sa, sb, sr = _DeviceWords(W, H), _DeviceWords(W, H), _DeviceWords(W, H, 0x99)
    mirt.set_frames_in_flight(2)
    try:
        for i in range(40):
            mirt.raytrace_device(va, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_AUTO, 0, H, 0, sa.ptr, W * 4)
            mirt.raytrace_device(vb, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_AUTO, 0, H, 0, sb.ptr, W * 4)
        assert mirt.stats()["shadow_rays"] == want_b["stats"]["shadow_rays"]
        assert np.array_equal(sa.read(), want_a["xrgb"]) and np.array_equal(sb.read(), want_b["xrgb"])
        # an odd number of calls, then calls that must not overlap their neighbours
        mirt.raytrace_device(va, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_AUTO, 0, H, 0, sa.ptr, W * 4)
        mirt.raytrace_device(vb, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, sb.ptr, W * 4)
        mirt.raytrace_device(va, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_BRUTE, 0, H, 0, sa.ptr, W * 4)
        assert mirt.stats()["shadow_rays"] == want_a["stats"]["shadow_rays"]
        mirt.scene_upload(tris, culled)
        mirt.rasterise_device(va, DEFAULT_LIGHT, (0.2, 0.2, 0.2), 0, H, 0, sr.ptr, W * 4)
        mirt.raytrace_device(vb, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_AUTO, 0, H, 0, sb.ptr, W * 4)
        mirt.rasterise_device(va, DEFAULT_LIGHT, (0.2, 0.2, 0.2), 0, H, 0, sr.ptr, W * 4)
        assert np.array_equal(sr.read(), want_r)
        assert np.array_equal(sa.read(), want_a["xrgb"]) and np.array_equal(sb.read(), want_b["xrgb"])
        got = mirt.raytrace(va, DEFAULT_LIGHT)                               # host-buffer entry point under the same mode
        assert np.array_equal(got["xrgb"], want_a["xrgb"]) and got["stats"]["shadow_rays"] == want_a["stats"]["shadow_rays"]
    finally:
        mirt.set_frames_in_flight(1)
        for s in (sa, sb, sr):
            s.free()
    with pytest.raises(mirt.MirtError):
        mirt.set_frames_in_flight(5)


def test_rt_binned_pair_list_grows(oracle, tmp_path):
    """The (bin, triangle) pair list starts with room for 2^20 pairs and is re-sized from the count the binning pass
    reports; started with room for 1000 (MIRT_BIN_INITIAL_PAIRS), a soup that needs ~100 times that must still render the
    brute-force frame -- in a child process, because the first capacity is read once per process."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "import mirt\n"
        "mirt.init(0)\n"
        "tris = mirt.scene_soup(8, 9000, 0.1)\n"
        "mirt.scene_upload(tris)\n"
        "rot = np.zeros(9, np.float32); rot[0] = rot[4] = rot[8] = 1\n"
        "view = mirt.make_view((0, 0, -2), rot, 180.0, 480, 360)\n"
        "light = np.array([[0, -0.5, -0.7, 1, 1, 1, 14]], np.float32)\n"
        "a = mirt.raytrace(view, light, mode=mirt.RT_BINNED)\n"
        "b = mirt.raytrace(view, light, mode=mirt.RT_BINNED)\n"      # second frame: cached count, no re-size
        "c = mirt.raytrace(view, light, mode=mirt.RT_BRUTE)\n"
        "assert a['stats']['mode_used'] == mirt.RT_BINNED\n"
        "ok = all(np.array_equal(a[k], c[k]) and np.array_equal(b[k], c[k]) for k in ('xrgb', 'index')) and np.array_equal(a['rgb'].view(np.uint32), c['rgb'].view(np.uint32))\n"
        "print('OK' if ok else 'MISMATCH')\n" % os.path.join(root, "cpp-raytracer-rasterizer_amd"))
    mirt.shutdown()
    try:
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MIRT_BIN_INITIAL_PAIRS="1000"),
                             capture_output=True, text=True, timeout=300)
    finally:
        mirt.init(0)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().endswith("OK"), out.stdout[-500:]


@pytest.mark.parametrize("seed", range(48))
def test_rt_binned_equals_brute_on_random_configurations(oracle, seed):
    """Seeded random scenes, cameras (some inside the soup, some rotated past 90 degrees) and one to three lights (some
    inside the soup, some almost in a triangle's plane): the binned frame -- conservative boxes, behind-the-plane rule,
    flattened bin tests, sorted pair lists -- must equal the brute-force frame word for word, plane for plane.  (Brute
    force itself is checked against the oracle above; this widens the binner's coverage cheaply.)"""
    rng = np.random.RandomState(1000 + seed)
    n = int(rng.choice([600, 1500, 4000, 9000]))
    size = float(rng.choice([0.03, 0.08, 0.2, 0.5]))
    tris = mirt.scene_soup(200 + seed, n, size)
    if seed % 4 == 0:
        tris = np.concatenate([tris, mirt.scene_cornell()])             # walls: the wave-walk path, exact ties
    W, H = int(rng.randint(90, 420)), int(rng.randint(70, 300))
    cam = rng.uniform(-1.2, 1.2, 3) if seed % 3 == 0 else np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), -rng.uniform(1.5, 3.0)])
    rot = oracle.rot_from_yaw(float(rng.uniform(-3.1, 3.1)) if seed % 2 else float(rng.uniform(-0.4, 0.4)), 1.0)
    focal = float(rng.uniform(0.3, 1.2) * H)
    nl = 1 + seed % 3
    lights = np.zeros((nl, 7), np.float32)
    lights[:, 0:3] = rng.uniform(-0.9, 0.9, (nl, 3))
    lights[:, 3:6] = rng.uniform(0.2, 1.0, (nl, 3))
    lights[:, 6] = rng.uniform(3, 20, nl)
    if seed % 5 == 0:                                                   # a light (almost) in the plane of triangle 7
        v0, e1, e2 = tris[7, 0:3], tris[7, 3:6] - tris[7, 0:3], tris[7, 6:9] - tris[7, 0:3]
        lights[0, 0:3] = v0 + 3.0 * e1 - 2.5 * e2 + (1e-7 if seed % 10 == 0 else 0.0) * tris[7, 9:12]
    mirt.scene_upload(tris)
    view = mirt.make_view(cam, rot, focal, W, H)
    a = mirt.raytrace(view, lights, mode=mirt.RT_BINNED)
    b = mirt.raytrace(view, lights, mode=mirt.RT_BRUTE)
    assert a["stats"]["mode_used"] == mirt.RT_BINNED and b["stats"]["mode_used"] == mirt.RT_BRUTE
    assert np.array_equal(a["index"], b["index"]), "closest-hit index differs in %d pixels" % int((a["index"] != b["index"]).sum())
    assert np.array_equal(a["rgb"].view(np.uint32), b["rgb"].view(np.uint32))
    assert np.array_equal(a["xrgb"], b["xrgb"])
    assert a["stats"]["shadow_rays"] == b["stats"]["shadow_rays"]


@pytest.mark.parametrize("seed", range(24))
def test_rt_tile_kernel_on_random_small_scenes(oracle, seed):
    """Scenes of 1 to 64 triangles take the two-pixels-per-lane tile kernel (packed FP32, candidate masks, DPP direction
    boxes).  Seeded random triangles (large ones, so tiles see many candidates), cameras, lights and ragged frame sizes,
    sometimes with soft shadows: index, float colours and surface against the oracle."""
    rng = np.random.RandomState(5000 + seed)
    n = int(rng.choice([1, 2, 7, 30, 63, 64]))
    tris = mirt.scene_soup(900 + seed, n, float(rng.choice([0.3, 0.8, 1.5])))
    W, H = int(rng.randint(17, 200)), int(rng.randint(9, 150))
    cam = np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6), -rng.uniform(0.5, 3.0)])
    rot = oracle.rot_from_yaw(float(rng.uniform(-0.8, 0.8)), 1.0)
    nl = 1 + seed % 2
    lights = np.zeros((nl, 7), np.float32)
    lights[:, 0:3] = rng.uniform(-1.0, 1.0, (nl, 3))
    lights[:, 3:6] = rng.uniform(0.2, 1.0, (nl, 3))
    lights[:, 6] = rng.uniform(3, 20, nl)
    samples = 4 if seed % 6 == 0 else 1
    jit = _jitter(oracle, lights, samples, seed=seed + 1) if samples > 1 else None
    got, _ = _rt_compare(oracle, tris, cam, rot, float(rng.uniform(0.4, 1.1) * H), W, H, lights, mode=mirt.RT_AUTO, threads=8,
                         samples=samples, jitter=jit)
    assert got["stats"]["mode_used"] == mirt.RT_BRUTE


@pytest.mark.parametrize("seed", range(12))
def test_raster_on_random_configurations(oracle, seed):
    """Seeded random soups, cameras (rotated, close to and inside the geometry), cull flags and frame sizes through the
    rasteriser: culled set, owner index, depth, float colours and surface against the oracle."""
    rng = np.random.RandomState(7000 + seed)
    n = int(rng.choice([40, 300, 2000]))
    tris = mirt.scene_soup(300 + seed, n, float(rng.choice([0.05, 0.2, 0.6])))
    if seed % 3 == 0:
        tris = np.concatenate([tris, mirt.scene_cornell()])
    W, H = int(rng.randint(33, 260)), int(rng.randint(20, 200))
    cam = np.array([rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), -rng.uniform(0.3, 3.5)])
    rot = oracle.rot_from_yaw(float(rng.uniform(-1.0, 1.0)), 1.01)
    nl = 1 + seed % 2
    lights = np.zeros((nl, 7), np.float32)
    lights[:, 0:3] = rng.uniform(-1.0, 1.0, (nl, 3))
    lights[:, 3:6] = rng.uniform(0.2, 1.0, (nl, 3))
    lights[:, 6] = rng.uniform(3, 20, nl)
    _raster_compare(oracle, tris, cam, rot, float(rng.uniform(0.5, 1.3) * H), W, H, lights, cull_flags=seed % 4)


def test_rt_binned_frame_with_more_than_64_level0_cells(oracle):
    """A 4104 x 4104 frame has 9 x 9 = 81 cells of 64 x 64 bins, more than the 64-bit level-0 mask a lane keeps for a huge
    item; the walk then tests the cells itself.  Cornell walls (huge items covering most of the screen) + a sparse soup,
    binned against brute force."""
    tris = np.concatenate([mirt.scene_cornell(), mirt.scene_soup(77, 400, 0.25)])
    W = H = 4104
    mirt.scene_upload(tris)
    view = mirt.make_view((0.1, -0.05, -2.2), oracle.rot_from_yaw(0.05, 1.0), H / 2.0, W, H)
    a = mirt.raytrace(view, DEFAULT_LIGHT, mode=mirt.RT_BINNED, want_rgb=False)
    b = mirt.raytrace(view, DEFAULT_LIGHT, mode=mirt.RT_BRUTE, want_rgb=False)
    assert a["stats"]["mode_used"] == mirt.RT_BINNED
    assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["xrgb"], b["xrgb"])
    assert a["stats"]["shadow_rays"] == b["stats"]["shadow_rays"]


def test_two_frames_in_flight_with_depth_of_field(oracle):
    """Depth-of-field frames (library-owned pixelColours / focalDistances planes, one set per stream) of two views, ray
    traced and rasterised alternately into four surfaces with two frames in flight, against the same frames one at a time."""
    tris = mirt.scene_cornell()
    W, H = 210, 150
    va = mirt.make_view((0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 75.0, W, H)
    vb = mirt.make_view((0.15, 0.1, -2.6), oracle.rot_from_yaw(-0.3, 1.01), 110.0, W, H)
    mirt.scene_upload(tris, mirt.cull(tris, vb, 3))
    mirt.set_depth_of_field(8, 1.6)
    surf = [_DeviceWords(W, H, 0x11 * (i + 1)) for i in range(4)]
    try:
        want = []
        for i, (v, rt) in enumerate([(va, True), (vb, False), (vb, True), (va, False)]):
            if rt:
                mirt.raytrace_device(v, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_AUTO, 0, H, 0, surf[i].ptr, W * 4)
            else:
                mirt.rasterise_device(v, DEFAULT_LIGHT, (0.2, 0.2, 0.2), 0, H, 0, surf[i].ptr, W * 4)
            want.append(surf[i].read())
        assert not np.array_equal(want[0], want[2])
        mirt.set_frames_in_flight(2)
        for _ in range(25):
            mirt.raytrace_device(va, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_AUTO, 0, H, 0, surf[0].ptr, W * 4)
            mirt.rasterise_device(vb, DEFAULT_LIGHT, (0.2, 0.2, 0.2), 0, H, 0, surf[1].ptr, W * 4)
            mirt.raytrace_device(vb, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_AUTO, 0, H, 0, surf[2].ptr, W * 4)
            mirt.rasterise_device(va, DEFAULT_LIGHT, (0.2, 0.2, 0.2), 0, H, 0, surf[3].ptr, W * 4)
        for i in range(4):
            assert np.array_equal(surf[i].read(), want[i]), "surface %d" % i
    finally:
        mirt.set_frames_in_flight(1)
        mirt.set_depth_of_field(0)
        for s in surf:
            s.free()


@pytest.mark.parametrize("path", ["direct", "dma"])
def test_registered_host_surface(oracle, path):
    """mirt_surface_register: frames delivered into a pinned + mapped host surface (render kernels store straight into it, or
    one DMA copy) hold the same words as the pageable path -- with a pitch wider than the frame, the border the ray tracer
    never writes, and the rasteriser's every-word-written rule; in a child process because the delivery mode is read once."""
    import os
    import subprocess
    import sys
    code = r"""
import sys, numpy as np
sys.path[:0] = [%r, %r]
import mirt
from mirt_oracle import Oracle, DEFAULT_LIGHT
o = Oracle()
mirt.init(0)
W, H, PW = 333, 207, 352
for kind in ("rt", "rtbinned", "raster", "rtdof"):
    tris = mirt.scene_cornell() if kind != "rtbinned" else np.concatenate([mirt.scene_cornell(), mirt.scene_soup(3, 500, 0.1)])
    rot = mirt.rot_from_yaw(0.2, 1.01 if kind == "raster" else 1.0)
    view = mirt.make_view((0.1, 0, -2.5), rot, 150.0, W, H)
    mirt.scene_upload(tris, mirt.cull(tris, view, 3) if kind == "raster" else None)
    mirt.set_depth_of_field(8 if kind == "rtdof" else 0, 1.3)
    call = (lambda x: mirt.rasterise(view, DEFAULT_LIGHT, xrgb=x)) if kind == "raster" else (lambda x: mirt.raytrace(view, DEFAULT_LIGHT, mode=mirt.RT_BINNED if kind == "rtbinned" else mirt.RT_AUTO, xrgb=x))
    want = np.full((H, PW), 0xABCDEF01, np.uint32)
    call(want[:, :W])
    got = np.full((H, PW), 0xABCDEF01, np.uint32)
    mirt.surface_register(got)
    for rep in range(3):
        call(got[:, :W])
    assert np.array_equal(got, want), kind
    assert (got[:, W:] == 0xABCDEF01).all()
    if kind != "raster":
        assert (got[0, :W] == 0xABCDEF01).all() and (got[:, 0] == 0xABCDEF01).all()      # border never written (raytracer.cpp:618-620)
    mirt.surface_unregister(got)
    call(got[:, :W])                                   # back on the pageable path
    assert np.array_equal(got, want)
mirt.set_depth_of_field(0)
mirt.shutdown()
print("ok")
""" % (os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpp-raytracer-rasterizer_amd"),
       os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    env = dict(os.environ, MIRT_HOST_PATH=path)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("path", ["direct", "dma"])
def test_asynchronous_frames_into_registered_surfaces(path):
    """mirt_raytrace_async / mirt_rasterise_async: frames queued without a host sync into two registered surfaces in turn (two
    frames in flight: the copy of one overlaps the render of the next), completed by mirt_sync -- every surface then holds the
    words the synchronous call delivers for its view, pitch wider than the frame, border untouched; a surface that is not
    registered is refused.  In a child process: the delivery mode is read once."""
    import os
    import subprocess
    import sys
    code = r"""
import sys, numpy as np
sys.path[:0] = [%r]
import mirt
mirt.init(0)
L = mirt.DEFAULT_LIGHT
W, H, PW = 333, 207, 352
for kind in ("rt", "rtbinned", "raster", "rtdof"):
    tris = mirt.scene_cornell() if kind != "rtbinned" else np.concatenate([mirt.scene_cornell(), mirt.scene_soup(3, 500, 0.1)])
    views = [mirt.make_view((0.1 + 0.02 * i, 0, -2.5), mirt.rot_from_yaw(0.2, 1.01 if kind == "raster" else 1.0), 150.0, W, H) for i in range(6)]
    mirt.scene_upload(tris, mirt.cull(tris, views[0], 0) if kind == "raster" else None)
    mirt.set_depth_of_field(8 if kind == "rtdof" else 0, 1.3)
    mode = mirt.RT_BINNED if kind == "rtbinned" else mirt.RT_AUTO
    mirt.set_frames_in_flight(1)
    want = []
    for v in views:
        x = np.full((H, PW), 0xABCDEF01, np.uint32)
        (mirt.rasterise(v, L, xrgb=x[:, :W]) if kind == "raster" else mirt.raytrace(v, L, mode=mode, xrgb=x[:, :W]))
        want.append(x)
    big = np.full((len(views), H, PW), 0xABCDEF01, np.uint32)         # one registration, six surfaces inside it
    mirt.surface_register(big)
    for fl in (1, 2):
        big[:] = 0xABCDEF01
        mirt.set_frames_in_flight(fl)
        calls = [mirt.prepared_async("raster" if kind == "raster" else "rt", v, L, (0.2, 0.2, 0.2), mode, big[i][:, :W]) for i, v in enumerate(views)]
        for c in calls:
            c()
        mirt.sync()
        for i in range(len(views)):
            assert np.array_equal(big[i], want[i]), (kind, fl, i, int((big[i] != want[i]).sum()))
    mirt.set_frames_in_flight(1)
    loose = np.full((H, PW), 0xABCDEF01, np.uint32)
    try:
        mirt.prepared_async("raster" if kind == "raster" else "rt", views[0], L, (0.2, 0.2, 0.2), mode, loose[:, :W])()
        raise SystemExit("an unregistered surface was accepted")
    except mirt.MirtError as e:
        assert "registered" in str(e)
    mirt.surface_unregister(big)
mirt.set_depth_of_field(0)
mirt.shutdown()
print("ok")
""" % (os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpp-raytracer-rasterizer_amd"),)
    env = dict(os.environ, MIRT_HOST_PATH=path)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_rt_binned_overflowed_guess_regrows_while_the_view_stands_still(tmp_path):
    """Round-2 advisor finding: a guessed pair list that overflowed was never regrown while the view stayed the same (the
    overflow frame made the view's binning 'known', later identical frames reused its too-small list and fell back to brute
    force every time).  Here: view A (few pairs) sizes the list, then the camera jumps to view B (many pairs) and STAYS there:
    frame B1 overflows (brute force inside k_rt_trace2, rays x triangles filter evaluations), and by the time its count has
    reached the host a later frame of the same view must run binned again.  All frames equal brute force."""
    import os
    import subprocess
    import sys
    code = r"""
import sys, numpy as np
sys.path[:0] = [%r, %r]
import mirt
from devbuf import DeviceArray
mirt.init(0)
mirt.set_profiling(True)                           # (the binned kernel counts its filter evaluations only for profiled frames)
L = np.zeros((0, 7), np.float32)                   # no light: camera-only binning passes, nothing else sizes the pair list
W, H = 320, 200
tris = mirt.scene_soup(8, 20000, 0.3)           # large triangles: one tile each from afar, dozens of tiles each from close by
mirt.scene_upload(tris)
far = [mirt.make_view((0.001 * i, 0, -40.0), mirt.rot_from_yaw(0.0, 1.0), 100.0, W, H) for i in range(6)]
near = mirt.make_view((0.02, 0, -2.4), mirt.rot_from_yaw(0.01, 1.0), 100.0, W, H)
def frame(v, mode):
    b = DeviceArray((H, W), np.uint32, 0x21)
    mirt.raytrace_device(v, L, (0.2, 0.2, 0.2), mode, 0, H, 0, b.ptr, W * 4)
    st = mirt.stats()
    return b.read(), st["tests"]
want_near, _ = frame(near, mirt.RT_BRUTE)
# six far views: the first pass is sized by a read-back, the others are guessed from the far counts (a few thousand pairs)
for v in far:
    frame(v, mirt.RT_BINNED)
tests = []
for i in range(5):
    got, t = frame(near, mirt.RT_BINNED)           # (mirt.stats() waits for the frame: its count has reached the host by the next call)
    assert np.array_equal(got, want_near), "near frame %%d differs" %% i
    tests.append(t)
assert tests[0] > 100 * tests[-1] > 0, tests         # the first one overflowed into brute force ...
assert all(t < 2 * tests[-1] for t in tests[2:]), tests  # ... and from the third on the list has been regrown: binned again
# (the order inside a bin's list is not deterministic, so the counts of identical binned frames differ by a little)
mirt.shutdown()
print("ok")
""" % (os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpp-raytracer-rasterizer_amd"),
       os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MIRT_BIN_INITIAL_PAIRS="3000")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_rt_binned_pair_list_guess_overflows_into_brute_force(oracle, tmp_path):
    """A moving camera sizes the binned path's pair list from the count of an EARLIER frame, without a read-back; when a frame
    produces more pairs than that (here: the camera jumps from far away to right in front of the soup, with a list that
    starts at 1000 pairs) the sort stands down and the trace kernel renders the frame with every triangle as each tile's list
    (brute force inside k_rt_trace2) -- it must equal the brute-force frame, and the frames after it (list grown from the count
    learned meanwhile) as well.  In a child process: the first capacity is read once per process."""
    import os
    import subprocess
    import sys
    code = r"""
import sys, numpy as np
sys.path[:0] = [%r, %r]
import mirt
from devbuf import DeviceArray
mirt.init(0)
mirt.set_profiling(True)                           # (the binned kernel counts its filter evaluations only for profiled frames)
L = np.array([[0.0, -0.5, -0.7, 1, 1, 1, 14]], np.float32)
W, H = 320, 200
tris = mirt.scene_soup(8, 4000, 0.06)
mirt.scene_upload(tris)
views = [mirt.make_view((0, 0, -40.0), mirt.rot_from_yaw(0.0, 1.0), 100.0, W, H)] + \
        [mirt.make_view((0.02 * i, 0, -1.6), mirt.rot_from_yaw(0.01 * i, 1.0), 100.0, W, H) for i in range(4)]
want = []
for v in views:
    b = DeviceArray((H, W), np.uint32, 0x21)
    mirt.raytrace_device(v, L, (0.2, 0.2, 0.2), mirt.RT_BRUTE, 0, H, 0, b.ptr, W * 4)
    want.append(b.read())
got, filtered = [], []
for v in views:
    b = DeviceArray((H, W), np.uint32, 0x21)
    mirt.raytrace_device(v, L, (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, b.ptr, W * 4)
    st = mirt.stats()
    assert st["mode_used"] == mirt.RT_BINNED and st["shadow_rays"] > 0
    filtered.append(st["tests"])                  # filter evaluations of k_rt_trace2: rays x triangles when the frame fell back to brute force
    got.append(b.read())
# The first pass of a kind (here: the camera's, and the cube of a light not seen before) is sized by a read-back; the passes after it
# are guessed from its count and -- MIRT_TEST_PAIR_CAP pretends a guessed list holds 2000 pairs -- overflow: k_rt_trace2 takes every
# triangle the frame can see for every tile (hundreds of times the filter evaluations of a binned frame).  (Since round 4 the camera's
# pass is always of one kind -- the light cubes are a pass of their own --, so every view after the first is a guess here.)
assert filtered[0] > 0 and all(t > 100 * filtered[0] for t in filtered[1:]), filtered
for i, (a, b) in enumerate(zip(got, want)):
    assert np.array_equal(a, b), "view %%d differs in %%d words" %% (i, int((a != b).sum()))
lit = lambda w: int(((w != 0x21212121) & (w != 0)).sum())
assert lit(want[1]) > 20 * lit(want[0]) > 0      # the jump really multiplies the covered pixels
mirt.shutdown()
print("ok")
""" % (os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpp-raytracer-rasterizer_amd"),
       os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MIRT_BIN_INITIAL_PAIRS="1000", MIRT_TEST_PAIR_CAP="2000")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr



VARIANT_CODE = r"""
import sys, numpy as np
sys.path[:0] = [%r, %r, %r]
import mirt
from mirt_oracle import Oracle
from devbuf import DeviceArray
o = Oracle()
mirt.init(0)
L = np.array([[0.3, -0.5, -0.7, 1, 1, 1, 14], [-0.4, 0.2, -0.9, 0.5, 0.8, 1.0, 9]], np.float32)
W, H = 208, 120
def check_rt(tris, cam, mode):
    rot = o.rot_from_yaw(0.15, 1.0)
    v = mirt.make_view(cam, rot, H / 2.0, W, H)
    mirt.scene_upload(tris)
    ref = o.raytrace(tris, cam, rot, H / 2.0, W, H, L, threads=4)
    for rep in range(6):                       # the light settles into the shared cache on the way (transient, then cached tables)
        got = mirt.raytrace(v, L, mode=mode)
        assert np.array_equal(got["index"], ref["index"]) and np.array_equal(got["rgb"].view(np.uint32), ref["rgb"].view(np.uint32)) \
            and np.array_equal(got["xrgb"], ref["xrgb"]), ("ray tracer", len(tris), rep)
check_rt(mirt.scene_cornell(), (0, 0, -2), mirt.RT_AUTO)
check_rt(mirt.scene_soup(5, 3000, 0.12), (0.1, 0, -2.2), mirt.RT_BINNED)
check_rt(mirt.scene_soup(6, 300, 0.2), (0.1, 0, -2.2), mirt.RT_AUTO)
for tris in (mirt.scene_cornell(), mirt.scene_soup(7, 500, 0.3)):
    rot = o.rot_from_yaw(-0.2, 1.01)
    cam = (0.1, -0.1, -2.8)
    v = mirt.make_view(cam, rot, float(H), W, H)
    culled = mirt.cull(tris, v, 3)
    mirt.scene_upload(tris, culled)
    ref = o.rasterise(tris, culled, cam, rot, float(H), W, H, L)
    surf = np.full((H, W), 0x5A5A5A5A, np.uint32)
    mirt.surface_register(surf)
    got = mirt.rasterise(v, L, xrgb=surf)
    mirt.surface_unregister(surf)
    assert np.array_equal(got["index"], ref["index"]) and np.array_equal(got["depth"].view(np.uint32), ref["depth"].view(np.uint32)) \
        and np.array_equal(got["rgb"].view(np.uint32), ref["rgb"].view(np.uint32)) and np.array_equal(surf, ref["xrgb"]), ("rasteriser", len(tris))
mirt.shutdown()
print("ok")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("knob", ["", "MIRT_LIGHT_SHELLS=1", "MIRT_CAM_SHELLS=1", "MIRT_CUBE_BINS=64", "MIRT_CUBE_BINS=128", "MIRT_BIN_THRESHOLD=100000",
                                  "MIRT_RASTER_SMALL=0", "MIRT_RASTER_LDS_ROWS=0", "MIRT_HOST_PATH=direct", "MIRT_LAZY_GEO=1", "MIRT_BIN_REUSE=0", "MIRT_LIGHT_SIDE_STREAM=0", "MIRT_SMALL_WGS_PER_CU=1", "MIRT_BIN_WG=512", "MIRT_EDGE_SEGMENTS=0", "MIRT_EDGE_SEGMENTS=2", "MIRT_TR_WAVES5=1"])
def test_every_environment_variant_matches_the_oracle(knob):
    """Every environment variable that selects a kernel variant or a table geometry in csrc/ (each is read once per process):
    a Cornell frame (tile kernel), a binned soup (transient and cached light tables), a brute-force soup and two rasterised frames
    (small-scene path and atomic path, registered host surface) must equal the oracle bit for bit under each of them."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = VARIANT_CODE % (os.path.join(root, "cpp-raytracer-rasterizer_amd"), os.path.join(root, "oracle"), os.path.join(root, "tests"))
    env = dict(os.environ)
    if knob:
        k, v = knob.split("=")
        env[k] = v
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
