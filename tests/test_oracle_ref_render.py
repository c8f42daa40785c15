"""Pins the CPU restatement (oracle/mirt_oracle.c) to the REFERENCE'S OWN TEXT of the hot-path functions.

oracle/extract_ref.py copies the SDL-free line ranges of raytracer.cpp / rasteriser.cpp verbatim into a scratch directory,
oracle/ref_rt.cpp and oracle/ref_raster.cpp compile them against the reference's TestModel.h and the GLM it vendors (no
SDL, no stand-in), and every function is compared here with its restatement BIT FOR BIT on seeded inputs: yaw != 0, moved
cameras, several lights, soups, soft shadows, supersampling, off-screen spans, both frame sizes the reference can render.
The libraries are built in the build container (oracle/Makefile, target `ref`) and travel prebuilt to the GPU box; where
they are absent the module is skipped and tests/test_golden_ref_render.py (recorded outputs of the same cases) stands in.

Still NOT covered by this pin, because their text names an SDL type (they stay on SURVEY Appendix C's recorded hashes,
tests/test_oracle_pin.py): PutPixelSDL (SDLauxiliary.h:70-81), the surface clear in the rasteriser's Update() (:183-192).
"""
import ctypes

import numpy as np
import pytest

import ref_render
from ref_cases import RT_CASES, RASTER_CASES, build_scene, lights_array, reference_asset

pytestmark = pytest.mark.skipif(not ref_render.available(), reason="oracle/_ref not built (needs /root/reference; make -C oracle ref)")

FLT_MAX = np.finfo(np.float32).max


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def refs():
    return {500: ref_render.RefRayTracer(500), 150: ref_render.RefRayTracer(150)}


@pytest.fixture(scope="module")
def raster():
    return ref_render.RefRasteriser()


# ---- ray tracer --------------------------------------------------------------------------------------------------------

def test_reference_sizes_and_defaults(refs):
    """The two builds carry the reference's own constants (raytracer.cpp:59-71)."""
    assert refs[500].default_focal == 250.0 and refs[500].default_cam.tolist() == [0.0, 0.0, -2.0]
    assert refs[150].default_focal == 250.0 and np.allclose(refs[150].default_cam, [0.0, 0.0, -4.3])


def test_load_test_model(oracle, refs, raster):
    for r in (refs[500], refs[150], raster):
        assert same(r.load_test_model(), oracle.cornell())


@pytest.mark.parametrize("yaw", [0.0, 0.1, -0.1, 0.3, -1.1, 2.9, 12.5])
def test_camera_rotation_from_yaw(oracle, refs, yaw):
    """Update() :377-382 (cosf / sinf of the float yaw) == mirt_oracle_rot_from_yaw."""
    assert same(refs[500].set_view((0, 0, -2), yaw, 250.0), oracle.rot_from_yaw(yaw, 1.0))


def test_add_light_jitter_matches_rand_stream(oracle, refs):
    """AddLight (:180-193) draws its jitter from rand(); the restatement reproduces the draw order of the reference's
    compiler (the three RandomNumber() calls of one constructor call)."""
    r = refs[150]
    for samples, lights in ((16, [[0, -0.5, -0.7, 1, 1, 1, 14]]), (4, [[0.3, 0.2, -0.9, 1, 1, 1, 5], [-0.4, 0.1, 0.3, 1, 1, 1, 7]])):
        r.set_options(soft=samples)
        got = r.set_lights(np.array(lights, np.float32), seed=1)
        ctypes.CDLL(None).srand(1)
        want = np.concatenate([oracle.jitter(np.array(l[:3], np.float32), samples) for l in lights])
        assert same(got, want)
    r.set_options(soft=1)


@pytest.mark.parametrize("scene", [("cornell",), ("soup", 21, 700, 0.3), ("cornell+soup", 22, 64, 0.5)])
def test_closest_intersection_function(oracle, refs, scene):
    """ClosestIntersection :202-257 call by call: accept decision, position, distance and index, including the in/out
    record (a later call must only replace a record that is at least as far: the `>=` rule)."""
    r = refs[500]
    tris = build_scene(oracle, scene)
    r.set_scene(tris)
    rng = np.random.RandomState(5)
    hits = 0
    for k in range(400):
        start = rng.uniform(-1.5, 1.5, 3).astype(np.float32) if k % 3 else np.array([0, 0, -2], np.float32)
        d = rng.uniform(-1, 1, 3).astype(np.float32)
        if k % 5 == 0:                                            # aim at a vertex / an edge midpoint: exact ties and edge cases
            t = tris[rng.randint(len(tris))]
            d = ((t[0:3] if k % 10 else (t[0:3] + t[3:6]) * np.float32(0.5)) - start).astype(np.float32)
        rec = dict(pos=(0, 0, 0), distance=FLT_MAX, index=-1) if k % 4 else dict(pos=(1, 2, 3), distance=np.float32(rng.uniform(0.5, 3)), index=7)
        a = r.closest(start, d, is_light=True, **rec)
        b = oracle.closest_intersection(tris, start, d, **rec)
        assert a[0] == b[0] and same(a[1], b[1]) and same(a[2], b[2]) and a[3] == b[3], "call %d differs: %r vs %r" % (k, a, b)
        hits += a[0]
    assert hits > 100


@pytest.mark.parametrize("nl,samples", [(1, 1), (3, 1), (1, 16), (2, 4)])
def test_direct_light_function(oracle, refs, nl, samples):
    """DirectLight :265-327 on real hit records: light term, shadow test from the light, result2 += result quirk,
    soft-shadow positions."""
    r = refs[150]
    tris = build_scene(oracle, ("cornell+soup", 3, 200, 0.25))
    lights = lights_array([[0, -0.5, -0.7, 1, 1, 1, 14], [0.5, 0.3, -0.9, 1, 0.5, 0.2, 6], [-0.6, -0.2, 0.1, 0.3, 0.9, 0.4, 9]][:nl])
    r.set_scene(tris)
    r.set_options(soft=samples)
    jitter = r.set_lights(lights, seed=3)
    rng = np.random.RandomState(11)
    n = 0
    while n < 150:
        d = rng.uniform(-1, 1, 3).astype(np.float32)
        any_, pos, dist, idx = oracle.closest_intersection(tris, (0, 0, -2), d)
        if not any_:
            continue
        n += 1
        got = r.direct_light(pos, dist, idx)
        want = oracle.direct_light(tris, pos, dist, idx, lights, samples=samples, jitter=jitter if samples > 1 else None)
        assert same(got, want), "hit %d on triangle %d: %r vs %r" % (n, idx, got, want)
    r.set_options(soft=1)


@pytest.mark.parametrize("name", sorted(RT_CASES))
def test_draw_frame(oracle, refs, name):
    """Update()'s reset + Draw() :547-603 over a whole frame: closestIntersections (index, distance, position),
    pixelColours and focalDistances, bit for bit."""
    c = RT_CASES[name]
    r = refs[c["size"]]
    S = c["size"]
    tris = build_scene(oracle, c["scene"])
    lights = lights_array(c["lights"])
    r.set_scene(tris)
    rot = r.set_view(c["cam"], c["yaw"], c["focal"])
    r.set_options(aa=c["aa"], soft=c["soft"], focal_plane=1.3, threads=8)
    jitter = r.set_lights(lights, seed=1)
    got = r.draw()
    r.set_options()
    want = oracle.raytrace(tris, c["cam"], rot, c["focal"], S, S, lights, threads=8, samples=c["soft"],
                           jitter=jitter if c["soft"] > 1 else None, aa=c["aa"])
    assert np.array_equal(got["index"], want["index"]), "index differs in %d pixels" % int((got["index"] != want["index"]).sum())
    assert same(got["dist"], want["dist"]) and same(got["pos"], want["pos"])
    assert same(got["rgb"], want["rgb"])
    fd = np.where(want["index"] >= 0, want["dist"] - np.float32(1.3), np.float32(0)).astype(np.float32)      # raytracer.cpp:248-249
    assert same(got["fd"], fd)
    assert 0 < int((got["index"] >= 0).sum())


@pytest.mark.parametrize("size", [500, 150])
def test_depth_of_field_blur_loops(oracle, refs, size):
    """CalculateDOF's blur :613-645 (DOF_KERNEL_SIZE 8) on random planes.  Compared where every tap is inside the frame:
    beyond it the reference reads past its arrays (undefined behaviour, documented divergence)."""
    r = refs[size]
    rng = np.random.RandomState(2)
    rgb = rng.uniform(0, 1.5, (size, size, 3)).astype(np.float32)
    fd = rng.uniform(-1.6, 1.6, (size, size)).astype(np.float32)
    r.set_options(dof=8)
    got = r.blur(rgb, fd)
    r.set_options()
    want = oracle.dof_float(rgb, fd, 8)
    assert same(got[4:size - 4, 1:size - 1], want[4:size - 4, 1:size - 1])


# ---- rasteriser --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("yaw,cam", [(0.0, (0, 0, -3)), (0.6, (0.4, -0.2, -2.5)), (-2.8, (0.1, 0.3, 1.0))])
def test_update_camera_and_cull(oracle, raster, flags, yaw, cam):
    """Update() :377-447 + InCuboid :451-458: cameraRot from yaw (with cameraRot[1][1] = 1.01) and isCulled per triangle."""
    for scene in (("cornell",), ("soup", 5, 5000, 0.3)):
        tris = build_scene(oracle, scene)
        raster.set_scene(tris)
        rot, culled = raster.update(cam, yaw, 500.0, 1.01, backface=flags & 1, frustum=flags & 2)
        assert same(rot, oracle.rot_from_yaw(yaw, 1.01))
        assert np.array_equal(culled, oracle.cull(tris, cam, rot, 500.0, 500, 500, flags))


def test_vertex_shader_function(oracle, raster):
    """VertexShader :532-546: pos3d, zinv and the truncated screen coordinates."""
    raster.set_scene(oracle.cornell())
    rng = np.random.RandomState(8)
    for k in range(300):
        cam = (0.3, -0.1, -2.7) if k % 2 else (0, 0, -3)
        yaw = 0.0 if k % 3 == 0 else float(rng.uniform(-0.6, 0.6))
        rot, _ = raster.update(cam, yaw, 500.0, 1.01)
        v = rng.uniform(-1, 1, 3).astype(np.float32)
        x, y, zinv, p3 = raster.vertex_shader(v)
        ox, oy, oz, op = oracle.vertex_shader(v, cam, rot, 500.0, 500, 500)
        assert (x, y) == (ox, oy) and same(zinv, np.float32(oz)) and same(p3, op)


@pytest.mark.parametrize("name", sorted(RASTER_CASES))
def test_rasterise_frame(oracle, raster, name):
    """Clear + Draw()'s triangle loop :466-479 -> DrawPolygon, ComputePolygonRows, Interpolate, DrawRows, DrawLineSDL's
    body, Bresenham, PixelShader: depthBuffer, pixelColours and focalDistances of the whole frame, bit for bit -- views
    with spans that leave the screen included (uninitialised Pixels there are filled as MALLOC_PERTURB_=165 would)."""
    c = RASTER_CASES[name]
    tris = build_scene(oracle, c["scene"])
    lights = lights_array(c["lights"])
    raster.set_scene(tris)
    raster.set_lights(lights)
    rot, culled = raster.update(c["cam"], c["yaw"], c["focal"], c["rot11"], backface=c["flags"] & 1, frustum=c["flags"] & 2,
                                focal_plane=c["focal_plane"])
    got = raster.draw()
    want = oracle.rasterise(tris, culled, c["cam"], rot, c["focal"], 500, 500, lights, want=("rgb", "index", "fd"), focal_plane=c["focal_plane"])
    assert same(got["depth"], want["depth"]), "depthBuffer differs in %d pixels" % int((bits(got["depth"]) != bits(want["depth"])).sum())
    assert same(got["rgb"], want["rgb"]), "pixelColours differ in %d pixels" % int((bits(got["rgb"]) != bits(want["rgb"])).any(axis=2).sum())
    assert same(got["fd"], want["fd"])
    assert int((got["depth"] > 0).sum()) > 1000


@pytest.mark.parametrize("K", [8, 3])
def test_raster_depth_of_field_blur_loops(oracle, raster, K):
    rng = np.random.RandomState(4)
    rgb = rng.uniform(0, 1.5, (500, 500, 3)).astype(np.float32)
    fd = rng.uniform(-1.6, 1.6, (500, 500)).astype(np.float32)
    got = raster.blur(rgb, fd, K)
    want = oracle.dof_float(rgb, fd, K)
    assert same(got[4:496, 1:499], want[4:496, 1:499])


def test_stl_loader_on_the_reference_asset(oracle, raster, tmp_path):
    """LoadSTL::LoadSTLFile (LoadSTL.cpp:17-97) run on the reference's own mesh == the restated loader, bit for bit."""
    path = reference_asset(tmp_path)
    got = raster.load_stl(str(tmp_path))
    want = oracle.load_stl(path)
    assert got.shape == want.shape == (9028, 15)
    assert np.array_equal(bits(got), bits(want))
