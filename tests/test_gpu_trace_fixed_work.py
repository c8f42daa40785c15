"""The once-per-wave blocks of the binned trace kernel (csrc/rt_trace.hip): the stores behind the TRF_PLANES flag, the lights' loop
with one sample per light and with several, the light-cube offsets asked for by every lane, the record merge, the one-wave workgroup.

A seeded soup of 300 triangles (more than 64, so RT_BINNED runs k_rt_trace2) in a frame of 72 x 43 pixels -- nine tile columns, so
the last pair of a row has no second tile, and a height that is no multiple of eight -- rendered whole and as the band of rows
5 .. 38.  Every frame goes through the device entry point into planes pre-filled with a byte pattern and is compared bit for bit:
the XRGB-only call against the call with the four planes a caller can pass (rgb, index and the two intersection planes), and both
against RT_BRUTE.  The fifth optional plane, fd (focalDistances), is the library's own: a frame rendered with depth of field on
(mirt.set_depth_of_field) gets it, together with the library's rgb plane, beside whatever the caller passes -- so with the four
caller planes such a frame stores all five, and what was stored in fd shows in the blurred XRGB, which is compared bit for bit with
RT_BRUTE's under the same setting.  (No entry point renders a frame whose ONLY optional plane is fd: under depth of field rgb is
always there too.  tests/cpp/trace_flags_test.cpp covers that combination of the flags word on the host.)  Nothing is skipped: a
frame that was not rendered by the binned path, or a scene that does not show what the case is about, fails.
"""
import numpy as np
import pytest

import mirt
from devbuf import DeviceArray
from mirt_oracle import DEFAULT_LIGHT

pytestmark = pytest.mark.gpu

W, H = 72, 43
BAND = (5, 38)
CAM = (0.0, 0.0, -3.0)
FOCAL = 56.0                                     # the soup, two to four units away, fills most of the frame and leaves gaps
PLANES = ("rgb", "index", "dist", "pos")         # what a caller can pass; fd comes with depth of field (DOF)
DOF = (5, 1.3)                                   # blur kernel size and focal length: the frame then stores fd and rgb for the blur
FILL = 0x11
FILL_WORD = 0x11111111


def soup(n=300, seed=20261):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (n, 1, 3))
    v = (c + rng.uniform(-0.22, 0.22, (n, 3, 3))).astype(np.float32)
    t = np.zeros((n, 15), np.float32)
    t[:, 0:9] = v.reshape(n, 9)
    nrm = np.cross(v[:, 2] - v[:, 0], v[:, 1] - v[:, 0])
    t[:, 9:12] = nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    t[:, 12:15] = rng.uniform(0.15, 0.75, (n, 3))
    return t


def light(x, y, z, power):
    return [x, y, z, 1.0, 0.9, 0.8, power]


ONE = np.array(DEFAULT_LIGHT, np.float32)
TWO = np.array([DEFAULT_LIGHT[0], light(0.9, 0.4, -1.6, 9.0)], np.float32)
THREE = np.array([DEFAULT_LIGHT[0], light(0.9, 0.4, -1.6, 9.0), light(-1.1, -0.8, 0.3, 11.0)], np.float32)
NONE = np.zeros((0, 7), np.float32)
# (lights, soft-shadow samples).  One sample per light -- one, two or three lights -- is the path without a count (TRF_ONE_SAMPLE): the
# sum is closed at every light position.  Two samples per light count down: one light closes its sum once, at the second position;
# two lights x two samples (four positions) close it twice, so the count is also set up again for the second light.
LIGHTS = {"one-light": (ONE, 1), "one-light-two-samples": (ONE, 2), "two-lights": (TWO, 1), "three-lights": (THREE, 1), "no-light": (NONE, 1),
          "two-lights-two-samples": (TWO, 2)}


def jitter(lights, samples):
    """The positions the shadow rays of a soft light start from: `samples` per light, around it."""
    rng = np.random.default_rng(77)
    return (np.repeat(lights[:, 0:3], samples, axis=0) + rng.uniform(-0.08, 0.08, (len(lights) * samples, 3))).astype(np.float32)


def view_of(yaw=0.0):
    return mirt.make_view(CAM, mirt.rot_from_yaw(yaw, 1.0), FOCAL, W, H)


def render(mode, lights, band, planes, yaw=0.0):
    """One frame or band; `planes`: the optional planes asked for besides XRGB.  Returns the planes read back."""
    y0, y1 = band if band else (0, H)
    bufs = {"xrgb": DeviceArray((H, W), np.uint32, FILL)}
    shapes = {"rgb": ((H, W, 3), np.float32), "index": ((H, W), np.int32), "dist": ((H, W), np.float32), "pos": ((H, W, 3), np.float32)}
    for k in planes:
        bufs[k] = DeviceArray(shapes[k][0], shapes[k][1], FILL)
    try:
        mirt.raytrace_device(view_of(yaw), lights, (0.2, 0.2, 0.2), mode, y0, y1, 0, bufs["xrgb"].ptr, W * 4,
                             **{"d_" + k: bufs[k].ptr for k in planes})
        st = mirt.stats()
        assert st["mode_used"] == mode, "rendered by mode %d, not by %d" % (st["mode_used"], mode)
        return {k: b.read() for k, b in bufs.items()}
    finally:
        for b in bufs.values():
            b.free()


def reset():
    mirt.set_depth_of_field(0)
    mirt.set_soft_shadows(1)
    mirt.set_antialiasing(1)
    mirt.set_profiling(False)
    mirt.set_frames_in_flight(1)


def apply(lights_name, aa, dof=None):
    lights, samples = LIGHTS[lights_name]
    mirt.set_antialiasing(aa)
    if dof:
        mirt.set_depth_of_field(*dof)
    mirt.set_soft_shadows(samples, jitter(lights, samples) if samples > 1 else None)
    return lights


_brute = {}


def brute(lights_name, band, aa=1, yaw=0.0, dof=None):
    """The brute-force frame with the four caller planes (and, with `dof`, fd behind the blur): once per case, shared, never changed."""
    key = (lights_name, band, aa, yaw, dof)
    if key not in _brute:
        reset()
        ref = render(mirt.RT_BRUTE, apply(lights_name, aa, dof), band, PLANES, yaw)
        for a in ref.values():
            a.setflags(write=False)
        _brute[key] = ref
    return _brute[key]


def same_bits(got, want, keys, what):
    for k in keys:
        a, b = got[k].view(np.uint32), want[k].view(np.uint32)
        assert np.array_equal(a, b), "%s: %s differs in %d words" % (what, k, int((a != b).sum()))


def check(lights_name, band, flight, aa=1, yaw=0.0, profiled=False, dof=None):
    """XRGB-only == the four caller planes == brute force, `flight` frames in flight (one: the five-wave instantiation; four: the
    four-wave one).  With `dof` every frame also stores fd and the library's rgb (the XRGB-only call: those two alone), and XRGB is
    the blurred frame."""
    want = brute(lights_name, band, aa, yaw, dof)
    try:
        lights = apply(lights_name, aa, dof)
        mirt.set_frames_in_flight(flight)
        mirt.set_profiling(profiled)
        what = "%s, band %s, %d in flight, aa %d, dof %s" % (lights_name, band, flight, aa, dof)
        for _ in range(flight):                                   # (each stream runs a pass of its own)
            only = render(mirt.RT_BINNED, lights, band, (), yaw)
            full = render(mirt.RT_BINNED, lights, band, PLANES, yaw)
            same_bits(only, full, ("xrgb",), what + ": XRGB only against the caller's four planes")
            same_bits(full, want, ("xrgb",) + PLANES, what + ": binned against brute force")
            for k in ("rgb", "index"):                           # (the four- and five-argument entry point: some planes, not all)
                some = render(mirt.RT_BINNED, lights, band, (k,), yaw)
                same_bits(some, want, ("xrgb", k), what + ": XRGB and %s" % k)
        return want
    finally:
        reset()


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    mirt.scene_upload(soup())
    yield
    reset()
    mirt.shutdown()


def rows_of(band):
    return slice(*band) if band else slice(None)


def test_the_scene_is_what_the_cases_need():
    """Hits and misses in the frame, in its last tile column and in its last, partial tile row; lit and shadowed hits; and the
    lights' cases differ from each other, so that a frame accumulated the wrong way cannot pass for the right one."""
    ref = {k: brute(k, None) for k in LIGHTS}
    idx = ref["one-light"]["index"]
    assert (idx >= 0).sum() > 500 and (idx < 0).sum() > 50
    assert (idx[:, 64:] >= 0).any() and (idx[40:, :] >= 0).any()
    assert (ref["one-light"]["xrgb"] == FILL_WORD).all(axis=1)[[0, H - 1]].all(), "the frame's border rows are not stored (:618-620)"
    lit = (ref["one-light"]["rgb"] != ref["no-light"]["rgb"]).any(axis=2)
    hit = idx >= 0
    assert (lit & hit).sum() > 100 and (~lit & hit).sum() > 20, "no pixel in light or none in shadow"
    names = sorted(LIGHTS)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not np.array_equal(ref[a]["xrgb"], ref[b]["xrgb"]), (a, b)
    band = brute("one-light", BAND)
    assert (band["xrgb"][:BAND[0]] == FILL_WORD).all() and (band["xrgb"][BAND[1]:] == FILL_WORD).all()
    assert (band["index"][rows_of(BAND)] >= 0).sum() > 400


@pytest.mark.parametrize("flight", [1, 4])
@pytest.mark.parametrize("band", [None, BAND], ids=["whole", "band-5-38"])
@pytest.mark.parametrize("lights_name", ["one-light", "one-light-two-samples", "two-lights", "three-lights", "two-lights-two-samples"])
def test_planes_and_lights(lights_name, band, flight):
    check(lights_name, band, flight)


@pytest.mark.parametrize("band", [None, BAND], ids=["whole", "band-5-38"])
def test_no_light_at_all(band):
    want = check("no-light", band, 1)
    assert (want["index"][rows_of(band)] >= 0).sum() > 400
    check("no-light", band, 4)


@pytest.mark.parametrize("aa", [1, 2])
@pytest.mark.parametrize("band", [None, BAND], ids=["whole", "band-5-38"])
def test_a_view_that_sees_no_triangle(band, aa):
    """The camera turned away from the soup: every pair's lists are empty; with supersampling 2 the AA instantiations."""
    want = check("one-light", band, 1, aa=aa, yaw=np.pi)
    assert (want["index"][rows_of(band)] == -1).all(), "the view was to see nothing"
    assert (want["dist"][rows_of(band)] == np.float32(3.402823466e+38)).all()
    check("one-light", band, 4, aa=aa, yaw=np.pi)


@pytest.mark.parametrize("lights_name", ["one-light", "one-light-two-samples", "three-lights"])
def test_supersampled_and_profiled_instantiations(lights_name):
    """The same comparisons through the instantiations that carry a second set of sub-ray state and the kernel's own counts."""
    check(lights_name, None, 1, aa=2)
    check(lights_name, BAND, 4, aa=2)
    check(lights_name, None, 1, profiled=True)
    check(lights_name, BAND, 1, aa=2, profiled=True)


def test_depth_of_field_is_what_the_fd_cases_need():
    """The blur moves the frame, and what it does depends on fd: another focal length gives another frame."""
    plain, blurred = brute("one-light", None), brute("one-light", None, dof=DOF)
    other = brute("one-light", None, dof=(DOF[0], 2.6))
    assert not np.array_equal(plain["xrgb"], blurred["xrgb"]) and not np.array_equal(blurred["xrgb"], other["xrgb"])
    same_bits(plain, blurred, PLANES, "the planes beside XRGB stay the un-blurred ones")


@pytest.mark.parametrize("flight", [1, 4])
@pytest.mark.parametrize("band", [None, BAND], ids=["whole", "band-5-38"])
def test_fd_plane_behind_the_blur(band, flight):
    """All five optional planes in one frame (fd and rgb for the blur, the caller's four), and fd with rgb alone."""
    check("one-light", band, flight, dof=DOF)


@pytest.mark.parametrize("band", [None, BAND], ids=["whole", "band-5-38"])
def test_fd_plane_supersampled_and_profiled(band):
    check("one-light", band, 1, aa=2, dof=DOF)
    check("one-light", band, 4, aa=2, dof=DOF)
    check("one-light", band, 1, profiled=True, dof=DOF)
    check("one-light", band, 1, aa=2, profiled=True, dof=DOF)
    check("two-lights-two-samples", band, 4, dof=DOF)
