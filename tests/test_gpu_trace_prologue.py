"""The fixed per-wave work of the binned frame: the trace kernel's record lookup (csrc/rt_trace.hip: the wave's XCD group, its
class among the group's eight, its record -- all on the scalar unit, tile column and row packed into one word) and k_bs_local's
trip counts taken from the bucket's size (csrc/bin_bucket_sort.hip).

Every case renders a frame with RT_BINNED and with RT_BRUTE through the device entry point and compares XRGB, index, distance and
position bit for bit, under four settings: one frame in flight (the five-waves-per-SIMD instantiation of k_rt_trace2), four in
flight (the four-wave one), supersampling 2 x 2, and profiling on (the instantiation that keeps the kernel's own counts).

The scenes are stacks of small triangles placed over chosen 8 x 8-pixel tiles (camera on the z axis, identity rotation: pixel
(x, y) looks at ((x - W/2) d / f, (y - H/2) d / f, d - 2) at depth d), so the list length of every tile pair -- and with it the
class its record is filed under and the size of the sort bucket its pairs land in -- is known.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import mirt
from devbuf import DeviceArray
from mirt_oracle import DEFAULT_LIGHT

pytestmark = pytest.mark.gpu

SETTINGS = ["one-in-flight", "four-in-flight", "supersampled", "profiled"]
CAM = (0.0, 0.0, -2.0)


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_frames_in_flight(1)
    mirt.shutdown()


def _focal(H):
    return H / 2.0


def stack(W, H, tx, ty, count, depth0=2.0, seed=0):
    """`count` triangles inside tile (tx, ty) of a W x H frame (pixels 1.2 .. 6.8 of the tile's 8 in each direction, so the
    neighbouring tiles' lists stay as they are), 1e-3 apart in depth from depth0 on; colours from `seed`."""
    rng = np.random.default_rng(1000 * seed + 64 * ty + tx)
    f = _focal(H)
    d = depth0 + 1.0e-3 * np.arange(count, dtype=np.float64)
    # three corners per triangle, in pixels relative to the tile: a random sub-triangle of the inner square
    c = rng.uniform(1.2, 6.8, (count, 3, 2))
    c[0] = [[1.2, 1.2], [6.8, 1.2], [1.2, 6.8]]          # (the nearest one a fixed half of the square: every stack is seen)
    px = 8 * tx + c[:, :, 0] - W / 2.0
    py = 8 * ty + c[:, :, 1] - H / 2.0
    t = np.zeros((count, 15), np.float32)
    for k in range(3):
        t[:, 3 * k + 0] = px[:, k] * d / f
        t[:, 3 * k + 1] = py[:, k] * d / f
        t[:, 3 * k + 2] = d - 2.0
    e1 = t[:, 3:6] - t[:, 0:3]
    e2 = t[:, 6:9] - t[:, 0:3]
    n = np.cross(e2, e1)
    t[:, 9:12] = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    t[:, 12:15] = rng.uniform(0.15, 0.75, (count, 3))
    return t


def scene_ragged_72x40():
    """9 x 5 tiles: the last pair of a row has no second tile; XCD groups 2..7 have no pairs (tile rows 0..3 and 4)."""
    W, H = 72, 40
    parts = [mirt.scene_soup(7, 600, 0.2)]
    parts += [stack(W, H, 8, ty, 5 + 9 * ty, seed=1) for ty in range(5)]        # the lone last tile of every row
    return W, H, np.concatenate(parts), None


def scene_tall_64x264():
    """8 x 33 tiles: stripes of four tile rows dealt to eight groups -- the ninth stripe wraps round to group 0."""
    W, H = 64, 264
    parts = [mirt.scene_soup(9, 900, 0.25)]
    parts += [stack(W, H, (3 * ty) % 8, ty, 3 + (7 * ty) % 40, seed=2) for ty in range(33)]
    return W, H, np.concatenate(parts), None


def scene_tall_band():
    W, H, tris, _ = scene_tall_64x264()
    return W, H, tris, (13, 29)


def scene_every_class():
    """16 c + 1 triangles over the first tile of pair c (and c over its second), c = 0..7, on a 64 x 16 frame: two tile rows of
    four pairs, all of one group -- every class of that group holds exactly one record, the open-ended last class included."""
    W, H = 64, 16
    parts = []
    for c in range(8):
        tx, ty = 2 * (c % 4), c // 4
        parts.append(stack(W, H, tx, ty, 16 * c + 1, seed=3))
        if c:
            parts.append(stack(W, H, tx + 1, ty, c, seed=4))
    return W, H, np.concatenate(parts), None


def scene_big_bucket():
    """5000 triangles over one tile: one sort key, so a bucket above the 4096 pairs k_bs_local keeps in registers."""
    W, H = 72, 40
    return W, H, np.concatenate([stack(W, H, 4, 2, 5000, seed=5), stack(W, H, 1, 1, 3, seed=5)]), None


def scene_bucket_sizes():
    """256, 257 and 4096 pairs in single buckets (one full round of 256 threads, one pair more, the most the register-resident
    path takes), every other bucket of the 64 x 264 frame empty."""
    W, H = 64, 264
    return W, H, np.concatenate([stack(W, H, 0, 0, 256, seed=6), stack(W, H, 2, 10, 257, seed=6), stack(W, H, 5, 21, 4096, seed=6)]), None


SCENES = {
    "ragged-72x40": scene_ragged_72x40,
    "tall-64x264": scene_tall_64x264,
    "band-13-29": scene_tall_band,
    "every-class": scene_every_class,
    "bucket-above-4096": scene_big_bucket,
    "buckets-256-257-4096": scene_bucket_sizes,
}

_built = {}
_brute = {}


def _scene(name):
    if name not in _built:
        _built[name] = SCENES[name]()
    return _built[name]


def render(tris, W, H, band, mode, lights=DEFAULT_LIGHT, view=None):
    """One frame (or band) into device planes pre-filled with 0x11 bytes; returns (planes, stats)."""
    y0, y1 = band if band else (0, H)
    if view is None:
        view = mirt.make_view(CAM, mirt.rot_from_yaw(0.0, 1.0), _focal(H), W, H)
    planes = {"xrgb": DeviceArray((H, W), np.uint32, 0x11), "index": DeviceArray((H, W), np.int32, 0x11),
              "dist": DeviceArray((H, W), np.float32, 0x11), "pos": DeviceArray((H, W, 3), np.float32, 0x11)}
    try:
        mirt.raytrace_device(view, lights, (0.2, 0.2, 0.2), mode, y0, y1, 0, planes["xrgb"].ptr, W * 4,
                             d_index=planes["index"].ptr, d_dist=planes["dist"].ptr, d_pos=planes["pos"].ptr)
        st = mirt.stats()
        out = {k: p.read() for k, p in planes.items()}
    finally:
        for p in planes.values():
            p.free()
    return out, st


def apply_setting(setting):
    mirt.set_frames_in_flight(4 if setting == "four-in-flight" else 1)
    mirt.set_antialiasing(2 if setting == "supersampled" else 1)
    mirt.set_profiling(setting == "profiled")


def reset_settings():
    mirt.set_profiling(False)
    mirt.set_antialiasing(1)
    mirt.set_frames_in_flight(1)


def assert_same_bits(got, want, what):
    for k in ("xrgb", "index", "dist", "pos"):
        a, b = got[k].view(np.uint32), want[k].view(np.uint32)
        assert np.array_equal(a, b), "%s: %s differs in %d words" % (what, k, int((a != b).sum()))


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_binned_frame_equals_brute_force(name, setting):
    W, H, tris, band = _scene(name)
    aa = 2 if setting == "supersampled" else 1
    mirt.scene_upload(tris)
    try:
        if (name, aa) not in _brute:                      # the reference frame: once per scene and sampling, shared, never changed
            mirt.set_antialiasing(aa)
            ref, st = render(tris, W, H, band, mirt.RT_BRUTE)
            assert st["mode_used"] == mirt.RT_BRUTE
            assert (ref["index"][slice(*band) if band else slice(None)] >= 0).any(), "the scene is not in front of the camera"
            for a in ref.values():
                a.setflags(write=False)
            _brute[(name, aa)] = ref
        apply_setting(setting)
        got, st = render(tris, W, H, band, mirt.RT_BINNED)
        assert st["mode_used"] == mirt.RT_BINNED
        assert_same_bits(got, _brute[(name, aa)], "%s, %s" % (name, setting))
        if setting == "four-in-flight":                   # the other three streams have held no pass yet: each runs its own
            for _ in range(3):
                got, st = render(tris, W, H, band, mirt.RT_BINNED)
                assert st["mode_used"] == mirt.RT_BINNED
                assert_same_bits(got, _brute[(name, aa)], "%s, %s" % (name, setting))
    finally:
        reset_settings()


def test_stacks_land_on_their_tiles():
    """The scenes above mean what they say only if a stack covers pixels of its own tile and of no other: the closest hit of
    the every-class scene lies inside the inner square of the tile each stack was built over."""
    W, H, tris, _ = _scene("every-class")
    mirt.scene_upload(tris)
    ref, _ = render(tris, W, H, None, mirt.RT_BRUTE)
    owner, first = np.full(len(tris), -1), 0
    for c in range(8):
        for tile, count in ((2 * (c % 4) + 8 * (c // 4), 16 * c + 1), (2 * (c % 4) + 1 + 8 * (c // 4), c if c else 0)):
            owner[first:first + count] = tile
            first += count
    assert first == len(tris)
    ys, xs = np.nonzero(ref["index"] >= 0)
    assert len(ys) > 8 * 8
    assert np.array_equal(owner[ref["index"][ys, xs]], (ys // 8) * 8 + xs // 8)
    assert set(owner[ref["index"][ys, xs]]) == set(range(16)) - {1}       # (pair 0 has nothing over its second tile)


OVERFLOW_CODE = r"""
import sys, numpy as np
sys.path[:0] = [%r, %r]
import mirt
from devbuf import DeviceArray
mirt.init(0)
L = np.array([[0.0, -0.5, -0.7, 1, 1, 1, 14]], np.float32)
W, H = 136, 72                                       # 17 x 9 tiles: the last pair of a row has no second tile
tris = mirt.scene_soup(8, 4000, 0.06)
mirt.scene_upload(tris)
views = [mirt.make_view((0, 0, -40.0), mirt.rot_from_yaw(0.0, 1.0), 36.0, W, H)] + \
        [mirt.make_view((0.02 * i, 0, -1.6), mirt.rot_from_yaw(0.01 * i, 1.0), 36.0, W, H) for i in range(4)]
KEYS = ("xrgb", "index", "dist", "pos")
def frame(v, mode):
    p = {"xrgb": DeviceArray((H, W), np.uint32, 0x21), "index": DeviceArray((H, W), np.int32, 0x21),
         "dist": DeviceArray((H, W), np.float32, 0x21), "pos": DeviceArray((H, W, 3), np.float32, 0x21)}
    mirt.raytrace_device(v, L, (0.2, 0.2, 0.2), mode, 0, H, 0, p["xrgb"].ptr, W * 4, d_index=p["index"].ptr, d_dist=p["dist"].ptr, d_pos=p["pos"].ptr)
    st = mirt.stats()
    out = {k: p[k].read().view(np.uint32) for k in KEYS}
    for b in p.values():
        b.free()
    return out, st
# The first pass of a kind is sized by a read-back; the passes after it are guessed from its count, and MIRT_TEST_PAIR_CAP pretends a
# guessed list holds 2000 pairs: every view after the first overflows and k_rt_trace2 takes the selection as each tile's list.
for setting in ("profiled", "one-in-flight", "four-in-flight", "supersampled"):
    aa = 2 if setting == "supersampled" else 1
    mirt.set_frames_in_flight(1); mirt.set_profiling(False); mirt.set_antialiasing(aa)
    want = [frame(v, mirt.RT_BRUTE)[0] for v in views]
    mirt.set_frames_in_flight(4 if setting == "four-in-flight" else 1)
    mirt.set_profiling(setting == "profiled")
    order = range(len(views)) if setting == "profiled" else [1, 2, 3, 4, 0, 1, 2, 3, 4]
    for n, i in enumerate(order):
        got, st = frame(views[i], mirt.RT_BINNED)
        assert st["mode_used"] == mirt.RT_BINNED and st["shadow_rays"] > 0
        for k in KEYS:
            assert np.array_equal(got[k], want[i][k]), "%%s: view %%d: %%s differs in %%d words" %% (setting, i, k, int((got[k] != want[i][k]).sum()))
        if setting == "profiled":
            # candidates offered to primary rays (counted for profiled frames): an overflowed frame offers every selected triangle to
            # every pixel, a binned one only its tile's list -- fewer, unless every tile held every triangle
            whole = W * H * st["selected_triangles"]
            assert st["selected_triangles"] > 0
            assert (st["candidates"] >= whole) == (n > 0), (n, st["candidates"], whole)
mirt.shutdown()
print("ok")
"""


def test_overflowed_pair_list_takes_the_selection_count():
    """A frame whose pair list overflowed renders every tile pair against the triangles k_prep_select kept (sel_count, read with
    the wave's other counters): a moving camera with a list that pretends to hold 2000 pairs, under all four settings.  In a child
    process: the capacities are read once per process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = OVERFLOW_CODE % (os.path.join(root, "cpp-raytracer-rasterizer_amd"), os.path.join(root, "tests"))
    env = dict(os.environ, MIRT_BIN_INITIAL_PAIRS="1000", MIRT_TEST_PAIR_CAP="2000")
    mirt.shutdown()                      # the child process owns the GPU context for this test
    try:
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    finally:
        mirt.init(0)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
