"""The binned trace kernel's shadow rays (csrc/rt_trace.hip): a pixel whose light term D is exactly zero gets no shadow ray
(shadow_ray_needed, csrc/rt_common.hpp), and the rays that are needed are dealt over the lanes of the wave -- slot l and slot l + 64
of the wave's ray table -- so a lane walks the rays of other lanes' pixels and reports an occluder through the pixel's flag byte.

Scenes of more than 64 triangles (so that RT_BINNED runs k_rt_trace2) in frames of 72 x 43 pixels (nine tile columns: the last pair
of a row has one tile; a height that is no multiple of eight) and 16 x 8 (one tile pair):
  * a seeded soup of 300 triangles with random winding: about half of its hits face away from a light;
  * a wall whose stored normals point away from the light: every D is zero, no ray is walked; the same wall with every winding
    flipped: every hit is lit, every lane of a covered pair walks two rays;
  * the flipped wall with occluders between it and the light: certain occluders and drains, found by lanes that do not own the pixel.
Every frame is compared bit for bit, all planes and XRGB, with RT_BRUTE under the same setting, and its shadow-ray count (hits x
light positions, walked or not) with brute force's.  Nothing is skipped: a frame that was not rendered by the mode asked for fails.
"""
import numpy as np
import pytest

import mirt
from devbuf import DeviceArray
from mirt_oracle import DEFAULT_LIGHT

pytestmark = pytest.mark.gpu

W, H = 72, 43
SMALL = (16, 8)                                  # one tile pair
BAND = (5, 38)
CAM = (0.0, 0.0, -3.0)
FOCAL = 56.0
PLANES = ("rgb", "index", "dist", "pos")
FILL = 0x11
TILE = 8


def with_normals(v, colours):
    """n x 15 rows from n x 3 x 3 vertices: the stored normal follows the winding, cross(v2 - v0, v1 - v0)."""
    n = len(v)
    t = np.zeros((n, 15), np.float32)
    t[:, 0:9] = v.reshape(n, 9)
    nrm = np.cross(v[:, 2] - v[:, 0], v[:, 1] - v[:, 0])
    t[:, 9:12] = nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    t[:, 12:15] = colours
    return t


def flipped(t):
    """Every winding turned round: v1 and v2 change places, the stored normal changes sign."""
    v = t[:, 0:9].reshape(-1, 3, 3)[:, [0, 2, 1]].copy()
    return with_normals(v, t[:, 12:15])


def soup(n=300, seed=20263):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (n, 1, 3))
    v = (c + rng.uniform(-0.22, 0.22, (n, 3, 3))).astype(np.float32)
    return with_normals(v, rng.uniform(0.15, 0.75, (n, 3)))


def wall(towards_light, z=0.0, nx=12, ny=8, seed=5):
    """nx x ny cells of two triangles in the plane `z`, short of the frame's border so that it leaves misses.  The lights of these
    scenes stand in front of it (smaller z): stored normals (0, 0, -1) face them, (0, 0, 1) face away."""
    rng = np.random.default_rng(seed)
    xs, ys = np.linspace(-1.5, 1.5, nx + 1), np.linspace(-0.9, 0.9, ny + 1)
    v = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = (xs[i], ys[j], z), (xs[i + 1], ys[j], z), (xs[i + 1], ys[j + 1], z), (xs[i], ys[j + 1], z)
            v += [(a, b, c), (a, c, d)]                          # cross(v2 - v0, v1 - v0) = (0, 0, -1): towards the light
    t = with_normals(np.array(v, np.float32), rng.uniform(0.2, 0.8, (len(v), 3)))
    return t if towards_light else flipped(t)


def occluders(n=40, seed=9):
    """Small triangles parallel to the wall between it and the lights, facing the lights: they are lit themselves and shadow the wall."""
    rng = np.random.default_rng(seed)
    c = np.concatenate([rng.uniform(-1.2, 1.2, (n, 1, 1)), rng.uniform(-0.7, 0.7, (n, 1, 1)), rng.uniform(-1.2, -0.4, (n, 1, 1))], axis=2)
    off = np.array([[-0.2, -0.15, 0.0], [0.2, -0.15, 0.0], [0.0, 0.2, 0.0]]) * rng.uniform(0.6, 1.4, (n, 1, 1))
    t = with_normals((c + off).astype(np.float32), rng.uniform(0.2, 0.8, (n, 3)))
    return np.where(t[:, 11:12] > 0, flipped(t), t)              # (whatever the draw: normal (0, 0, -1))


def light(x, y, z, power, colour=(1.0, 0.9, 0.8)):
    return [x, y, z, colour[0], colour[1], colour[2], power]


FRONT = np.array([light(0.3, -0.2, -2.0, 14.0)], np.float32)     # in front of the wall and of every occluder
ONE = np.array(DEFAULT_LIGHT, np.float32)
THREE = np.array([DEFAULT_LIGHT[0], light(0.9, 0.4, -1.6, 9.0), light(-1.1, -0.8, 0.3, 11.0)], np.float32)
SCENES = {"soup": soup(), "away": wall(False), "towards": wall(True), "occluded": np.concatenate([wall(True), occluders()])}
for _t in SCENES.values():
    _t.setflags(write=False)
    assert len(_t) > 64

_uploaded = [None]


def upload(name):
    if _uploaded[0] != name:
        mirt.scene_upload(SCENES[name])
        _uploaded[0] = name


def jitter(lights, samples):
    rng = np.random.default_rng(77)
    return (np.repeat(lights[:, 0:3], samples, axis=0) + rng.uniform(-0.08, 0.08, (len(lights) * samples, 3))).astype(np.float32)


def reset():
    mirt.set_soft_shadows(1)
    mirt.set_antialiasing(1)
    mirt.set_profiling(False)
    mirt.set_frames_in_flight(1)


def render(mode, lights, size=(W, H), band=None):
    """One frame or band with the four caller planes; returns the planes read back and the call's counters."""
    w, h = size
    y0, y1 = band if band else (0, h)
    shapes = {"xrgb": ((h, w), np.uint32), "rgb": ((h, w, 3), np.float32), "index": ((h, w), np.int32), "dist": ((h, w), np.float32),
              "pos": ((h, w, 3), np.float32)}
    bufs = {k: DeviceArray(s[0], s[1], FILL) for k, s in shapes.items()}
    try:
        view = mirt.make_view(CAM, mirt.rot_from_yaw(0.0, 1.0), FOCAL * w / W, w, h)
        mirt.raytrace_device(view, lights, (0.2, 0.2, 0.2), mode, y0, y1, 0, bufs["xrgb"].ptr, w * 4,
                             **{"d_" + k: bufs[k].ptr for k in PLANES})
        st = mirt.stats()
        assert st["mode_used"] == mode, "rendered by mode %d, not by %d" % (st["mode_used"], mode)
        out = {k: b.read() for k, b in bufs.items()}
        out["stats"] = st
        return out
    finally:
        for b in bufs.values():
            b.free()


def same(got, want, what):
    for k in ("xrgb",) + PLANES:
        a, b = got[k].view(np.uint32), want[k].view(np.uint32)
        assert np.array_equal(a, b), "%s: %s differs in %d words" % (what, k, int((a != b).sum()))
    assert got["stats"]["shadow_rays"] == want["stats"]["shadow_rays"], "%s: shadow rays %d, brute force %d" % (
        what, got["stats"]["shadow_rays"], want["stats"]["shadow_rays"])


_brute = {}


def setting(lights, samples, aa):
    mirt.set_antialiasing(aa)
    mirt.set_soft_shadows(samples, jitter(lights, samples) if samples > 1 else None)


def brute(scene, lights, samples=1, aa=1, size=(W, H), band=None):
    """The brute-force frame of a case: rendered once, shared, never changed."""
    key = (scene, lights.tobytes(), samples, aa, size, band)
    if key not in _brute:
        reset()
        upload(scene)
        setting(lights, samples, aa)
        ref = render(mirt.RT_BRUTE, lights, size, band)
        reset()
        for k in ("xrgb",) + PLANES:
            ref[k].setflags(write=False)
        _brute[key] = ref
    return _brute[key]


def check(scene, lights, samples=1, aa=1, size=(W, H), band=None, flight=1, profiled=False):
    """`flight` binned frames (each stream runs a pass of its own) against brute force; returns the last frame."""
    want = brute(scene, lights, samples, aa, size, band)
    try:
        upload(scene)
        setting(lights, samples, aa)
        mirt.set_frames_in_flight(flight)
        mirt.set_profiling(profiled)
        what = "%s, %d light(s) x %d, aa %d, %s, band %s, %d in flight, profiling %s" % (scene, len(lights), samples, aa, size, band, flight, profiled)
        got = None
        for _ in range(flight):
            got = render(mirt.RT_BINNED, lights, size, band)
            same(got, want, what)
        if aa == 1 and band is None:                              # hits x light positions, whether a ray was walked or not
            assert got["stats"]["shadow_rays"] == int((want["index"] >= 0).sum()) * len(lights) * samples
        return got
    finally:
        reset()


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    _uploaded[0] = None
    yield
    reset()
    mirt.shutdown()


def needed_per_pair(scene, ref, positions):
    """For every tile pair of a whole frame and every light position: (hits, needed rays, hits left out as too close to call), from
    the brute-force index and pos planes in float64.  A ray is needed when dot(rDir, nDir) > 0 (then D = B * dot is not zero for the
    positive colours of these lights)."""
    idx, pos = ref["index"], ref["pos"].astype(np.float64)
    nrm = SCENES[scene][:, 9:12].astype(np.float64)
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    hit = idx >= 0
    out = []
    for L in positions.astype(np.float64):
        d = L - pos
        d /= np.maximum(np.linalg.norm(d, axis=2, keepdims=True), 1e-300)
        dot = (d * nrm[np.maximum(idx, 0)]).sum(axis=2)
        need, unsure = hit & (dot > 0), hit & (np.abs(dot) < 1e-4)
        h, w = idx.shape
        for y in range(0, h, TILE):
            for x in range(0, w, 2 * TILE):
                box = (slice(y, y + TILE), slice(x, x + 2 * TILE))
                out.append((int(hit[box].sum()), int((need & ~unsure)[box].sum()), int(unsure[box].sum())))
    return out


def test_the_scenes_are_what_the_cases_need():
    """On the CPU, from brute-force frames: the tile pairs of the frames include one with more than 64 needed rays (some lane walks
    two), one with 1 .. 64 (nobody walks a second), one with hits and no needed ray (the wave goes straight to the sum); the hits
    whose sign of dot(rDir, nDir) float64 cannot call are under 1 %; the wall shows what its two cases are about."""
    pairs = []
    for scene, lights in (("soup", ONE), ("soup", THREE), ("away", FRONT), ("towards", FRONT), ("occluded", FRONT)):
        pairs += needed_per_pair(scene, brute(scene, lights), lights[:, 0:3])
    pairs += needed_per_pair("soup", brute("soup", ONE, size=SMALL), ONE[:, 0:3])
    hits, unsure = sum(p[0] for p in pairs), sum(p[2] for p in pairs)
    assert hits > 5000 and unsure * 100 < hits, (hits, unsure)
    assert any(n > 64 for _, n, u in pairs), "no pair with more than 64 needed rays"
    assert any(1 <= n and n + u <= 64 for _, n, u in pairs), "no pair with 1 .. 64 needed rays"
    assert any(h > 0 and n + u == 0 for h, n, u in pairs), "no pair with hits and no needed ray"
    soup_pairs = needed_per_pair("soup", brute("soup", ONE), ONE[:, 0:3])
    assert any(n > 64 for _, n, u in soup_pairs) and any(1 <= n and n + u <= 64 for _, n, u in soup_pairs), "the soup alone shows both walks"
    share = sum(p[1] for p in soup_pairs) / float(sum(p[0] for p in soup_pairs))
    assert 0.25 < share < 0.75, "random winding: about half of the soup's hits face the light (%.2f)" % share
    away, towards, occ = (needed_per_pair(s, brute(s, FRONT), FRONT[:, 0:3]) for s in ("away", "towards", "occluded"))
    assert sum(p[0] for p in away) > 1000 and sum(p[1] + p[2] for p in away) == 0, "the wall turned away needs no ray at all"
    assert all(p[1] == p[0] for p in towards) and any(p[1] == 128 for p in towards), "the wall turned to the light: every hit, whole pairs"
    assert all(p[1] == p[0] for p in occ) and any(p[1] == 128 for p in occ)
    # occluders shadow part of the wall and are lit themselves
    lit_wall, shadowed = brute("towards", FRONT), brute("occluded", FRONT)
    wall_px = shadowed["index"] < len(SCENES["towards"])
    wall_px &= shadowed["index"] >= 0
    darker = (shadowed["rgb"] != lit_wall["rgb"]).any(axis=2) & wall_px & (lit_wall["index"] == shadowed["index"])
    assert darker.sum() > 100 and (wall_px & ~darker).sum() > 100, "no wall pixel in shadow or none in light"
    assert (shadowed["index"] >= len(SCENES["towards"])).sum() > 50, "no occluder in view"


CASES = {"one-light": (ONE, 1, 1), "three-lights": (THREE, 1, 1), "two-samples": (ONE, 2, 1), "supersampled": (ONE, 1, 2)}


@pytest.mark.parametrize("flight", [1, 4])
@pytest.mark.parametrize("profiled", [False, True], ids=["plain", "profiled"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_soup_with_random_winding(case, profiled, flight):
    lights, samples, aa = CASES[case]
    check("soup", lights, samples, aa, flight=flight, profiled=profiled)


@pytest.mark.parametrize("flight", [1, 4])
@pytest.mark.parametrize("case", ["one-light", "three-lights", "supersampled"])
def test_soup_band_of_rows_and_one_pair(case, flight):
    lights, samples, aa = CASES[case]
    check("soup", lights, samples, aa, band=BAND, flight=flight)
    check("soup", lights, samples, aa, size=SMALL, flight=flight, profiled=flight == 4)


@pytest.mark.parametrize("profiled", [False, True], ids=["plain", "profiled"])
def test_soup_under_a_light_that_moves_every_frame(profiled):
    """A light that has moved within the last frames is binned by the frame's own pass, not read from the shared cube; the first
    frames' lists are sized before any count is known."""
    for i in range(6):
        lights = np.array([light(-0.5 + 0.03 * i, -0.5, -0.7 + 0.02 * i, 14.0)], np.float32)
        check("soup", lights, flight=1, profiled=profiled)
    lights = np.array([light(-0.5, -0.5, -0.7, 14.0), light(0.9 + 0.01, 0.4, -1.6, 9.0)], np.float32)
    for i in range(3):
        lights = lights.copy()
        lights[1, 0] += 0.05
        check("soup", lights, flight=4, profiled=profiled)


def test_faces_turned_away_walk_no_ray():
    """Every D is zero: the frame equals brute force, and with profiling on it offers and tests fewer candidates than the same wall
    with every winding flipped, whose hits all need their rays -- while the shadow-ray count, hits x light positions, is the same."""
    away = check("away", FRONT, profiled=True)
    towards = check("towards", FRONT, profiled=True)
    a, t = away["stats"], towards["stats"]
    print("away: tests %d candidates %d shadow steps %d; towards: tests %d candidates %d shadow steps %d"
          % (a["tests"], a["candidates"], a["steps_shadow"], t["tests"], t["candidates"], t["steps_shadow"]))
    assert np.array_equal(away["index"], towards["index"]) and a["shadow_rays"] == t["shadow_rays"] > 1000
    assert a["tests"] < t["tests"] and a["candidates"] < t["candidates"]
    assert a["steps_shadow"] == 0, "no ray is needed, none is walked"
    check("away", FRONT, flight=4)
    check("away", THREE[:2], samples=2, aa=2)


@pytest.mark.parametrize("flight", [1, 4])
def test_faces_turned_to_the_light_behind_occluders(flight):
    """Every lane of a covered pair walks two rays; certain occluders and queued pairs, found on behalf of other lanes' pixels."""
    got = check("occluded", FRONT, flight=flight, profiled=True)
    assert got["stats"]["steps_shadow"] > 0 and got["stats"]["drains"] > 0
    check("occluded", FRONT, flight=flight)
    check("occluded", np.array([FRONT[0], light(-0.6, 0.5, -2.4, 9.0)], np.float32), samples=2, flight=flight)
    check("occluded", FRONT, aa=2, band=BAND, flight=flight)
    check("towards", FRONT, flight=flight)


@pytest.mark.parametrize("scene", ["soup", "occluded"])
def test_signs_of_zero_and_nan(scene):
    """A light of colour zero (every D is +0 or -0 ... or NaN at r = 0), one of negative colour (D = -0 where the face is turned
    away, negative where it is lit), and a light placed exactly on a vertex in view."""
    pos = (0.3, -0.2, -2.0) if scene == "occluded" else DEFAULT_LIGHT[0][0:3]
    dark = np.array([light(pos[0], pos[1], pos[2], 14.0, (0.0, 0.0, 0.0))], np.float32)
    check(scene, dark)
    check(scene, dark, profiled=True)
    negative = np.array([light(pos[0], pos[1], pos[2], 14.0, (-1.0, -0.9, -0.8))], np.float32)
    check(scene, negative)
    check(scene, np.concatenate([negative, dark, FRONT]), flight=4)
    ref = brute(scene, FRONT if scene == "occluded" else ONE)
    seen = ref["index"][H // 2, W // 2]
    assert seen >= 0, "the frame's centre shows no triangle"
    for corner in range(3):
        at = SCENES[scene][seen, 3 * corner:3 * corner + 3]
        on_vertex = np.array([light(at[0], at[1], at[2], 14.0)], np.float32)
        check(scene, on_vertex)
        check(scene, np.concatenate([on_vertex, negative]), aa=2, profiled=True)
