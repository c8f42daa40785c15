"""Supersampling at 2 to 8 samples on every ray-trace kernel path, against the oracle: k_rt_tile2<16, true>, k_rt_small<2>,
k_rt_brute<2> and k_rt_trace2<true, ...> each have an instantiation of their own for it, and at 4, 6, 7 and 8 samples the reference's
chain of sub-ray coordinates ends a few ulp beyond the half pixel that the binning's pads and the tile kernel's rectangles allow for
(tests/supersampling.py; tests/test_aa_reach.py holds the set-up arithmetic, tests/test_supersampling_host.py the guards of these
cases with the oracle alone).  Every comparison is _rt_compare's of tests/test_gpu_parity.py: index, distance and position planes,
float colour bits, XRGB words and both ray counts."""
import ctypes

import numpy as np
import pytest

import mirt
import supersampling as ss
from devbuf import DeviceArray

pytestmark = pytest.mark.gpu

MODES = {"auto": mirt.RT_AUTO, "brute": mirt.RT_BRUTE, "binned": mirt.RT_BINNED}
INDIRECT = (0.2, 0.2, 0.2)
DEFAULT_LIGHT = np.array([[0.0, -0.5, -0.7, 1.0, 1.0, 1.0, 14.0]], np.float32)


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)          # raises MirtError (fails loudly) when libmirt.so or the GPU is missing
    yield
    mirt.set_antialiasing(1)
    mirt.set_soft_shadows(1)
    mirt.set_frames_in_flight(1)
    mirt.shutdown()


def _render(tris, cam, rot, focal, W, H, lights, mode, aa, samples=1, jitter=None):
    mirt.scene_upload(tris)
    mirt.set_soft_shadows(samples, jitter)
    mirt.set_antialiasing(aa)
    try:
        return mirt.raytrace(mirt.make_view(cam, rot, focal, W, H), lights, mode=mode, want_intersection=True)
    finally:
        mirt.set_soft_shadows(1)
        mirt.set_antialiasing(1)


def _compare(oracle, tris, cam, rot, focal, W, H, lights, mode, aa, samples=1, jitter=None, ref=None):
    if ref is None:
        ref = oracle.raytrace(tris, cam, rot, focal, W, H, lights, threads=16, samples=samples, jitter=jitter, aa=aa)
    got = _render(tris, cam, rot, focal, W, H, lights, mode, aa, samples, jitter)
    ss.compare_frames(got, ref, W, H, aa)
    return got, ref


def _jitter(oracle, lights, samples, seed=1):
    ctypes.CDLL(None).srand(seed)
    return np.concatenate([oracle.jitter(l[0:3], samples) for l in np.asarray(lights, np.float32).reshape(-1, 7)])


# ---- a. sub-rays past the half pixel ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["tile", "small65", "brute300", "brute400", "binned65", "binned300", "binned400"])
@pytest.mark.parametrize("samples", ss.SLIVER_SAMPLES + (ss.CONTROL_SAMPLES,))
def test_slivers_beyond_the_half_pixel(oracle, samples, path):
    """A right triangle behind every last column and row of an 8-pixel bin whose chain of sub-ray coordinates overshoots, its edge
    half the overshoot beyond the half pixel: only the last sub-ray sees it, and only a tile or bin that keeps the pair lets it.  The
    bare scene takes the tile kernel (rectangles widened by exactly 0.5); padded with a far soup it takes the LDS-resident kernel
    (65 triangles), the chunked brute-force kernel (300, 400) and the binned trace kernel (bins padded by exactly half a pixel)."""
    n = None if path == "tile" else int(path.lstrip("abcdefghijklmnopqrstuvwxyz"))
    mode = mirt.RT_AUTO if path == "tile" else mirt.RT_BINNED if path.startswith("binned") else mirt.RT_BRUTE
    case = ss.sliver_case(oracle, samples, n)
    ref, plain = ss.sliver_frames(oracle, samples, n)
    ss.assert_sliver_guards(case, ref, plain, samples)
    got, _ = _compare(oracle, case["tris"], ss.SLIVER_CAM, case["rot"], ss.SLIVER_FOCAL, ss.SLIVER_W, ss.SLIVER_H, ss.SLIVER_LIGHT, mode, samples, ref=ref)
    assert got["stats"]["mode_used"] == (mirt.RT_BINNED if mode == mirt.RT_BINNED else mirt.RT_BRUTE)
    if path == "tile":
        assert len(case["tris"]) <= 64


@pytest.mark.parametrize("path", ["tile", "brute300", "binned300"])
@pytest.mark.parametrize("samples", ss.SLIVER_SAMPLES)
def test_slivers_in_bands(oracle, samples, path):
    """The same frame as three bands into device planes: the first band's last row overshoots and carries a row sliver (the rows
    below it belong to another call), the third starts at a row that is no multiple of 8."""
    n = None if path == "tile" else 300
    mode = mirt.RT_AUTO if path == "tile" else mirt.RT_BINNED if path.startswith("binned") else mirt.RT_BRUTE
    case = ss.sliver_case(oracle, samples, n)
    ref, plain = ss.sliver_frames(oracle, samples, n)
    ss.assert_sliver_guards(case, ref, plain, samples)
    bands = ss.sliver_bands(case)
    assert bands[0][1] - 1 in case["rows"] and any(y0 % 8 for y0, _ in bands)
    W, H = ss.SLIVER_W, ss.SLIVER_H
    view = mirt.make_view(ss.SLIVER_CAM, case["rot"], ss.SLIVER_FOCAL, W, H)
    planes = {"xrgb": DeviceArray((H, W), np.uint32), "rgb": DeviceArray((H, W, 3), np.float32), "index": DeviceArray((H, W), np.int32, 0xFF),
              "dist": DeviceArray((H, W), np.float32), "pos": DeviceArray((H, W, 3), np.float32)}
    mirt.scene_upload(case["tris"])
    mirt.set_antialiasing(samples)
    try:
        counts = {"primary_rays": 0, "shadow_rays": 0}
        for y0, y1 in bands:
            mirt.raytrace_device(view, ss.SLIVER_LIGHT, INDIRECT, mode, y0, y1, 0, planes["xrgb"].ptr, W * 4, planes["rgb"].ptr,
                                 planes["index"].ptr, planes["dist"].ptr, planes["pos"].ptr)
            st = mirt.stats()                                       # (waits for the band) the device's counters of this call alone
            band = oracle.raytrace(case["tris"], ss.SLIVER_CAM, case["rot"], ss.SLIVER_FOCAL, W, H, ss.SLIVER_LIGHT, y0=y0, y1=y1,
                                   threads=16, aa=samples, want=())
            assert st["primary_rays"] == W * (y1 - y0) * samples * samples
            assert st["shadow_rays"] == band["nshadow"], "band %d..%d: %d shadow rays, the oracle traces %d" % (y0, y1, st["shadow_rays"], band["nshadow"])
            assert st["mode_used"] == (mirt.RT_BINNED if mode == mirt.RT_BINNED else mirt.RT_BRUTE)
            for k in counts:
                counts[k] += st[k]
        got = {k: p.read() for k, p in planes.items()}
        got["stats"] = counts                                       # the bands' sums: compare_frames holds them against the whole frame's
    finally:
        mirt.set_antialiasing(1)
        for p in planes.values():
            p.free()
    ss.compare_frames(got, ref, W, H, samples)


# ---- b. every sample count on every kernel ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", sorted(ss.SOUP_PATHS))
@pytest.mark.parametrize("aa", range(2, 9))
def test_every_sample_count_on_every_kernel(oracle, aa, path):
    """Sparse soups at the triangle counts where capi/rt_frame.cpp changes kernel.  In 20 % to 80 % of the pixels a sub-ray misses:
    x1 stands still after it and the closest-hit record is carried to the next sub-ray, or the pixel ends without a hit
    (supersampling.sparse_share, asserted here as in test_supersampling_host.py).  brute1200_auto: RT_AUTO, which keeps a frame this
    small on the brute-force kernel."""
    mode, tris, lights, rot = ss.soup_case(oracle, path)
    ref = ss.soup_frame(oracle, path, aa)
    assert 0.2 <= ss.soup_share(oracle, path, aa) <= 0.8
    got, _ = _compare(oracle, tris, ss.SOUP_CAM, rot, ss.SOUP_FOCAL, ss.SOUP_W, ss.SOUP_H, lights, MODES[mode], aa, ref=ref)
    assert got["stats"]["mode_used"] == (mirt.RT_BINNED if mode == "binned" else mirt.RT_BRUTE)


@pytest.mark.parametrize("aa", ss.AUTO_BINS_SAMPLES)
def test_auto_selects_the_bins_supersampled(oracle, aa):
    """RT_AUTO bins from 4e7 pixel-triangles on whatever the sample count.  A soup of 6600 triangles crosses that on the 96 x 64
    frame; the oracle's budget (4e7 * samples^2 tests) admits 2 and 3 samples."""
    mode, tris, lights, rot = ss.soup_case(oracle, "auto_bins")
    assert 0.2 <= ss.soup_share(oracle, "auto_bins", aa) <= 0.8
    got, _ = _compare(oracle, tris, ss.SOUP_CAM, rot, ss.SOUP_FOCAL, ss.SOUP_W, ss.SOUP_H, lights, mirt.RT_AUTO, aa, ref=ss.soup_frame(oracle, "auto_bins", aa))
    assert got["stats"]["mode_used"] == mirt.RT_BINNED


# ---- c. binned against brute on random configurations, supersampled ----------------------------------------------------------------

@pytest.mark.parametrize("seed", range(24))
def test_binned_equals_brute_on_random_supersampled_configurations(oracle, seed):
    """test_rt_binned_equals_brute_on_random_configurations with a sample count drawn from 2 to 8: cameras inside the soup, yaws past
    90 degrees, one to three lights, Cornell walls every fourth seed, soft shadows of 2 samples every sixth.  The binned frame equals
    the brute-force frame word for word, plane for plane (brute force itself is held against the oracle above)."""
    rng = np.random.RandomState(7000 + seed)
    aa = 2 + seed % 7 if seed < 14 else int(rng.randint(2, 9))       # every count twice, then drawn
    n = int(rng.choice([300, 1000, 2500, 4000]))
    size = float(rng.choice([0.1, 0.25, 0.5] if n <= 1000 else [0.05, 0.1, 0.25]))
    tris = oracle.soup(300 + seed, n, size)
    if seed % 4 == 0:
        tris = np.concatenate([tris, oracle.cornell()])
    W, H = int(rng.randint(40, 161)), int(rng.randint(30, 121))
    inside = seed % 3 == 0
    cam = rng.uniform(-0.8, 0.8, 3) if inside else np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), -rng.uniform(1.5, 3.0)])
    # (a camera outside the soup keeps it in view; one inside it looks backwards on every second of its seeds)
    yaw = float(rng.uniform(1.6, 3.1) * rng.choice([-1.0, 1.0])) if inside and seed % 2 else float(rng.uniform(-0.4, 0.4))
    rot = oracle.rot_from_yaw(yaw, 1.0)
    focal = float(rng.uniform(0.3, 1.2) * H)
    nl = 1 + seed % 3
    lights = np.zeros((nl, 7), np.float32)
    lights[:, 0:3] = rng.uniform(-0.9, 0.9, (nl, 3))
    lights[:, 3:6] = rng.uniform(0.2, 1.0, (nl, 3))
    lights[:, 6] = rng.uniform(3, 20, nl)
    samples = 2 if seed % 6 == 0 else 1
    jit = _jitter(oracle, lights, samples, seed=seed + 1) if samples > 1 else None
    a = _render(tris, cam, rot, focal, W, H, lights, mirt.RT_BINNED, aa, samples, jit)
    b = _render(tris, cam, rot, focal, W, H, lights, mirt.RT_BRUTE, aa, samples, jit)
    assert a["stats"]["mode_used"] == mirt.RT_BINNED and b["stats"]["mode_used"] == mirt.RT_BRUTE
    assert (b["index"] >= 0).mean() > 0.02
    assert np.array_equal(a["index"], b["index"]), "closest-hit index differs in %d pixels at %d samples" % (int((a["index"] != b["index"]).sum()), aa)
    for k in ("dist", "pos", "rgb"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert np.array_equal(a["xrgb"], b["xrgb"])
    assert a["stats"]["primary_rays"] == b["stats"]["primary_rays"] == W * H * aa * aa
    assert a["stats"]["shadow_rays"] == b["stats"]["shadow_rays"]


# ---- d. tiny and ragged supersampled frames ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("aa", [2, 4, 8])
@pytest.mark.parametrize("W,H", [(1, 1), (2, 3), (3, 3), (7, 5), (65, 9), (130, 3)])
def test_tiny_and_ragged_supersampled_frames(oracle, W, H, aa):
    """Frames smaller than a tile or a wave, widths that are a multiple of nothing: the Cornell box through the tile kernel, a
    90-triangle soup through the LDS-resident kernel and through the bins."""
    rot = oracle.rot_from_yaw(0.0, 1.0)
    focal = max(H, 2) / 2.0
    _compare(oracle, oracle.cornell(), (0, 0, -2), rot, focal, W, H, DEFAULT_LIGHT, mirt.RT_AUTO, aa)
    tris = oracle.soup(8, 90, 0.5)
    ref = oracle.raytrace(tris, (0, 0, -2), rot, focal, W, H, DEFAULT_LIGHT, threads=16, aa=aa)
    _compare(oracle, tris, (0, 0, -2), rot, focal, W, H, DEFAULT_LIGHT, mirt.RT_BRUTE, aa, ref=ref)
    got, _ = _compare(oracle, tris, (0, 0, -2), rot, focal, W, H, DEFAULT_LIGHT, mirt.RT_BINNED, aa, ref=ref)
    assert got["stats"]["mode_used"] == mirt.RT_BINNED


# ---- e. arithmetic outside the fast range -----------------------------------------------------------------------------------------

HUGE_AND_TINY_COLOUR = np.array([[0.0, -0.5, -0.7, 3.0e11, 1.0e-14, 1.0, 14.0]], np.float32)      # ODD_LIGHTS of tests/test_gpu_parity.py


def test_odd_light_supersampled(oracle):
    """A light colour beyond 2^40 and below 2^-40 at 4 samples: the tile kernel (Cornell box) and the binned trace kernel (soup)
    take the general divisions."""
    _compare(oracle, oracle.cornell(), (0, 0, -3), oracle.rot_from_yaw(0.0, 1.0), 96.0, 96, 96, HUGE_AND_TINY_COLOUR, mirt.RT_AUTO, 4)
    got, _ = _compare(oracle, oracle.soup(21, 1200, 0.15), (0.1, 0, -2.2), oracle.rot_from_yaw(0.2, 1.0), 64.0, 128, 80, HUGE_AND_TINY_COLOUR, mirt.RT_BINNED, 4)
    assert got["stats"]["mode_used"] == mirt.RT_BINNED


@pytest.mark.parametrize("scale", [1.0e-9, 3.0e5])
def test_scaled_scenes_supersampled(oracle, scale):
    """test_scaled_scenes_leave_the_fast_range at 4 samples: products, determinants and squared distances below 2^-40 or beyond the
    range at the top, through the tile kernel and the binned trace kernel."""
    tris = np.array(oracle.cornell())
    tris[:, 0:9] *= np.float32(scale)
    L = np.array([[0.0, -0.5 * scale, -0.7 * scale, 1.0, 1.0, 1.0, 14.0 * scale * scale]], np.float32)
    _compare(oracle, tris, (0.0, 0.0, -3.0 * scale), oracle.rot_from_yaw(0.1, 1.0), 96.0, 96, 96, L, mirt.RT_AUTO, 4)
    soup = oracle.soup(23, 1200, 0.15)
    soup[:, 0:9] *= np.float32(scale)
    got, _ = _compare(oracle, soup, (0.0, 0.0, -2.0 * scale), oracle.rot_from_yaw(0.0, 1.0), 64.0, 128, 80, L, mirt.RT_BINNED, 4)
    assert (got["index"] >= 0).any()


@pytest.mark.parametrize("n", [65, 400])
def test_huge_coordinates_supersampled(oracle, n):
    """test_rt_huge_coordinates_take_exact_path's scene at 3 samples and at the sizes of the LDS-resident (65) and the chunked
    brute-force kernel (400): operands beyond the pre-reject filter's range set their `unsafe` flag."""
    tris = oracle.soup(6, n, 0.3)
    tris[5, 0:9] *= 1.0e12
    got, _ = _compare(oracle, tris, (0, 0, -2), oracle.rot_from_yaw(0.0, 1.0), 64.0, 128, 128, DEFAULT_LIGHT, mirt.RT_BRUTE, 3)
    assert (got["index"] >= 0).any() and (got["index"] < 0).any()


# ---- f. a kept binning pass follows the sample count ------------------------------------------------------------------------------

@pytest.mark.parametrize("in_flight", [1, 2])
def test_kept_binning_pass_follows_the_sample_count(oracle, in_flight):
    """One view, one scene, binned frames at 1, 4, 1, 3, 8 and 8 samples: a pass kept from the plain frame has pads of 0 and -1, a
    supersampled frame needs half a pixel on either side (the pass key mixes the sample count).  Every frame equals the oracle's."""
    W, H = ss.SOUP_W, ss.SOUP_H
    mode, tris, lights, rot = ss.soup_case(oracle, "binned1200")
    view = mirt.make_view(ss.SOUP_CAM, rot, ss.SOUP_FOCAL, W, H)
    seq = [1, 4, 1, 3, 8, 8]
    want = {aa: (ss.soup_frame(oracle, "binned1200", aa) if aa > 1 else
                 oracle.raytrace(tris, ss.SOUP_CAM, rot, ss.SOUP_FOCAL, W, H, lights, threads=16)) for aa in set(seq)}
    mirt.scene_upload(tris)
    outs = []
    try:
        mirt.set_frames_in_flight(in_flight)
        for i, aa in enumerate(seq):
            planes = {"xrgb": DeviceArray((H, W), np.uint32), "rgb": DeviceArray((H, W, 3), np.float32), "index": DeviceArray((H, W), np.int32, 0xFF),
                      "dist": DeviceArray((H, W), np.float32), "pos": DeviceArray((H, W, 3), np.float32)}
            outs.append(planes)
            mirt.set_antialiasing(aa)
            mirt.raytrace_device(view, lights, INDIRECT, mirt.RT_BINNED, 0, H, 0, planes["xrgb"].ptr, W * 4, planes["rgb"].ptr,
                                 planes["index"].ptr, planes["dist"].ptr, planes["pos"].ptr)
            st = mirt.stats()                                       # (waits for the frame)
            assert st["mode_used"] == mirt.RT_BINNED
            if i and seq[i - 1] != aa and in_flight == 1:
                assert not st["bins_reused"], "frame %d at %d samples kept the pass of %d samples" % (i, aa, seq[i - 1])
            got = {k: p.read() for k, p in planes.items()}
            got["stats"] = st
            ss.compare_frames(got, want[aa], W, H, aa)
    finally:
        mirt.set_antialiasing(1)
        mirt.set_frames_in_flight(1)
        for planes in outs:
            for p in planes.values():
                p.free()


# ---- g. arguments -------------------------------------------------------------------------------------------------------------------

def test_sample_count_arguments(oracle):
    """More than 8 samples are refused and leave the count in force; 0, 1 and -3 switch supersampling off."""
    mode, tris, lights, rot = ss.soup_case(oracle, "small65")
    W, H = ss.SOUP_W, ss.SOUP_H
    view = mirt.make_view(ss.SOUP_CAM, rot, ss.SOUP_FOCAL, W, H)
    plain = oracle.raytrace(tris, ss.SOUP_CAM, rot, ss.SOUP_FOCAL, W, H, lights, threads=16)
    mirt.scene_upload(tris)
    try:
        mirt.set_antialiasing(6)
        with pytest.raises(mirt.MirtError):
            mirt.set_antialiasing(9)
        ss.compare_frames(mirt.raytrace(view, lights, mode=mirt.RT_BRUTE, want_intersection=True), ss.soup_frame(oracle, "small65", 6), W, H, 6)
        for off in (0, 1, -3):
            mirt.set_antialiasing(4)
            mirt.set_antialiasing(off)
            ss.compare_frames(mirt.raytrace(view, lights, mode=mirt.RT_BRUTE, want_intersection=True), plain, W, H, 1)
    finally:
        mirt.set_antialiasing(1)
