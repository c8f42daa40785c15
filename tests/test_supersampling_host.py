"""The guards of tests/test_gpu_supersampling.py with the oracle alone, and the comparison it uses against planted corruptions: a
case that exercises nothing, or a comparison that lets a wrong plane through, shows here, without a GPU."""
import numpy as np
import pytest

import supersampling as ss
from ref_cases import aa_overshoot, overshooting


@pytest.mark.parametrize("samples", [2, 3, 5])
def test_no_coordinate_overshoots(samples):
    c = np.arange(4200)
    assert (aa_overshoot(c, samples) <= 0).all()
    assert overshooting(ss.SLIVER_W, samples) == [] and overshooting(ss.SLIVER_H, samples) == []


@pytest.mark.parametrize("samples", ss.SLIVER_SAMPLES + (ss.CONTROL_SAMPLES,))
def test_sliver_guards(oracle, samples):
    """Every sliver of the 96 x 72 frame begins beyond the half pixel around its column or row; the plain frame never sees it, the
    supersampled oracle frame gives it 20 pixels and more -- and none at the control's 5 samples.  The far soup that pads the scene
    to the other kernels' triangle counts changes no pixel."""
    case = ss.sliver_case(oracle, samples)
    frame, plain = ss.sliver_frames(oracle, samples)
    ss.assert_sliver_guards(case, frame, plain, samples)
    for n in (65, 300, 400):
        padded = ss.sliver_case(oracle, samples, n)
        assert len(padded["tris"]) == n and np.array_equal(padded["tris"][:len(case["tris"])], case["tris"])
        f, p = ss.sliver_frames(oracle, samples, n)
        ss.assert_sliver_guards(padded, f, p, samples)
        assert np.array_equal(f["index"], frame["index"]) and np.array_equal(f["rgb"].view(np.uint32), frame["rgb"].view(np.uint32))


@pytest.mark.parametrize("samples", ss.SLIVER_SAMPLES)
def test_sliver_bands(oracle, samples):
    case = ss.sliver_case(oracle, samples)
    bands = ss.sliver_bands(case)
    assert bands[0][0] == 0 and bands[-1][1] == ss.SLIVER_H and all(a[1] == b[0] and a[0] < a[1] for a, b in zip(bands, bands[1:]))
    last = bands[0][1] - 1
    assert last in case["rows"] and aa_overshoot(last, samples, ss.SLIVER_H / 2.0) > 0          # a band ends on an overshooting row
    assert any(y0 % 8 for y0, _ in bands)
    frame, _ = ss.sliver_frames(oracle, samples)
    assert int((frame["index"][last] == 2 + len(case["cols"]) + case["rows"].index(last)).sum()) >= 20


@pytest.mark.parametrize("path", sorted(set(ss.SOUP_PATHS) - {"brute1200_auto"}))       # (brute1200_auto is binned1200's scene)
def test_sparse_soups_leave_sub_rays_without_a_hit(oracle, path):
    """Between 20 % and 80 % of the pixels hold a sub-ray that missed -- x1 stood still, the record was carried or stayed empty --
    at every sample count; pixels with no hit at all, with some and with every sub-ray hitting all occur."""
    mode, tris, lights, rot = ss.soup_case(oracle, path)
    assert len(tris) == ss.SOUP_PATHS[path][1] and len(lights) == ss.SOUP_PATHS[path][2]
    for aa in range(2, 9):
        assert ss.SOUP_W * ss.SOUP_H * aa * aa * len(tris) <= 5e8
        hits = ss.sub_ray_hits(oracle, tris, ss.SOUP_CAM, rot, ss.SOUP_FOCAL, ss.SOUP_W, ss.SOUP_H, aa)
        share = float((hits < aa * aa).mean())
        assert 0.2 <= share <= 0.8, (path, aa, share)
        assert (hits == 0).mean() > 0.05 and ((hits > 0) & (hits < aa * aa)).mean() > 0.05 and (hits == aa * aa).mean() > 0.05
        if aa in (2, 8):
            assert np.array_equal(ss.soup_frame(oracle, path, aa)["index"] < 0, hits == 0)


def test_selection_boundaries_are_those_of_the_frame_code():
    """capi/rt_frame.cpp: n <= 64 takes the tile kernel, 16 + 48 * n * (2 + lights) <= 48 KiB the LDS-resident one."""
    fits = lambda n, nl: 16 + 48 * n * (2 + nl) <= 48 * 1024
    p = ss.SOUP_PATHS
    assert p["tile64"][1] == 64 and p["small65"][1] == 65
    assert fits(p["small255"][1], p["small255"][2]) and not fits(p["brute256"][1], p["brute256"][2]) and p["brute256"][1] == p["small255"][1] + 1
    assert fits(p["brute342"][1] - 1, p["brute342"][2]) and not fits(p["brute342"][1], p["brute342"][2])
    assert p["brute1200_auto"][1:] == p["binned1200"][1:]
    # RT_AUTO bins from 4e7 pixel-triangles on (mode_bins): brute1200_auto stays below, AUTO_BINS lies above, within the oracle's budget
    assert ss.SOUP_W * ss.SOUP_H * p["brute1200_auto"][1] < 40000000 <= ss.SOUP_W * ss.SOUP_H * ss.AUTO_BINS[1] and ss.SOUP_W * ss.SOUP_H > 4096
    assert ss.SOUP_W * ss.SOUP_H * ss.AUTO_BINS[1] * max(ss.AUTO_BINS_SAMPLES) ** 2 <= 5e8


@pytest.mark.parametrize("aa", ss.AUTO_BINS_SAMPLES)
def test_auto_bins_soup_is_sparse(oracle, aa):
    assert 0.2 <= ss.soup_share(oracle, "auto_bins", aa) <= 0.8


def _as_rendered(ref):
    got = {k: np.array(v) for k, v in ref.items() if isinstance(v, np.ndarray)}
    got["stats"] = {"primary_rays": 0, "shadow_rays": ref["nshadow"]}
    return got


def test_comparison_catches_planted_corruptions(oracle):
    """compare_frames passes the oracle's own frame and fails when one sliver pixel's index is the backdrop's, one colour is off by
    an ulp, one missed pixel's distance is 0, one XRGB word or one count is off."""
    W, H, aa = ss.SLIVER_W, ss.SLIVER_H, 8
    case = ss.sliver_case(oracle, aa)
    ref, _ = ss.sliver_frames(oracle, aa)
    good = _as_rendered(ref)
    good["stats"]["primary_rays"] = W * H * aa * aa
    ss.compare_frames(good, ref, W, H, aa)
    ys, xs = np.nonzero(ref["index"] == 2)                          # the first column sliver
    assert len(ys) >= 20

    def corrupted(change):
        got = _as_rendered(ref)
        got["stats"]["primary_rays"] = W * H * aa * aa
        change(got)
        with pytest.raises(AssertionError):
            ss.compare_frames(got, ref, W, H, aa)

    def backdrop_index(g):
        g["index"][ys[3], xs[3]] = 0
    def colour_ulp(g):
        g["rgb"].view(np.uint32)[H // 2, W // 2, 1] += 1
    def xrgb_word(g):
        g["xrgb"][H // 2, W // 2] ^= 1
    def rays(g):
        g["stats"]["primary_rays"] -= 1
    def shadows(g):
        g["stats"]["shadow_rays"] += 1
    for change in (backdrop_index, colour_ulp, xrgb_word, rays, shadows):
        corrupted(change)
    assert abs(float(good["rgb"][H // 2, W // 2, 1]) - float(np.nextafter(good["rgb"][H // 2, W // 2, 1], np.float32(9)))) < ss.TOL
    # a missed pixel: the sparse soup has them, the sliver frame has none
    sref = ss.soup_frame(oracle, "small65", 4)
    my, mx = np.nonzero(sref["index"] < 0)
    assert len(my) and sref["dist"][my[0], mx[0]] == ss.FLT_MAX
    got = _as_rendered(sref)
    got["stats"]["primary_rays"] = ss.SOUP_W * ss.SOUP_H * 16
    ss.compare_frames(got, sref, ss.SOUP_W, ss.SOUP_H, 4)
    got["dist"][my[0], mx[0]] = 0.0
    with pytest.raises(AssertionError):
        ss.compare_frames(got, sref, ss.SOUP_W, ss.SOUP_H, 4)
