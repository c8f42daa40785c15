"""Shadow masks (mirt_shadow_mask*, mirt_direct_light_masked*): DirectLight's shadow decision per (record, light position), and
DirectLight from those bits.

The records are the closest hits of test_gpu_many_lights' two ray batches (257 and 513 rays, seeds 7 and 8) on `cornell` and
`soup2000`, with the odd records of its case() mixed in -- index -1, index n, a NaN coordinate, positions equal to light positions --,
the lights its lights_of() with rq.jitter(seed=3).  Light sets: 2 hard lights (one word, one pass), 3 x 11 = 33 positions (two planes;
the second pass holds one position) and 16 x 16 = 256 (eight planes).  Every comparison is bit for bit, and every oracle answer is
computed once and shared (with test_gpu_many_lights, where both run)."""
import numpy as np
import pytest

import mirt
import query_helpers as rq
from devbuf import DeviceArray, to_device
from test_gpu_many_lights import case as many_case, lights_of, scene_hits

pytestmark = pytest.mark.gpu

SETS = {"2x1": (2, 1), "3x11": (3, 11), "16x16": (16, 16)}
SCENES = ("cornell", "soup2000")
MODES = (("brute", mirt.QUERY_BRUTE), ("binned", mirt.QUERY_BINNED), ("auto", mirt.QUERY_AUTO))
FILL, FILLW = 0x5A, 0x5A5A5A5A
_cases, _decisions = {}, {}


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_query_mode(mirt.QUERY_AUTO)
    mirt.set_profiling(False)
    mirt.set_soft_shadows(1)
    mirt.set_frames_in_flight(1)
    mirt.shutdown()


def case(oracle, scene, lset):
    """(triangles, records, lights, samples, jitter or None, the light positions, the oracle's DirectLight), once per (scene, set);
    leaves the scene uploaded.  3 x 11 and 16 x 16 are test_gpu_many_lights' cases; 2 hard lights are made the same way."""
    if lset != "2x1":
        tris, recs, L, samples, jit, want = many_case(oracle, scene, lset)
        return tris, recs, L, samples, jit, jit, want
    tris, hits = scene_hits(scene)
    key = (scene, lset)
    if key not in _cases:
        L = lights_of(2)
        recs = hits.copy()
        n = len(tris)
        ids = np.flatnonzero(recs["index"] >= 0)
        recs["index"][ids[3]] = -1
        recs["index"][ids[5::97]] = n
        recs["position"][ids[10]][1] = np.float32("nan")
        recs["position"][ids[20]] = L[1, :3]
        want = rq.oracle_direct_light(oracle, tris, recs, L)
        assert np.isnan(want).any() and (want[np.isfinite(want).all(axis=1)] > 0).any()
        want.setflags(write=False)
        _cases[key] = (tris, recs, L, 1, None, np.ascontiguousarray(L[:, :3]), want)
    return _cases[key]


def soft(samples, jit):
    mirt.set_soft_shadows(samples, jit if samples > 1 else None)


def device_mask(recs, L, npos, guard=0):
    """mirt_shadow_mask_device into a pre-filled buffer with `guard` words behind the last plane: (planes, guard words)."""
    words = mirt.mask_words(npos)
    d_hits = to_device(recs)
    with DeviceArray((words * len(recs) + guard,), np.uint32, FILL) as d_mask:
        mirt.shadow_mask_device(d_hits.ptr, len(recs), L, d_mask.ptr)
        got = d_mask.read()
    d_hits.free()
    return got[:words * len(recs)].reshape(words, len(recs)), got[words * len(recs):]


def device_relight(recs, L, mask):
    d_hits, d_mask = to_device(recs), to_device(mask)
    with DeviceArray((len(recs), 3), np.float32, FILL) as d_rgb:
        mirt.direct_light_masked_device(d_hits.ptr, len(recs), L, d_mask.ptr, d_rgb.ptr)
        got = d_rgb.read()
    d_hits.free()
    d_mask.free()
    return got


def bit_matrix(mask, npos):
    """(records, positions) booleans of a (words, records) mask."""
    j = np.arange(npos)
    return ((mask[j >> 5, :] >> (j & 31).astype(np.uint32)[:, None]) & 1).T.astype(bool)


# ---- 1. mask, then relight, is DirectLight -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lset", list(SETS))
@pytest.mark.parametrize("scene", SCENES)
def test_mask_then_relight_equals_direct_light_and_the_oracle(oracle, scene, lset):
    tris, recs, L, samples, jit, P, want = case(oracle, scene, lset)
    npos, words = len(P), mirt.mask_words(len(P))
    one = np.flatnonzero((recs["index"] >= 0) & (recs["index"] < len(tris)))[7]
    soft(samples, jit)
    masks = {}
    try:
        for mname, mode in MODES:
            mirt.set_query_mode(mode)
            what = "%s %s %s" % (scene, lset, mname)
            rq.same_bits(mirt.direct_light(recs, L), want, what + ": direct_light itself")
            mask = mirt.shadow_mask(recs, L)
            st = mirt.shadow_mask_stats()
            assert mask.shape == (words, len(recs)) and mask.dtype == np.uint32, what
            if mode != mirt.QUERY_AUTO:
                assert st["mode_used"] == mode, (what, st)
            assert (st["cube_source"] != 0) == (st["mode_used"] == mirt.QUERY_BINNED), (what, st)
            if npos % 32:
                assert not (mask[-1] >> np.uint32(npos % 32)).any(), what + ": bits beyond the positions"
            rq.same_bits(mirt.direct_light_masked(recs, L, mask), want, what + " host")
            dmask, _ = device_mask(recs, L, npos)
            assert np.array_equal(dmask, mask), what + ": device mask"
            rq.same_bits(device_relight(recs, L, dmask), want, what + " device")
            m1 = mirt.shadow_mask(recs[one:one + 1], L)
            assert np.array_equal(m1, mask[:, one:one + 1]), what + ": single record's mask"
            rq.same_bits(mirt.direct_light_masked(recs[one:one + 1], L, m1), want[one:one + 1], what + " single record")
            masks[mname] = mask
        assert np.array_equal(masks["brute"], masks["binned"]) and np.array_equal(masks["auto"], masks["brute"])
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
        mirt.set_soft_shadows(1)


# ---- 2. the bits are DirectLight's decisions, from the oracle alone ---------------------------------------------------------------------

def oracle_decisions(oracle, scene, lset):
    """(hit records, (records, positions) booleans): raytracer.cpp:306-315 per pair with the oracle's own operations -- r =
    distance(pos, P), rDir = normalize(P - pos), ClosestIntersection(P, -rDir) on a fresh record, any && j.distance < r * 0.99f."""
    key = (scene, lset)
    if key not in _decisions:
        tris, hits = scene_hits(scene)
        L = lights_of(SETS[lset][0])
        P = np.ascontiguousarray(L[:, :3]) if SETS[lset][1] == 1 else rq.jitter(oracle, L, SETS[lset][1], seed=3)
        recs = hits[hits["index"] >= 0]
        lib = oracle.lib
        bits = np.zeros((len(recs), len(P)), bool)
        rdir = np.zeros(3, np.float32)
        for i, pos in enumerate(np.ascontiguousarray(recs["position"], np.float32)):
            for j, p in enumerate(P):
                r = np.float32(lib.mirt_oracle_distance(pos, p))
                lib.mirt_oracle_normalize((p - pos).astype(np.float32), rdir)
                hit, _, dist, _ = oracle.closest_intersection(tris, p, (-rdir).astype(np.float32))
                bits[i, j] = hit and dist < r * np.float32(0.99)
        bits.setflags(write=False)
        _decisions[key] = (recs, L, P, bits)
    return _decisions[key]


@pytest.mark.parametrize("lset", ["2x1", "3x11"])
@pytest.mark.parametrize("scene,lo,hi", [("cornell", 0.25, 0.45), ("soup2000", 0.8, 0.95)])
def test_bits_are_the_oracles_shadow_decisions(oracle, scene, lo, hi, lset):
    recs, L, P, want = oracle_decisions(oracle, scene, lset)
    samples = SETS[lset][1]
    share, per_position = want.mean(), want.mean(axis=0)
    print("%s %s: %d hit records, share of set bits %.3f, per position %.3f .. %.3f" % (scene, lset, len(recs), share, per_position.min(), per_position.max()))
    assert (want.any(axis=0) & ~want.all(axis=0)).all(), "a position's column holds one value only"
    assert lo <= share <= hi, share
    soft(samples, P)
    try:
        for mname, mode in MODES[:2]:
            mirt.set_query_mode(mode)
            got = bit_matrix(mirt.shadow_mask(recs, L), len(P))
            assert np.array_equal(got, want), "%s %s %s: %d decisions differ" % (scene, lset, mname, int((got != want).sum()))
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
        mirt.set_soft_shadows(1)


# ---- 3. the index is not read ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [mirt.QUERY_BRUTE, mirt.QUERY_BINNED])
def test_the_index_is_not_read(oracle, mode):
    tris, recs, L, samples, jit, P, want = case(oracle, "soup2000", "3x11")
    soft(samples, jit)
    mirt.set_query_mode(mode)
    try:
        masks = []
        for index in (-1, len(tris), 0):
            points = recs.copy()
            points["index"] = index
            masks.append(mirt.shadow_mask(points, L))
            if index != 0:
                assert not mirt.direct_light_masked(points, L, masks[-1]).view(np.uint32).any(), index
        assert np.array_equal(masks[0], masks[1]) and np.array_equal(masks[0], masks[2])
        assert np.array_equal(masks[0], mirt.shadow_mask(recs, L)) and masks[0].any()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
        mirt.set_soft_shadows(1)


# ---- 4. exact extent -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [mirt.QUERY_BRUTE, mirt.QUERY_BINNED])
def test_exactly_the_masks_words_are_written(oracle, mode):
    tris, recs, L, samples, jit, P, want = case(oracle, "soup2000", "3x11")
    soft(samples, jit)
    mirt.set_query_mode(mode)
    try:
        full = mirt.shadow_mask(recs, L)
        for nhits in (1, 63, 64, 65, 257, 513):
            planes, guard = device_mask(recs[:nhits], L, 33, guard=64)
            assert (planes != FILLW).sum() == 2 * nhits, nhits
            assert not (planes[1] >> np.uint32(1)).any(), "%d: bits 1 .. 31 of plane 1" % nhits
            assert (guard == FILLW).all(), "%d: words behind the last plane written" % nhits
            assert np.array_equal(planes, full[:, :nhits]), nhits
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
        mirt.set_soft_shadows(1)


# ---- 5. relighting ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", SCENES)
def test_relighting_from_a_kept_mask(oracle, scene):
    tris, recs, L, samples, jit, P, want = case(oracle, scene, "3x11")
    soft(samples, jit)
    try:
        mask = mirt.shadow_mask(recs, L)
        # every colour and intensity changed: the bits depend on positions only
        L2 = L.copy()
        L2[:, 3:6] = np.array([[0.5, 1.0, 0.25], [1.0, 0.75, 0.5], [0.75, 0.25, 1.0]], np.float32)
        L2[:, 6] = [5, 11, 2]
        assert not np.array_equal(L2[:, 3:], L[:, 3:])
        recoloured = rq.oracle_direct_light(oracle, tris, recs, L2, samples=samples, jitter=jit)
        assert not np.array_equal(recoloured.view(np.uint32), want.view(np.uint32))
        rq.same_bits(mirt.direct_light_masked(recs, L2, mask), recoloured, "recoloured lights against the oracle")
        rq.same_bits(mirt.direct_light(recs, L2), recoloured, "recoloured lights against direct_light")
        # the last light deleted, `samples` unchanged: a prefix of the planes at the same stride
        two = rq.oracle_direct_light(oracle, tris, recs, L[:2], samples=samples, jitter=jit[:2 * samples])
        rq.same_bits(mirt.direct_light_masked(recs, L[:2], mask), two, "two of three lights against the oracle")
        rq.same_bits(mirt.direct_light(recs, L[:2]), two, "two of three lights against direct_light")
        assert np.array_equal(mirt.shadow_mask(recs, L[:2])[0], mask[0] & np.uint32((1 << 22) - 1))
        # all clear: DirectLight in a scene that holds the record's own triangle only (that shadow ray ends at r, not below 0.99 r)
        clear = mirt.direct_light_masked(recs, L, np.zeros_like(mask))
        alone = np.zeros_like(clear)
        for i, h in enumerate(recs):
            if 0 <= h["index"] < len(tris):
                alone[i] = oracle.direct_light(tris[h["index"]:h["index"] + 1], h["position"], float(h["distance"]), 0, L, samples=samples, jitter=jit)
        rq.same_bits(clear, alone, "an all-clear mask")
        assert not np.array_equal(clear.view(np.uint32), want.view(np.uint32))
        # all set: 0 x colour
        assert not mirt.direct_light_masked(recs, L, np.full_like(mask, 0xFFFFFFFF)).view(np.uint32).any()
    finally:
        mirt.set_soft_shadows(1)


# ---- 6. shared cubes, untouched statistics ---------------------------------------------------------------------------------------------------

def test_cubes_are_shared_with_direct_light_and_other_statistics_stay(oracle):
    tris, recs, L, samples, jit, P, want = case(oracle, "soup2000", "3x11")
    soft(samples, jit)
    mirt.set_query_mode(mirt.QUERY_BINNED)
    try:
        mirt.scene_upload(tris)                                  # a new scene version: no cube is held
        rq.same_bits(mirt.direct_light(recs, L), want, "direct_light builds")
        assert mirt.query_stats()["cube_source"] == 1
        mirt.intersect_from(rq.INSIDE, recs["position"][:64])
        mirt.occluded(mirt.make_rays(rq.INSIDE, recs["position"][:64]))
        before = (mirt.query_stats(), mirt.fan_stats(), mirt.occlusion_stats())
        mask = mirt.shadow_mask(recs, L)
        st = mirt.shadow_mask_stats()
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2 and st["cube_bins"] > 0, st
        rq.same_bits(mirt.direct_light_masked(recs, L, mask), want, "relight")
        assert (mirt.query_stats(), mirt.fan_stats(), mirt.occlusion_stats()) == before
        assert mirt.shadow_mask_stats() == st, "the masked call keeps no statistics"

        mirt.scene_upload(tris)                                  # ... and the reverse
        assert np.array_equal(mirt.shadow_mask(recs, L), mask)
        assert mirt.shadow_mask_stats()["cube_source"] == 1
        rq.same_bits(mirt.direct_light(recs, L), want, "direct_light after the mask's build")
        assert mirt.query_stats()["cube_source"] == 2

        mirt.set_profiling(True)
        assert np.array_equal(mirt.shadow_mask(recs, L), mask)
        binned = mirt.shadow_mask_stats()
        mirt.set_query_mode(mirt.QUERY_BRUTE)
        assert np.array_equal(mirt.shadow_mask(recs, L), mask)
        brute = mirt.shadow_mask_stats()
        assert binned["mode_used"] == mirt.QUERY_BINNED and brute["mode_used"] == mirt.QUERY_BRUTE and brute["cube_source"] == 0
        assert binned["shadow_rays"] == brute["shadow_rays"] == len(recs) * len(P), (binned, brute)
        assert 0 < binned["tests"] < brute["tests"], (binned, brute)
    finally:
        mirt.set_profiling(False)
        mirt.set_query_mode(mirt.QUERY_AUTO)
        mirt.set_soft_shadows(1)


# ---- 7. four frames in flight ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [mirt.QUERY_BRUTE, mirt.QUERY_BINNED])
def test_four_calls_in_flight(oracle, mode):
    tris, recs, L, samples, jit, P, want = case(oracle, "soup2000", "3x11")
    soft(samples, jit)
    mirt.set_query_mode(mode)
    try:
        mask = mirt.shadow_mask(recs, L)                         # one stream
        rq.same_bits(mirt.direct_light_masked(recs, L, mask), want, "one stream")
        lens = (len(recs), 513, 257, 65)
        mirt.set_frames_in_flight(4)
        d_hits = [to_device(recs[:n]) for n in lens]
        d_masks = [DeviceArray((2, n), np.uint32, FILL) for n in lens]
        d_rgbs = [DeviceArray((n, 3), np.float32, FILL) for n in lens]
        try:
            for h, m, n in zip(d_hits, d_masks, lens):
                mirt.shadow_mask_device(h.ptr, n, L, m.ptr)
            # (the streams take the calls in turn: call k of these four follows call k of those four on its stream)
            for h, m, c, n in zip(d_hits, d_masks, d_rgbs, lens):
                mirt.direct_light_masked_device(h.ptr, n, L, m.ptr, c.ptr)
            mirt.sync()
            for m, c, n in zip(d_masks, d_rgbs, lens):
                assert np.array_equal(m.read(), mask[:, :n]), n
                rq.same_bits(c.read(), want[:n], "%d records" % n)
        finally:
            for d in d_hits + d_masks + d_rgbs:
                d.free()
    finally:
        mirt.set_frames_in_flight(1)
        mirt.set_query_mode(mirt.QUERY_AUTO)
        mirt.set_soft_shadows(1)
