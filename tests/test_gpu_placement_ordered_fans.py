"""The ordered hits from shared origins on scenes placed away from the world origin: mirt_intersect_ordered_from* and
mirt_intersect_ordered_fans* on soup2000 and the tie scene at the placements of tests/placement.py, origins moved with the scene, BINNED
and BRUTE with max_hits 4, against the CPU oracle on the placed float32 inputs, byte for byte.  The cubes bin everywhere the one-hit
fan calls bin: what mirt_intersect_from / mirt_intersect_fans report for the placement -- the library is asked, nothing is written
down here -- is what the ordered call must report."""
import numpy as np
import pytest

import mirt
import ordered_fans_helpers as F
import ordered_helpers as O
import placement as pl

pytestmark = pytest.mark.gpu

BRUTE, BINNED, AUTO = mirt.QUERY_BRUTE, mirt.QUERY_BINNED, mirt.QUERY_AUTO
PLACES = ("3_0_0", "300_200_-100", "1000_1000_1000", "0_0_4096", "origin_x1024", "origin_div1024")
NRAYS, HITS = 257, 4
_cases = {}


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_query_mode(mirt.QUERY_AUTO)
    mirt.shutdown()


def placed_case(oracle, scene, pname):
    """The placed scene, five origins and NRAYS directions moved with it (the unit batch of ordered_fans_helpers: seams and random
    directions, origins mixed), and the oracle's answers for the many-origin rays and for all directions from origin 0."""
    key = scene, pname
    if key not in _cases:
        T, s = pl.PLACEMENTS[pname]
        unit = pl.unit_scene(scene)
        origins = F.origins_for(np.asarray(unit).reshape(-1, 15), 5)
        of, dirs = F.make_batch(origins, 1.0, 0)
        of, dirs = np.ascontiguousarray(of[:NRAYS]), pl.place_dirs(dirs[:NRAYS], s)
        tris, origins = pl.placed_scene(scene, pname), pl.place(origins, T, s)
        many = O.peel(oracle, tris, mirt.make_rays(origins[of], dirs), HITS)
        one = O.peel(oracle, tris, mirt.make_rays(np.broadcast_to(origins[0], (NRAYS, 3)), dirs), HITS)
        _cases[key] = tris, origins, of, dirs, many, one
    return _cases[key]


@pytest.mark.parametrize("pname", PLACES)
@pytest.mark.parametrize("scene", ["soup2000", pl.TIE_SCENE])
def test_placed(oracle, scene, pname):
    tris, origins, of, dirs, many, one = placed_case(oracle, scene, pname)
    assert (many[1] >= 2).mean() >= 0.2 and (one[1] >= 2).mean() >= 0.2, "the placed batch hits too little"
    if scene == pl.TIE_SCENE:
        h, c = many
        tie = (c >= 2) & (h["distance"][:, 0] == h["distance"][:, 1]) & (h["index"][:, 1] < h["index"][:, 0])
        assert tie.sum() >= 3, "no tie pair in slots 0 / 1"
    mirt.scene_upload(tris)
    # what the one-hit calls do on this placement
    mirt.set_query_mode(BINNED)
    try:
        mirt.intersect_fans(origins, of, dirs)
        fans_mode = mirt.fan_stats()["mode_used"]
        mirt.intersect_from(origins[0], dirs)
        from_mode = mirt.fan_stats()["mode_used"]
    finally:
        mirt.set_query_mode(AUTO)
    for form in ("host", "device"):
        for o, idx, want, binned_mode, family in ((origins, of, many, fans_mode, "fans"), (origins[0], None, one, from_mode, "from")):
            what = "%s at %s, %s, %s form" % (scene, pname, family, form)
            got = F.ordered_fans(form, o, idx, dirs, HITS, mode=BRUTE, what=what)
            assert got[2]["mode_used"] == BRUTE, (what, got[2])
            F.same(got, want, what + ", brute")
            got = F.ordered_fans(form, o, idx, dirs, HITS, mode=BINNED, what=what)
            assert got[2]["mode_used"] == binned_mode, (what, got[2])
            F.same(got, want, what + ", binned")
