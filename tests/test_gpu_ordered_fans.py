"""Every hit along rays from shared origins, in order, on the GPU: mirt_intersect_ordered_from* (k_fan_order) and
mirt_intersect_ordered_fans* (k_fans_order) through the cubes around the origins, and by the sweep over the rays written out, against
the CPU oracle, byte for byte.

The expectation is ordered_helpers.peel / from_table on the rays {origins[origin_of[i]], dirs[i]} (ordered_fans_helpers.case: computed
once per case, read-only).  Every call goes through buffers prefilled with 0xAA with guard records and guard counts behind them: each
slot and count of the call is written, and nothing beyond.  The batches are test_gpu_fans_query.py's: the 182 seam directions of every
origin among random ones, origins mixed within every wave."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mirt
import ordered_fans_helpers as F
import ordered_helpers as O
from devbuf import DeviceArray, hip, hip_fill, to_device
from query_helpers import INSIDE, LIGHTS, OUTSIDE

pytestmark = pytest.mark.gpu

INVALID = -3
INT_MAX = np.iinfo(np.int32).max
BRUTE, BINNED, AUTO = mirt.QUERY_BRUTE, mirt.QUERY_BINNED, mirt.QUERY_AUTO
BOTH = (("brute", BRUTE), ("binned", BINNED))
REC = F.REC
call = F.ordered_fans
same = F.same
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_query_mode(mirt.QUERY_AUTO)
    mirt.set_profiling(False)
    mirt.set_frames_in_flight(1)
    mirt.shutdown()


def mode_is(st, mode, what, source=None):
    if mode == BRUTE:
        assert st["mode_used"] == BRUTE and st["cube_source"] == 0 and st["cube_bins"] == 0, (what, st)
    else:
        assert st["mode_used"] == BINNED and st["cube_source"] in ((1, 2) if source is None else (source,)) and st["cube_bins"] in (64, 128, 256) \
            and st["shells"] >= 1, (what, st)


def fresh_slot0(h, c, fresh, what):
    """Slot 0 without `after` is the one-hit fan call on fresh records, all 20 bytes."""
    hit = c > 0
    assert np.array_equal(hit, fresh["index"] >= 0), what
    assert h[:, 0][hit].tobytes() == fresh[hit].tobytes(), what + ": slot 0 is not the one-hit call's record"
    assert h[:, 0][~hit].tobytes() == mirt.fresh_hits(int((~hit).sum())).tobytes(), what


# ---- 1: records, counts and trailing fresh slots; modes, forms and which path ran -----------------------------------------------------------

CASES = (("soup2000", 1, 2049), ("soup2000", 5, 2049), ("cornell", 5, 1025), ("soup65x2", 5, 1025), ("cornell+soup2000", 5, 2049), ("one", 2, 257))


@pytest.mark.parametrize("key", CASES, ids=lambda k: "%s-%d" % k[:2])
def test_records_equal_the_oracle(oracle, key):
    name, K, nrays = key
    tris, origins, of, dirs, rays, want10 = F.case(oracle, *key)
    if key in F.FLOORS:
        F.floors_hold(key, want10)
    single = K == 1
    mirt.scene_upload(tris)
    fresh = mirt.intersect_fans(origins, of, dirs)
    first = True
    cases = [(n, m, "host") for n in (1, 63, 65, 257) for m in F.HITS] + [(65, 4, "device"), (min(2049, nrays), 8, "device"), (min(2049, nrays), 1, "device")]
    for n, m, form in cases:
        want = F.prefix(want10, n, m)
        got = {}
        for mname, mode in (("brute", BRUTE), ("binned", BINNED), ("auto", AUTO)):
            what = "%s, %d origins, %d rays, max_hits %d, %s form, %s" % (name, K, n, m, form, mname)
            got[mname] = call(form, origins[0] if single else origins, of[:n], dirs[:n], m, mode=mode, what=what)
            st = got[mname][2]
            if mode == AUTO:                                         # (the cube of the BINNED call in front is held: AUTO takes it)
                mode_is(st, BINNED, what, 2)
            elif mode == BINNED:
                mode_is(st, BINNED, what, 1 if first else 2)         # (a fresh upload: built by the first call, held from then on)
                first = False
            else:
                mode_is(st, BRUTE, what)
            same(got[mname], want, what + " vs the oracle")
        same(got["binned"], got["brute"], "%s, %d rays, max_hits %d: BINNED vs BRUTE" % (name, n, m))
        fresh_slot0(got["binned"][0], got["binned"][1], fresh[:n], what)
    if single:
        # the single-origin call and the fans call of one origin give the same bytes (with and without indices)
        one = call("device", origins[0], None, dirs, 4, mode=BINNED)
        for idx in (None, of):
            many = call("device", origins, idx, dirs, 4, mode=BINNED)
            assert one[0].tobytes() == many[0].tobytes() and one[1].tobytes() == many[1].tobytes()


def test_auto_with_nothing_held(oracle):
    """AUTO is the fan calls' own rule: for several origins on soup2000 BRUTE at 4096 rays and BINNED at 4097; from one origin BINNED from
    one ray on; cornell never bins."""
    tris, origins, of, dirs, rays, want = F.case(oracle, "soup2000", 5, 4097, 2)
    assert len(dirs) == 4097
    for n, mode in ((4096, BRUTE), (4097, BINNED)):
        mirt.scene_upload(tris)                                     # (a new scene version: nothing is held)
        got = call("device", origins, of[:n], dirs[:n], 2, mode=AUTO)
        mode_is(got[2], mode, "AUTO, %d rays" % n, None if mode == BRUTE else 1)
        same(got, F.prefix(want, n, 2), "soup2000, AUTO with nothing held, %d rays" % n)
    tris, origins, of, dirs, rays, want = F.case(oracle, "soup2000", 1, 2049)
    for n in (1, 65):
        mirt.scene_upload(tris)
        got = call("host", origins[0], None, dirs[:n], 3, mode=AUTO)
        mode_is(got[2], BINNED, "one origin, AUTO, %d rays" % n, 1)
        same(got, F.prefix(want, n, 3), "soup2000, one origin, AUTO, %d rays" % n)
    tris, origins, of, dirs, rays, want = F.case(oracle, "cornell", 5, 1025)
    mirt.scene_upload(tris)
    for single in (False, True):
        got = call("host", origins[0] if single else origins, None if single else of, dirs, 4, mode=AUTO)
        mode_is(got[2], BRUTE, "cornell, AUTO")
        if not single:
            same(got, F.prefix(want, 1025, 4), "cornell, AUTO")


def test_the_wrappers_return_the_same(oracle):
    tris, origins, of, dirs, rays, want = F.case(oracle, "soup2000", 5, 2049)
    mirt.scene_upload(tris)
    mirt.set_query_mode(BINNED)
    try:
        hits, counts = mirt.intersect_ordered_fans(origins, of[:257], dirs[:257], 4)
        assert hits.shape == (257, 4) and counts.shape == (257,)
        same((hits, counts), F.prefix(want, 257, 4), "mirt.intersect_ordered_fans")
        one = F.case(oracle, "soup2000", 1, 2049)
        hits, counts = mirt.intersect_ordered_from(one[1][0], one[3][:257], 3)
        same((hits, counts), F.prefix(one[5], 257, 3), "mirt.intersect_ordered_from")
        assert mirt.intersect_ordered_from(INSIDE, dirs[:0], 4)[0].shape == (0, 4)
    finally:
        mirt.set_query_mode(AUTO)


# ---- 2: passes, and indices that name no origin ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [32, 33, 70])
def test_passes_and_stray_indices(oracle, K):
    # (33 origins: the case of the floors' table; 32 and 70: the batch of fewest rays, 16 random ones an origin, peeled to the 4 hits asked for)
    tris, origins, of, dirs, rays, want = F.case(oracle, "soup2000", K, 6534) if K == 33 else F.case(oracle, "soup2000", K, 0, 4)
    n = len(dirs)
    assert len(np.unique(of)) == K and all(len(np.unique(of[w:w + 64])) > 1 for w in range(0, n - 64, 64)), "a wave with one origin only"
    mirt.scene_upload(tris)
    bad_of = of.copy()
    bad = np.concatenate([w + np.array([1, 30, 63]) for w in range(0, n - 64, 64)])
    bad_of[bad[0::3]] = -1
    bad_of[bad[1::3]] = K
    bad_of[bad[2::3]] = INT_MAX
    stray = np.zeros(n, bool)
    stray[bad] = True
    w4 = F.prefix(want, n, 4)
    for mname, mode in BOTH:
        what = "soup2000, %d origins, max_hits 4, %s" % (K, mname)
        got = call("device", origins, of, dirs, 4, mode=mode, what=what)
        mode_is(got[2], mode, what)
        same(got, w4, what)
        got = call("device", origins, bad_of, dirs, 4, mode=mode, what=what + ", stray indices", stray=stray)
        mode_is(got[2], mode, what)
        assert (got[1][stray] == 0).all(), what + ": the count of a stray ray is not 0"
        same((got[0][~stray], got[1][~stray]), (w4[0][~stray], w4[1][~stray]), what + ": the rays around the strays")
    # the host form refuses the same array and writes nothing
    lib, P = mirt.load(), mirt._ptr
    hbuf, cbuf = F.guarded_host(n, 4)
    before = hbuf.tobytes(), cbuf.tobytes()
    assert lib.mirt_intersect_ordered_fans(P(origins), K, P(bad_of), P(dirs), n, None, 4, P(hbuf), P(cbuf)) == INVALID
    assert b"origin_of[%d]" % bad[0] in lib.mirt_last_error()
    assert (hbuf.tobytes(), cbuf.tobytes()) == before


# ---- 3: `after` records, and the in-place peel -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["soup2000", "soup65x2"])
def test_after_records(oracle, name):
    """`after` records of every kind of ordered_helpers.after_records, at every rotation, against the per-triangle table sorted as the
    contract words it."""
    n = 257
    tris, origins, of, dirs, rays, want10 = F.case(oracle, name, 5, {"soup2000": 2049, "soup65x2": 1025}[name])
    of, dirs, rays = of[:n], dirs[:n], rays[:n]
    rec = O.table(oracle, tris, rays)
    same(O.from_table(rec, None, 8), F.prefix(want10, n, 8), name + ": table vs peel")
    mirt.scene_upload(tris)
    slot0 = O.from_table(rec, None, 1)[0][:, 0]
    on_a_hit = np.zeros(O.AFTER_KINDS, bool)
    for shift in range(O.AFTER_KINDS):
        after, kind = O.after_records(slot0, shift)
        on_a_hit[np.unique(kind[slot0["index"] >= 0])] = True
        for m in (1, 2, 8):
            want = O.from_table(rec, after, m)
            for mname, mode in BOTH:
                for form in ("host", "device"):
                    what = "%s, after kinds from %d on, max_hits %d, %s, %s form" % (name, shift, m, mname, form)
                    got = call(form, origins, of, dirs, m, after=after, mode=mode, what=what)
                    mode_is(got[2], mode, what)
                    same(got, want, what)
    assert on_a_hit.all()


@pytest.mark.parametrize("form", ["host", "device"])
def test_the_in_place_peel_over_two_passes(oracle, form):
    """after == hits with max_hits 1, repeated until every count is 0, equals the peel to 10 hits; 33 origins: two passes write into the
    one array."""
    tris, origins, of, dirs, rays, want = F.case(oracle, "soup2000", 33, 6534)
    hits, counts = want
    deep = int(counts.max())
    assert 8 < deep < F.CAP, "the oracle's peel to %d hits must show every hit of every ray, and more than 8 of some" % F.CAP
    mirt.scene_upload(tris)
    for mname, mode in BOTH:
        recs, cnts = F.peel_in_place(form, origins, of, dirs, mode, F.CAP + 1)
        assert len(recs) == deep + 1, "the peel ran %d rounds, the deepest ray has %d hits" % (len(recs), deep)
        for r in range(deep + 1):
            live = counts > r
            what = "in-place peel, round %d, %s, %s form" % (r, mname, form)
            assert np.array_equal(cnts[r], live.astype(np.int32)), what
            assert recs[r][live].tobytes() == np.ascontiguousarray(hits[live, r]).tobytes(), what
            assert recs[r][~live].tobytes() == mirt.fresh_hits(int((~live).sum())).tobytes(), what
    assert mirt.fan_stats()["mode_used"] == BINNED


# ---- 4: directions the cube does not take ------------------------------------------------------------------------------------------------------

def test_directions_outside_the_window_sweep(oracle):
    tris, origins, of, dirs, rays, _ = F.case(oracle, "soup2000", 5, 2049)
    n = 513
    of, dirs = of[:n], dirs[:n].copy()
    ordinary = np.flatnonzero((np.abs(dirs).max(axis=1) > 1e-3) & (np.abs(dirs).max(axis=1) < 1e3) & (np.abs(dirs).min(axis=1) > 0))
    odd = np.intersect1d(np.concatenate([w + np.array([3, 17, 40]) for w in range(0, n - 64, 64)]), ordinary)
    kept = np.setdiff1d(ordinary, odd)[:14]
    assert len(odd) >= 15                                           # (each of the five kinds three times)
    for k, i in enumerate(odd):
        unit = dirs[i] / np.abs(dirs[i]).max()                      # largest component exactly +-1
        kind = k % 5
        if kind == 0:
            dirs[i] = 0
        elif kind == 1:
            dirs[i][k % 3] = np.float32("nan")
        elif kind == 2:
            dirs[i][k % 3] = np.float32("inf") * (1 if k % 2 else -1)
        elif kind == 3:
            dirs[i] = unit * np.float32(2.0 ** -40)
        else:
            dirs[i] = unit * np.float32(2.0 ** 20)
    for k, i in enumerate(kept):                                    # these stay binned
        dirs[i] = dirs[i] / np.abs(dirs[i]).max() * np.float32(2.0 ** -32 if k % 2 else 2.0 ** 18)
    want = O.peel(oracle, tris, mirt.make_rays(origins[of], dirs), 8)
    assert (want[1][odd[3::5]] > 0).any() and (want[1][odd[4::5]] > 0).any() and (want[1][kept] > 0).any()
    mirt.scene_upload(tris)
    mirt.set_profiling(True)
    try:
        for m in (1, 4, 8):
            got = call("device", origins, of, dirs, m, mode=BINNED)
            st = got[2]
            assert st["mode_used"] == BINNED and st["fallback_records"] == len(odd) and st["shadow_rays"] == n, (st, len(odd))
            same(got, F.prefix(want, n, m), "directions outside the window, max_hits %d" % m)
    finally:
        mirt.set_profiling(False)
    same(call("host", origins, of, dirs, 8, mode=BRUTE), want, "directions outside the window, brute")


# ---- 5: origins the frame path would not bin ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["1e9", "nan"])
def test_unbinnable_origin(oracle, what):
    tris, origins, of, dirs, rays, _ = F.case(oracle, "soup2000", 5, 2049)
    n = 257
    origins = origins.copy()
    origins[3] = {"1e9": (1e9, 0, 0), "nan": (0.1, np.nan, 0.2)}[what]
    want = O.peel(oracle, tris, mirt.make_rays(origins[of[:n]], dirs[:n]), 4)
    assert (want[1][of[:n] != 3] >= 2).sum() > 50
    mirt.scene_upload(tris)
    for mname, mode in (("brute", BRUTE), ("auto", AUTO), ("binned", BINNED)):
        got = call("device", origins, of[:n], dirs[:n], 4, mode=mode)
        mode_is(got[2], BRUTE, "origin %s among ordinary ones, %s" % (what, mname))
        same(got, want, "origin %s among ordinary ones, %s" % (what, mname))
    got = call("host", origins[3], None, dirs[:n], 4, mode=BINNED)
    mode_is(got[2], BRUTE, "the single origin " + what)
    same(got, O.peel(oracle, tris, mirt.make_rays(np.broadcast_to(origins[3], (n, 3)), dirs[:n]), 4), "the single origin " + what)


# ---- 6: shared cubes ----------------------------------------------------------------------------------------------------------------------------

def test_shared_cubes(oracle):
    tris, origins, of, dirs, rays, want = F.case(oracle, "soup2000", 5, 2049)
    n = 513
    of, dirs = of[:n], dirs[:n]
    w4 = F.prefix(want, n, 4)
    one = F.case(oracle, "soup2000", 1, 2049)
    mirt.set_query_mode(BINNED)
    try:
        # a cube mirt_intersect_fans built serves the ordered call, and the other way round; likewise mirt_occluded_fans
        mirt.scene_upload(tris)
        mirt.intersect_fans(origins, of, dirs)
        assert mirt.fan_stats()["cube_source"] == 1
        got = call("device", origins, of, dirs, 4, mode=BINNED)
        mode_is(got[2], BINNED, "after mirt_intersect_fans", 2)
        same(got, w4, "through mirt_intersect_fans' cube")
        mirt.scene_upload(tris)
        got = call("device", origins, of, dirs, 4, mode=BINNED)
        mode_is(got[2], BINNED, "fresh upload", 1)
        mirt.set_query_mode(BINNED)
        mirt.intersect_fans(origins, of, dirs)
        assert mirt.fan_stats()["cube_source"] == 2
        mirt.occluded_fans(origins, of, dirs)
        assert mirt.occlusion_stats()["cube_source"] == 2
        mirt.scene_upload(tris)
        mirt.occluded_fans(origins, of, dirs)
        assert mirt.occlusion_stats()["cube_source"] == 1
        got = call("device", origins, of, dirs, 4, mode=BINNED)
        mode_is(got[2], BINNED, "after mirt_occluded_fans", 2)
        same(got, w4, "through mirt_occluded_fans' cube")
        # the single fan's cube likewise
        mirt.set_query_mode(BINNED)
        mirt.intersect_from(one[1][0], one[3][:n])
        assert mirt.fan_stats()["cube_source"] == 1
        got = call("device", one[1][0], None, one[3][:n], 4, mode=BINNED)
        mode_is(got[2], BINNED, "after mirt_intersect_from", 2)
        same(got, F.prefix(one[5], n, 4), "through mirt_intersect_from's cube")
        # origins equal to the positions of DirectLight's cube read that cube
        mirt.set_query_mode(BINNED)
        recs = mirt.intersect_fans(origins, of, dirs)
        recs = recs[recs["index"] >= 0]
        mirt.direct_light(recs, LIGHTS)
        qs = mirt.query_stats()
        assert qs["mode_used"] == BINNED and qs["cube_source"] == 1, qs
        lpos = np.ascontiguousarray(LIGHTS[:, :3])
        lof = (of % 2).astype(np.int32)
        got = call("device", lpos, lof, dirs[:129], 4, mode=BINNED)
        st = got[2]
        assert st["mode_used"] == BINNED and st["cube_source"] == 4 and st["cube_bins"] == qs["cube_bins"] and st["shells"] == qs["shells"], st
        same(got, O.peel(oracle, tris, mirt.make_rays(lpos[lof[:129]], dirs[:129]), 4), "through DirectLight's cube")
        assert mirt.query_stats() == qs
        # the scene moves: the cube is built again, and the answers follow the scene
        got = call("device", origins, of, dirs, 4, mode=BINNED)
        mode_is(got[2], BINNED, "before the move", 2)
        rot = np.array([0, 1, 0, -1, 0, 0, 0, 0, 1], np.float32)
        mirt.scene_transform(0, len(tris), rot, np.array([0.25, -0.125, 0.0625], np.float32))
        moved = O.peel(oracle, mirt.scene_download(), mirt.make_rays(origins[of[:129]], dirs[:129]), 4)
        got = call("device", origins, of[:129], dirs[:129], 4, mode=BINNED)
        mode_is(got[2], BINNED, "after scene_transform", 1)
        same(got, moved, "after scene_transform")
        assert not np.array_equal(moved[0]["index"], w4[0]["index"][:129])
    finally:
        mirt.set_query_mode(AUTO)
        mirt.scene_upload(tris)


# ---- 7: profiling on ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 5, 33])
def test_profiling_on(oracle, K):
    tris, origins, of, dirs, rays, want = F.case(oracle, "soup2000", K, {1: 2049, 5: 2049, 33: 6534}[K])
    n = min(len(dirs), 2049)
    mirt.scene_upload(tris)
    tests = {}
    mirt.set_profiling(True)
    try:
        for m in F.HITS:
            got = call("device", origins[0] if K == 1 else origins, of[:n], dirs[:n], m, mode=BINNED)
            st = got[2]
            assert st["mode_used"] == BINNED and st["shadow_rays"] == n and st["fallback_records"] == 0 and 0 < st["tests"] <= st["candidates"], st
            same(got, F.prefix(want, n, m), "%d origins, max_hits %d, the STATS instantiation" % (K, m))
            tests[m] = st["tests"], st["candidates"]
    finally:
        mirt.set_profiling(False)
    assert tests[8][0] >= tests[1][0] and tests[8][1] >= tests[1][1], tests
    got = call("device", origins[0] if K == 1 else origins, of[:n], dirs[:n], 8, mode=BINNED)   # without profiling the counters stay zero
    assert got[2]["shadow_rays"] == 0 and got[2]["candidates"] == 0


# ---- 8: coarse and fine cubes, one shell and many: a process each -------------------------------------------------------------------------------

CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %r)
import mirt
z = np.load(sys.argv[1])
hits, counts = z["hits"].view(mirt.HIT_DTYPE).reshape(len(z["counts"]), -1), z["counts"]
mirt.init(0)
mirt.scene_upload(z["tris"])
mirt.set_query_mode(mirt.QUERY_BINNED)
for m in (1, 4, 8):
    h, c = mirt.intersect_ordered_fans(z["origins"], z["of"], z["dirs"], m)
    st = mirt.fan_stats()
    assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_bins"] == (int(sys.argv[2]) or st["cube_bins"]) and st["shells"] == (int(sys.argv[3]) or st["shells"]), st
    assert np.array_equal(c, np.minimum(counts, m)), m
    assert h.tobytes() == np.ascontiguousarray(hits[:, :m]).tobytes(), m
mirt.shutdown()
print("ok")
'''


@pytest.mark.parametrize("knob", [("MIRT_CUBE_BINS", 64), ("MIRT_CUBE_BINS", 256), ("MIRT_LIGHT_SHELLS", 1), ("MIRT_LIGHT_SHELLS", 16)], ids=lambda k: "%s=%d" % k)
def test_coarse_and_fine_cubes(oracle, tmp_path, knob):
    """MIRT_CUBE_BINS and MIRT_LIGHT_SHELLS are read once per process.  One shell means the list's end never moves; many exercise its
    moving in."""
    tris, origins, of, dirs, rays, want = F.case(oracle, "soup2000", 5, 2049)
    n = 513
    path = str(tmp_path / "case.npz")
    np.savez(path, tris=tris, origins=origins, of=of[:n], dirs=dirs[:n], hits=np.ascontiguousarray(want[0][:n]).view(np.uint8), counts=want[1][:n])
    # (what the knob sets is checked; the other figure -- 0 here -- follows from the library's own rules)
    bins = knob[1] if knob[0] == "MIRT_CUBE_BINS" else 0
    shells = knob[1] if knob[0] == "MIRT_LIGHT_SHELLS" else 0
    mirt.shutdown()
    try:
        r = subprocess.run([sys.executable, "-c", CHILD % os.path.join(ROOT, "cpp-raytracer-rasterizer_amd"), path, str(bins), str(shells)],
                           env=dict(os.environ, **{knob[0]: str(knob[1])}), capture_output=True, text=True, timeout=300)
    finally:
        mirt.init(0)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]


# ---- 9: between binned frames in flight -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_flight", [2, 4])
def test_device_form_between_binned_frames_in_flight(oracle, in_flight):
    tris, origins, of, dirs, rays, want = F.case(oracle, "soup2000", 5, 2049)
    one = F.case(oracle, "soup2000", 1, 2049)
    mirt.scene_upload(tris)
    W, H = 160, 120
    view = mirt.make_view((0, 0, -2.5), oracle.rot_from_yaw(0.1, 1.0), 120.0, W, H)
    light = LIGHTS[:1]
    want_frame = mirt.raytrace(view, light, mode=mirt.RT_BRUTE)["xrgb"]
    # (several origins, one origin) in turn, with ray counts on either side of a block
    calls = [(origins, of[:n], dirs[:n], F.prefix(want, n, m), m) if k % 2 == 0 else (one[1][0], None, one[3][:n], F.prefix(one[5], n, m), m)
             for k, (n, m) in enumerate(((1500, 4), (3, 8), (700, 1), (2049, 2), (64, 5), (257, 8)))]
    bufs = []
    mirt.set_query_mode(BINNED)
    try:
        mirt.set_frames_in_flight(in_flight)
        for o, idx, d, w, m in calls:
            n = len(d)
            held = [to_device(d), DeviceArray((n * m * REC,), np.uint8, 0xAA), DeviceArray((n,), np.int32, 0xAA), DeviceArray((H, W), np.uint32, 0)]
            if idx is not None:
                held.append(to_device(idx))
            bufs.append(held)
            mirt.raytrace_device(view, light, (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, held[3].ptr, W * 4)
            if idx is None:
                mirt.intersect_ordered_from_device(o, held[0].ptr, n, None, m, held[1].ptr, held[2].ptr)
            else:
                mirt.intersect_ordered_fans_device(o, held[4].ptr, held[0].ptr, n, None, m, held[1].ptr, held[2].ptr)
            assert mirt.fan_stats()["mode_used"] == BINNED
        mirt.sync()
        for i, (held, (o, idx, d, w, m)) in enumerate(zip(bufs, calls)):
            h = np.frombuffer(held[1].read().tobytes(), mirt.HIT_DTYPE).reshape(len(d), m)
            same((h, held[2].read()), w, "call %d of %d in flight" % (i, in_flight))
            assert np.array_equal(held[3].read()[1:-1, 1:-1], want_frame[1:-1, 1:-1]), "frame %d" % i
        # a standing view: every stream holds its pass by now; ordered calls between its frames leave the passes alone
        x = bufs[0][3]
        for i in range(2 * in_flight):
            assert hip_fill(x, 0x11)
            mirt.raytrace_device(view, light, (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, x.ptr, W * 4)
            st = mirt.stats()
            assert st["mode_used"] == mirt.RT_BINNED and st["bins_reused"] == 1, (i, st)
            assert np.array_equal(x.read()[1:-1, 1:-1], want_frame[1:-1, 1:-1]), "standing frame %d" % i
            held, (o, idx, d, w, m) = bufs[i % len(calls)], calls[i % len(calls)]
            assert hip_fill(held[1], 0xAA) and hip_fill(held[2], 0xAA)
            if idx is None:
                mirt.intersect_ordered_from_device(o, held[0].ptr, len(d), None, m, held[1].ptr, held[2].ptr)
            else:
                mirt.intersect_ordered_fans_device(o, held[4].ptr, held[0].ptr, len(d), None, m, held[1].ptr, held[2].ptr)
            h = np.frombuffer(held[1].read().tobytes(), mirt.HIT_DTYPE).reshape(len(d), m)
            same((h, held[2].read()), w, "standing call %d" % i)
            assert mirt.stats() == st
    finally:
        mirt.set_query_mode(AUTO)
        mirt.set_frames_in_flight(1)
        for held in bufs:
            for x in held:
                x.free()


# ---- 10: errors, and an empty call ----------------------------------------------------------------------------------------------------------------

def test_errors_and_an_empty_call():
    lib = mirt.load()
    mirt.scene_upload(mirt.scene_cornell())
    cases, keep, snapshot = F.bad_calls()
    before = snapshot()
    for name, args, why in cases:
        assert getattr(lib, name)(*args) == INVALID, (name, why)
        assert lib.mirt_last_error(), (name, why)
    P = mirt._ptr
    origin, origins, of, dirs, hits, counts = keep
    # an empty call succeeds and does nothing, NULL arrays and an empty origin list included
    assert lib.mirt_intersect_ordered_from(P(origin), None, 0, None, 1, None, None) == 0
    assert lib.mirt_intersect_ordered_from_device(None, None, 0, None, 8, None, None) == 0
    assert lib.mirt_intersect_ordered_fans(None, 0, None, None, 0, None, 2, None, None) == 0
    assert lib.mirt_intersect_ordered_fans_device(P(origins), 2, P(of), None, 0, None, 2, None, None) == 0
    assert snapshot() == before, "a refused or empty call wrote something"
    h, c = mirt.intersect_ordered_fans(origins, np.zeros(0, np.int32), np.zeros((0, 3), np.float32), 3)
    assert h.shape == (0, 3) and c.shape == (0,)
