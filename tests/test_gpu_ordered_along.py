"""Every hit along parallel rays, in order, on the GPU: mirt_intersect_ordered_along* (k_along_order) and
mirt_intersect_ordered_alongs* (k_alongs_order) through the grids across the directions, and by the sweep over the rays written out,
against the CPU oracle, byte for byte.

The expectation is ordered_helpers.peel / from_table on mirt.make_rays(starts, d) (ordered_along_helpers.case).  Every call goes
through buffers prefilled with 0xAA with guard records and guard counts behind them: each slot and count of the call is written, and
nothing beyond.  Starts: even rays inside the scene with along_helpers.plant_odd_starts' kinds among them, odd rays pulled back in
front of it (ordered_along_helpers.starts_of)."""
import numpy as np
import pytest

import mirt
import ordered_along_helpers as A
import ordered_helpers as O
import placement as pl
from along_helpers import OBLIQUE, SHELLS, directions, plant_odd_starts
from devbuf import DeviceArray, to_device
from query_helpers import INF, NAN, make_batch, scene_of

pytestmark = pytest.mark.gpu

INVALID = -3
BRUTE, BINNED, AUTO = mirt.QUERY_BRUTE, mirt.QUERY_BINNED, mirt.QUERY_AUTO
BOTH = (("brute", BRUTE), ("binned", BINNED))
REC = A.REC
call = A.ordered_along
same = A.same


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_query_mode(mirt.QUERY_AUTO)
    mirt.set_profiling(False)
    mirt.set_frames_in_flight(1)
    mirt.shutdown()


def mode_is(st, mode, what):
    if mode == BRUTE:
        assert st["mode_used"] == BRUTE and st["cube_source"] == 0 and st["cube_bins"] == 0, (what, st)
    else:
        assert st["mode_used"] == BINNED and st["cube_source"] in (1, 2) and st["cube_bins"] >= 8 and st["shells"] == SHELLS, (what, st)


# ---- 1: records, counts and trailing fresh slots; modes and forms ------------------------------------------------------------------------

@pytest.mark.parametrize("name", A.SCENES)
def test_records_equal_the_oracle(oracle, name):
    tris, starts, planted, back, want2 = A.case(oracle, name, OBLIQUE, 4097, 2)
    want8 = A.case(oracle, name, OBLIQUE, 257, 8)[4]
    assert A.case(oracle, name, OBLIQUE, 257, 8)[1].tobytes() == starts[:257].tobytes()
    A.floors_hold(name, want8, back, name + ", 257 rays")
    A.floors_hold(name, want2, back, name + ", 4097 rays")
    if name == "soup2000":
        full = np.flatnonzero(want8[1] == 8)
        assert O.peel(oracle, tris, mirt.make_rays(starts[full], OBLIQUE), 10)[1].max() > 8, "no ray has more than 8 hits"
    assert planted[:257].sum() >= 3
    mirt.scene_upload(tris)
    fresh = mirt.intersect_along(OBLIQUE, starts)
    cases = [(n, m) for n in (1, 63, 65, 257) for m in A.HITS] + [(4097, 2)]
    for n, m in cases:
        want = A.prefix(want8 if n <= 257 else want2, n, m)
        for form in ("host", "device") if n in (65, 4097) else ("host",):
            got = {}
            for mname, mode in (("brute", BRUTE), ("binned", BINNED), ("auto", AUTO)):
                what = "%s, %d rays, max_hits %d, %s form, %s" % (name, n, m, form, mname)
                got[mname] = call(form, OBLIQUE, starts[:n], m, mode=mode, what=what)
                st = got[mname][2]
                if mode == AUTO:                                     # (the grid of the BINNED call in front is held: AUTO takes it)
                    assert st["mode_used"] == BINNED and st["cube_source"] == 2, (what, st)
                else:
                    mode_is(st, mode, what)
                same(got[mname], want, what + " vs the oracle")
            same(got["binned"], got["brute"], "%s, %d rays, max_hits %d: BINNED vs BRUTE" % (name, n, m))
            # slot 0 is mirt_intersect_along on a fresh record
            h, c = got["binned"][:2]
            hit = c > 0
            assert np.array_equal(hit, fresh["index"][:n] >= 0), what
            assert h[:, 0][hit].tobytes() == fresh[:n][hit].tobytes(), what + ": slot 0 is not mirt_intersect_along's record"
            assert h[:, 0][~hit].tobytes() == mirt.fresh_hits(int((~hit).sum())).tobytes(), what
    # a fresh upload, a small AUTO call: nothing is held, the sweep answers
    mirt.scene_upload(tris)
    got = call("device", OBLIQUE, starts[:65], 4, mode=AUTO)
    mode_is(got[2], BRUTE, name + ", AUTO with nothing held")
    same(got, A.prefix(want8, 65, 4), name + ", AUTO with nothing held")


def test_the_wrappers_return_the_same(oracle):
    tris, starts, planted, back, want8 = A.case(oracle, "soup2000", OBLIQUE, 257, 8)
    mirt.scene_upload(tris)
    mirt.set_query_mode(BINNED)
    try:
        hits, counts = mirt.intersect_ordered_along(OBLIQUE, starts, 4)
        assert hits.shape == (257, 4) and counts.shape == (257,)
        same((hits, counts), A.prefix(want8, 257, 4), "mirt.intersect_ordered_along")
        hits, counts = mirt.intersect_ordered_alongs([OBLIQUE], None, starts, 3)
        same((hits, counts), A.prefix(want8, 257, 3), "mirt.intersect_ordered_alongs, one direction, no indices")
        assert mirt.intersect_ordered_along(OBLIQUE, starts[:0], 4)[0].shape == (0, 4)
    finally:
        mirt.set_query_mode(AUTO)


# ---- 2: directions ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["soup2000", "cornell"])
def test_directions(oracle, name):
    """The 26 axis, diagonal and corner directions, the oblique one and the two ends of the magnitude window, 65 starts each."""
    dirs = directions()
    assert len(dirs) == 29
    mirt.scene_upload(O.scene(name))
    hit_twice = 0
    for k, d in enumerate(dirs):
        tris, starts, planted, back, want = A.case(oracle, name, d, 65, 4)
        hit_twice += int((want[1] >= 2).sum())
        what = "%s, direction %r" % (name, d.tolist())
        got = call("device", d, starts, 4, mode=BINNED, what=what)
        if k >= 27:
            mode_is(got[2], BINNED, what)                            # magnitudes 2^-30 and 2^18 stay binned
        else:
            assert got[2]["mode_used"] in (BRUTE, BINNED), (what, got[2])   # (an edge-on scene may give the grid up)
        same(got, want, what)
    assert hit_twice > 29 * 65 // 10


def test_a_direction_outside_the_window_is_the_sweep(oracle):
    name = "soup65x2"
    mirt.scene_upload(O.scene(name))
    for d in (np.array([0, 0, 2.0 ** 20], np.float32), np.array([2.0 ** -40, 0, 0], np.float32), np.array([0, 0, 0], np.float32), np.array([1, NAN, 0], np.float32)):
        tris, starts, planted, back, want = A.case(oracle, name, d, 65, 4)
        got = call("device", d, starts, 4, mode=BINNED, what=repr(d))
        assert got[2]["mode_used"] == BRUTE and got[2]["cube_source"] == 0, (d, got[2])
        same(got, want, repr(d))
    assert A.case(oracle, name, np.array([0, 0, 2.0 ** 20], np.float32), 65, 4)[4][1].sum() > 20


# ---- 3: an edge-on scene: the every-ray list at work -------------------------------------------------------------------------------------

def edge_on_case(axis):
    """test_gpu_along.py's edge-on scenes and starts: (d, tris, starts) for dir in the planes of Cornell's walls, exactly and one ulp
    either way."""
    from test_gpu_along import edge_on_scene
    base = np.zeros(3, np.float32)
    base[axis] = -1.0
    tilted = []
    for c in ((axis + 1) % 3, (axis + 2) % 3):
        for to in (INF, -INF):
            e = base.copy()
            e[c] = np.nextafter(np.float32(0), to)
            tilted.append(e)
    up = base.copy()
    up[axis] = np.nextafter(np.float32(-1), np.float32(0))
    rng = np.random.default_rng(29)
    for d in [base] + tilted + [up]:
        tris = edge_on_scene(d)
        starts = rng.uniform(-0.99, 0.99, (320, 3)).astype(np.float32)
        for k in range(0, 160):
            starts[k][(axis + 1 + k % 2) % 3] = (1.0, -1.0)[(k // 2) % 2]
        on_tri = tris[-8:, 0:3] + 0.3 * (tris[-8:, 3:6] - tris[-8:, 0:3]) + 0.2 * (tris[-8:, 6:9] - tris[-8:, 0:3])
        starts[160:168] = on_tri - 0.4 * d / np.float32(np.abs(d).max())
        yield d, tris, starts


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_edge_on_scene(oracle, axis):
    """max_hits 8: BINNED equals BRUTE equals the oracle, and some ray's answer holds a triangle of the every-ray list: one whose
    plane lies within 2^-20 rad of dir is filed there whatever else (along.hpp: |den| below 64 m_d, and m_d is at least 2^-20 / 3 of
    |e1 x e2| |d'|)."""
    for d, tris, starts in edge_on_case(axis):
        mirt.scene_upload(tris)
        want = O.peel(oracle, tris, mirt.make_rays(starts, d), 8)
        v = tris[:, :9].reshape(-1, 3, 3).astype(np.float64)
        normal = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        normal /= np.linalg.norm(normal, axis=1)[:, None]
        on_list = np.flatnonzero(np.abs(normal @ (d.astype(np.float64) / np.linalg.norm(d.astype(np.float64)))) < 2.0 ** -20)
        assert len(on_list) >= 8 and np.isin(want[0]["index"], on_list).any(), "no answer holds a triangle of the every-ray list"
        what = "edge-on, %r" % d.tolist()
        brute = call("device", d, starts, 8, mode=BRUTE, what=what)
        binned = call("device", d, starts, 8, mode=BINNED, what=what)
        assert binned[2]["mode_used"] == BINNED, binned[2]           # (38 triangles: the every-ray list never outgrows its floor of 64)
        same(brute, want, what + ", brute")
        same(binned, want, what + ", binned")


# ---- 4: continuation -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mname,mode", BOTH)
@pytest.mark.parametrize("name", ("soup2000", "soup65x2"))
def test_continuation_enumerates_every_hit(oracle, name, mname, mode):
    tris, starts, planted, back, (wh, wc) = A.case(oracle, name, OBLIQUE, 64, 40)
    assert wc.max() < 40
    if name == "soup2000":
        assert wc.max() > 4, "no ray needs a third round"
    else:
        assert ((wh["distance"][:, 1:] == wh["distance"][:, :-1]) & (wh["index"][:, 1:] >= 0)).sum() > 20, "no ties"
    mirt.scene_upload(tris)
    # max_hits = 2, again and again behind each ray's last record
    parts, after = [], None
    for rnd in range(25):
        what = "%s, %s, round %d" % (name, mname, rnd)
        hits, counts, st = call("host" if rnd % 2 == 0 else "device", OBLIQUE, starts, 2, after=after, mode=mode, what=what)
        mode_is(st, mode, what)
        parts.append(hits)
        if (counts < 2).all():
            break
        after = A.last_records(hits, counts, 2)
    else:
        raise AssertionError("the enumeration does not end")
    got = np.concatenate(parts, axis=1)
    assert got.shape[1] >= wc.max()
    width = max(got.shape[1], wh.shape[1])
    pad = lambda h: np.concatenate([h, np.broadcast_to(mirt.fresh_hits(1)[0], (len(h), width - h.shape[1]))], axis=1)
    assert pad(got).tobytes() == pad(wh).tobytes(), "%s, %s: the concatenated rounds differ from the oracle's enumeration" % (name, mname)
    # the in-place peel: max_hits == 1, after == hits; started behind distance -1, which admits everything
    n = len(starts)
    mirt.set_query_mode(mode)
    try:
        start = mirt.fresh_hits(n)
        start["distance"] = -1.0
        s32 = np.ascontiguousarray(starts, np.float32)
        d32 = np.ascontiguousarray(OBLIQUE, np.float32)
        d_starts, d_rec = to_device(s32), to_device(start)
        host_rec = start.copy()
        cnt = np.zeros(n, np.int32)
        P = mirt._ptr
        try:
            with DeviceArray((n,), np.int32, 0xAA) as d_cnt:
                for k in range(int(wc.max()) + 1):
                    mirt.intersect_ordered_along_device(OBLIQUE, d_starts.ptr, n, d_rec.ptr, 1, d_rec.ptr, d_cnt.ptr)
                    mirt.sync()
                    rec = np.frombuffer(d_rec.read().tobytes(), mirt.HIT_DTYPE)
                    assert rec.tobytes() == np.ascontiguousarray(wh[:, k]).tobytes(), "%s, %s: in-place peel, device form, step %d" % (name, mname, k)
                    assert np.array_equal(d_cnt.read(), (wc > k).astype(np.int32))
                    mirt._check(mirt.load().mirt_intersect_ordered_along(P(d32), P(s32), n, P(host_rec), 1, P(host_rec), P(cnt)))
                    assert host_rec.tobytes() == rec.tobytes() and np.array_equal(cnt, (wc > k).astype(np.int32)), "%s, %s: in-place peel, host form, step %d" % (name, mname, k)
        finally:
            d_starts.free(); d_rec.free()
    finally:
        mirt.set_query_mode(AUTO)


@pytest.mark.parametrize("name,n", (("soup2000", 32), ("soup65x2", 257), ("cornell", 257)))
def test_after_records(oracle, name, n):
    """`after` records of every kind of ordered_helpers.after_records, against the per-triangle table sorted as the contract words it."""
    tris, starts, planted, back, want8 = A.case(oracle, name, OBLIQUE, 257, 8)
    starts = starts[:n]
    rays = mirt.make_rays(starts, OBLIQUE)
    key = ("table", name, n)
    if key not in A._cache:
        A._cache[key] = O.table(oracle, tris, rays)
        A._cache[key].setflags(write=False)
    rec = A._cache[key]
    same(O.from_table(rec, None, 8), A.prefix(want8, n, 8), name + ": table vs peel")
    mirt.scene_upload(tris)
    slot0 = O.from_table(rec, None, 1)[0][:, 0]
    for shift in (0, 4, 8):                                         # (every ray meets three of the kinds)
        after, kind = O.after_records(slot0, shift)
        for m in (1, 3, 8):
            want = O.from_table(rec, after, m)
            for mname, mode in BOTH:
                what = "%s, after kinds from %d on, max_hits %d, %s" % (name, shift, m, mname)
                got = call("host" if m == 3 else "device", OBLIQUE, starts, m, after=after, mode=mode, what=what)
                mode_is(got[2], mode, what)
                same(got, want, what)
        c = O.from_table(rec, after, 3)[1]
        assert np.array_equal(c[kind == 0], O.from_table(rec, None, 3)[1][kind == 0])
        assert c[kind == 0].sum() > 0 and c[kind >= 8].sum() == 0, "the kinds do not admit what they should"


# ---- 5: several directions in one call --------------------------------------------------------------------------------------------------------

def direction_list(K):
    """K directions out of along_helpers.directions(), each later round of 29 scaled by another dyadic factor; from K = 3 on the last
    one repeats the first bit for bit (test_gpu_alongs.py: direction_list)."""
    base = directions()
    out = [(base[k % len(base)] * np.float32(1.0 + 0.25 * (k // len(base)))).astype(np.float32) for k in range(K)]
    if K >= 3:
        out[-1] = out[0].copy()
    return np.ascontiguousarray(out, np.float32)


def several(oracle, name, K, n, cap):
    """(tris, dirs, of, starts, want): K directions dealt to n starts in random order; the starts are pulled back along THEIR direction."""
    key = ("several", name, K, n, cap)
    if key not in A._cache:
        tris = O.scene(name)
        dirs = direction_list(K)
        of = np.random.default_rng(31 + K).permutation(np.arange(n) % K).astype(np.int32)
        B = make_batch(n, 1.5, 1.0)["start"]
        starts, _ = plant_odd_starts(B, A.extent_of(tris))
        dh = dirs[of].astype(np.float64)
        dh /= np.linalg.norm(dh, axis=1)[:, None]
        odd = np.arange(n) % 2 == 1
        starts[odd] = (B[odd].astype(np.float64) / 1.5 - 3.0 * dh[odd]).astype(np.float32)
        want = O.peel(oracle, tris, mirt.make_rays(starts, dirs[of]), cap)
        for x in (dirs, of, starts) + want:
            x.setflags(write=False)
        A._cache[key] = tris, dirs, of, starts, want
    return A._cache[key]


@pytest.mark.parametrize("K", [1, 3, 33, 70])
def test_several_directions(oracle, K):
    """1, 3, 33 and 70 directions -- one, one, two and three passes of 32 --, dir_of in random order, 257 rays, max_hits 4."""
    tris, dirs, of, starts, want = several(oracle, "soup2000", K, 257, 4)
    assert (want[1] >= 2).mean() > 0.2
    mirt.scene_upload(tris)
    for mname, mode in BOTH:
        for form in ("host", "device"):
            what = "%d directions, %s, %s form" % (K, mname, form)
            got = call(form, dirs, starts, 4, mode=mode, what=what, dir_of=of)
            mode_is(got[2], mode, what)
            same(got, want, what)
    if K == 1:
        got = call("device", dirs, starts, 4, mode=BINNED, dir_of=None)
        same(got, want, "one direction, no indices")
    else:
        # continuing behind the first two, and peeling in place over the passes
        after = A.last_records(*A.prefix(want, 257, 2), 2)
        got = call("device", dirs, starts, 2, after=after, mode=BINNED, dir_of=of)
        full = want[1] >= 2
        assert got[0][full].tobytes() == np.ascontiguousarray(want[0][:, 2:4][full]).tobytes(), "%d directions: continuation" % K
        assert not got[1][~full].any()
        n = len(starts)
        start = mirt.fresh_hits(n)
        start["distance"] = -1.0
        mirt.set_query_mode(BINNED)
        d_starts, d_of, d_rec = to_device(np.ascontiguousarray(starts)), to_device(np.ascontiguousarray(of)), to_device(start)
        try:
            with DeviceArray((n,), np.int32, 0xAA) as d_cnt:
                for k in range(3):
                    mirt.intersect_ordered_alongs_device(dirs, d_of.ptr, d_starts.ptr, n, d_rec.ptr, 1, d_rec.ptr, d_cnt.ptr)
                    mirt.sync()
                    rec = np.frombuffer(d_rec.read().tobytes(), mirt.HIT_DTYPE)
                    assert rec.tobytes() == np.ascontiguousarray(want[0][:, k]).tobytes(), "%d directions: in-place peel, step %d" % (K, k)
                    assert np.array_equal(d_cnt.read(), (want[1] > k).astype(np.int32))
        finally:
            mirt.set_query_mode(AUTO)
            d_starts.free(); d_of.free(); d_rec.free()


@pytest.mark.parametrize("K", [16, 17])
def test_a_grid_of_256_cells_a_side(K):
    """33 000 triangles: B = 256, a group holds 15 directions -- two passes.  64 rays per direction; BINNED against
    mirt_intersect_ordered_device on the same rays written out (that sweep is pinned to the oracle by test_gpu_ordered_hits.py)."""
    tris = pl.unit_scene("soup33000")
    mirt.scene_upload(tris)
    n = 64 * K
    dirs = direction_list(K)
    of = np.random.default_rng(37).permutation(np.arange(n) % K).astype(np.int32)
    B = make_batch(n, 1.5, 1.0)["start"]
    dh = dirs[of].astype(np.float64)
    dh /= np.linalg.norm(dh, axis=1)[:, None]
    starts = np.where((np.arange(n) % 2 == 1)[:, None], B.astype(np.float64) / 1.5 - 3.0 * dh, B).astype(np.float32)
    rays = np.ascontiguousarray(mirt.make_rays(starts, dirs[of]))
    d_rays = to_device(rays)
    try:
        with DeviceArray((n * 4 * REC,), np.uint8, 0xAA) as d_hits, DeviceArray((n,), np.int32, 0xAA) as d_counts:
            mirt.intersect_ordered_device(d_rays.ptr, n, None, 4, d_hits.ptr, d_counts.ptr)
            mirt.sync()
            want = np.frombuffer(d_hits.read().tobytes(), mirt.HIT_DTYPE).reshape(n, 4).copy(), d_counts.read().copy()
    finally:
        d_rays.free()
    assert (want[1] >= 2).mean() > 0.2 and (want[1] == 4).any()
    got = call("device", dirs, starts, 4, mode=BINNED, dir_of=of, what="%d directions on 33 000 triangles" % K)
    assert got[2]["mode_used"] == BINNED and got[2]["cube_bins"] == 256, got[2]
    same(got, want, "%d directions on 33 000 triangles" % K)


@pytest.mark.parametrize("K", [5, 33])
def test_indices_outside_the_list(oracle, K):
    """-1 and ndirs: the device form leaves the ray's slots as they were and writes its count 0, under both modes, its neighbours
    right; the host form refuses with nothing written."""
    tris, dirs, of, starts, want = several(oracle, "soup2000", K, 257, 4)
    mirt.scene_upload(tris)
    n = len(starts)
    idx = of.copy()
    stray = np.zeros(n, bool)
    for j, bad in enumerate((-1, K)):
        idx[3 + j::37] = bad
        stray[3 + j::37] = True
    exp_h, exp_c = want[0].copy(), want[1].copy()
    exp_c[stray] = 0
    for mname, mode in BOTH:
        for m in (4, 1):
            what = "%d directions, stray indices, %s, max_hits %d" % (K, mname, m)
            got = call("device", dirs, starts, m, mode=mode, what=what, dir_of=idx, stray=stray)      # (asserts the strays' slots are still 0xAA)
            mode_is(got[2], mode, what)
            wh, wc = A.prefix((exp_h, exp_c), n, m)
            assert np.array_equal(got[1], wc), what
            assert got[0][~stray].tobytes() == wh[~stray].tobytes(), what
    lib = mirt.load()
    P = mirt._ptr
    hbuf = np.frombuffer(np.full(n * 4 * REC, 0xAA, np.uint8).tobytes(), mirt.HIT_DTYPE).copy()
    cbuf = np.full(n, -1431655766, np.int32)
    s32 = np.ascontiguousarray(starts, np.float32)
    assert lib.mirt_intersect_ordered_alongs(P(dirs), K, P(idx), P(s32), n, None, 4, P(hbuf), P(cbuf)) == INVALID
    assert (hbuf.view(np.uint8) == 0xAA).all() and (cbuf == -1431655766).all()
    with pytest.raises(mirt.MirtError, match=r"dir_of\[3\] = -1 is outside \[0, %d\)" % K):
        mirt.intersect_ordered_alongs(dirs, idx, starts, 4)


# ---- 6: keeping and sharing the structure -------------------------------------------------------------------------------------------------------

def test_keeping_and_sharing(oracle):
    tris, starts, planted, back, want8 = A.case(oracle, "soup2000", OBLIQUE, 257, 8)
    want = A.prefix(want8, 257, 4)
    mirt.scene_upload(tris)                                         # (a new scene version: nothing is held)
    got = call("device", OBLIQUE, starts, 4, mode=BINNED)
    assert got[2]["cube_source"] == 1 and got[2]["cube_bins"] == 32, got[2]
    same(got, want, "built")
    got = call("host", OBLIQUE, starts, 4, mode=BINNED)
    assert got[2]["cube_source"] == 2, got[2]
    same(got, want, "kept")
    # one structure serves both families, either way round
    mirt.scene_upload(tris)
    mirt.set_query_mode(BINNED)
    try:
        mirt.intersect_along(OBLIQUE, starts)
        assert mirt.along_stats()["cube_source"] == 1
    finally:
        mirt.set_query_mode(AUTO)
    got = call("device", OBLIQUE, starts, 4, mode=BINNED)
    assert got[2]["cube_source"] == 2, got[2]
    same(got, want, "the grid mirt_intersect_along built")
    mirt.scene_upload(tris)
    call("device", OBLIQUE, starts, 4, mode=BINNED)
    mirt.set_query_mode(BINNED)
    try:
        mirt.intersect_along(OBLIQUE, starts)
        assert mirt.along_stats()["cube_source"] == 2
    finally:
        mirt.set_query_mode(AUTO)
    # the scene moves
    rot = np.array([0, 1, 0, -1, 0, 0, 0, 0, 1], np.float32)
    shift = np.array([0.25, -0.125, 0.0625], np.float32)
    mirt.scene_transform(0, len(tris), rot, shift)
    moved = O.peel(oracle, mirt.scene_download(), mirt.make_rays(starts, OBLIQUE), 4)
    got = call("device", OBLIQUE, starts, 4, mode=BINNED)
    assert got[2]["cube_source"] == 1 and got[2]["mode_used"] == BINNED, got[2]
    same(got, moved, "after mirt_scene_transform")
    assert moved[0].tobytes() != want[0].tobytes() and (moved[1] > 0).mean() > 0.2
    # four device calls on two streams right after an upload: the first one builds
    n = len(starts)
    mirt.set_frames_in_flight(2)
    mirt.set_query_mode(BINNED)
    d_starts = to_device(np.ascontiguousarray(starts))
    outs = [(DeviceArray((n * 4 * REC,), np.uint8, 0xAA), DeviceArray((n,), np.int32, 0xAA)) for _ in range(4)]
    try:
        mirt.scene_upload(tris)
        for h, c in outs:
            mirt.intersect_ordered_along_device(OBLIQUE, d_starts.ptr, n, None, 4, h.ptr, c.ptr)
        mirt.sync()
        for k, (h, c) in enumerate(outs):
            same((np.frombuffer(h.read().tobytes(), mirt.HIT_DTYPE).reshape(n, 4), c.read()), want, "call %d of 4 on two streams" % k)
    finally:
        mirt.set_query_mode(AUTO)
        mirt.set_frames_in_flight(1)
        d_starts.free()
        for h, c in outs:
            h.free(); c.free()


@pytest.mark.parametrize("pname,cls", [("40_-25_60_div1024", "gave_up"), ("0_0_4096", "no_grid")])
def test_placements_the_grid_does_not_serve(oracle, pname, cls):
    """One placement where the grid gives up and one where there is none: the sweep answers, equal to the oracle on the placed inputs."""
    assert pl.along_class("soup2000", pname, "oblique") == cls
    T, s = pl.PLACEMENTS[pname]
    tris = pl.placed_scene("soup2000", pname)
    d = pl.place_dirs(OBLIQUE, s)
    unit = A.starts_of(pl.unit_scene("soup2000"), OBLIQUE, 65)[0]
    starts = pl.place(np.where(np.isfinite(unit) & (np.abs(unit) < 100), unit, 0.0), T, s)
    want = O.peel(oracle, tris, mirt.make_rays(starts, d), 4)
    assert (want[1] >= 1).mean() > 0.3
    mirt.scene_upload(tris)
    for form in ("host", "device"):
        got = call(form, d, starts, 4, mode=BINNED, what=pname)
        mode_is(got[2], BRUTE, pname)
        same(got, want, "%s, %s form" % (pname, form))
    dirs = np.ascontiguousarray([d, pl.place_dirs(pl.ALONG_DIRS["xy"], s)], np.float32)
    of = (np.arange(65) % 2).astype(np.int32)
    want2 = O.peel(oracle, tris, mirt.make_rays(starts, dirs[of]), 4)
    got = call("device", dirs, starts, 4, mode=BINNED, dir_of=of, what=pname)
    mode_is(got[2], BRUTE, pname + ", two directions")
    same(got, want2, pname + ", two directions")


# ---- 7: rows offered -----------------------------------------------------------------------------------------------------------------------------

def test_rows_offered():
    """With profiling on, on soup2000 in BINNED mode, test_gpu_along.py: test_rows_offered's inputs: candidates <= rays * n // 8 for
    max_hits 1 (tests/test_along_host.py shows that the inputs leave the bound room), non-decreasing over max_hits 1, 2, 4, 8, and
    the planted starts, no others, sweep."""
    tris, a, b = scene_of("soup2000")
    starts, planted = plant_odd_starts(make_batch(4097 + 300, a, b)["start"], A.extent_of(tris))
    n, rays = len(tris), len(starts)
    mirt.scene_upload(tris)
    mirt.set_profiling(True)
    try:
        offered = []
        for m in (1, 2, 4, 8):
            st = call("device", OBLIQUE, starts, m, mode=BINNED)[2]
            print(m, st)
            assert st["mode_used"] == BINNED and st["shadow_rays"] == rays, st
            assert st["fallback_records"] == int(planted.sum()) > 50, (st, int(planted.sum()))
            assert 0 < st["tests"] <= st["candidates"], st
            assert st["candidates"] >= int(planted.sum()) * n          # the sweeps count every row
            offered.append(st["candidates"])
        assert offered[0] <= rays * n // 8, offered
        assert offered == sorted(offered), offered
    finally:
        mirt.set_profiling(False)
    st = call("device", OBLIQUE, starts, 4, mode=BINNED)[2]
    assert st["mode_used"] == BINNED and st["shadow_rays"] == st["candidates"] == st["tests"] == st["fallback_records"] == 0, st


# ---- 8: errors and the empty call ---------------------------------------------------------------------------------------------------------------

def test_errors_and_an_empty_call():
    mirt.scene_upload(mirt.scene_cornell())
    lib = mirt.load()
    cases, keep, snapshot = A.bad_calls()
    before = snapshot()
    for name, args, why in cases:
        fn = getattr(lib, name)
        assert fn(*args) == INVALID, (name, why)
        assert lib.mirt_last_error(), (name, why)
        with pytest.raises(mirt.MirtError):
            mirt._check(fn(*args))
    P = mirt._ptr
    d, dirs, of, origins, hits, counts = keep
    for name in A.NAMES:
        fn = getattr(lib, name)
        if "alongs" in name:
            assert fn(P(dirs), 2, P(of), P(origins), 0, None, 2, P(hits), P(counts)) == 0
            assert fn(None, 0, None, None, 0, None, 8, None, None) == 0
        else:
            assert fn(P(d), P(origins), 0, None, 2, P(hits), P(counts)) == 0
            assert fn(None, None, 0, None, 8, None, None) == 0
    assert snapshot() == before, "a refused or empty call wrote something"


def test_no_scene():
    mirt.shutdown()
    mirt.init(0)
    with pytest.raises(mirt.MirtError, match="no scene uploaded"):
        mirt.intersect_ordered_along([0, 0, 1], np.zeros((2, 3), np.float32), 2)
    with pytest.raises(mirt.MirtError, match="no scene uploaded"):
        mirt.intersect_ordered_alongs([[0, 0, 1], [0, 1, 0]], [0, 1], np.zeros((2, 3), np.float32), 2)
