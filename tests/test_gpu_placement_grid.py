"""The arbitrary-ray grid and the ordered hits on scenes placed away from the world origin (tests/placement.py, placed_grid.py):
mirt_intersect* / mirt_occluded* under mirt_set_ray_grid, mirt_intersect_ordered* by sweep and through that grid, and
mirt_intersect_ordered_along(s)* through the along grids -- on soup2000 and on the tie scene soup2000+dup, host and device forms.

The contract is test_gpu_placement.py's: everything is compared byte for byte with the CPU oracle ON THE PLACED float32 INPUTS, there
is no tolerance, and no placed result is compared with a unit one.  Beside equality: where placement.RAY_GRID / ALONG_CLASS say
binned the statistics say so -- the structure built by the first call after the scene arrived and kept from then on, the ray grid's
plane-index pairs and every-ray rows those of tests/cpp/ray_grid_test.cpp (the same header functions count them on both sides) --;
where the structure gives up or is refused the sweep answers with the same bytes; the unfit rays and no others sweep; and no call
touches another family's statistics.  What the oracle's answers have to show for all this to mean something -- hit shares, full
lists, ties at the cuts, phantom acceptances -- is checked without a GPU by test_placement_host.py.

What fails here: a ray-grid walk that drops plane-index pairs (test_ray_grid and test_ordered at every binned placement: the phantom
rays' records), a structure kept over a move (test_in_place).  What cannot: a non-strict `near` reject in the ordered-along walk --
the structure lowers `near` by 2 sigma, far more than an ulp of the threshold, so a row at the threshold of a full list is never
eligible; tests/cpp/along_order_test.cpp's far regime pins that rule on the CPU.

test_in_place reaches the far placement and (10, -7, 5) from the unit upload by mirt_scene_transform and by mirt_scene_set_objects +
mirt_scene_pose with the unit scene's ray grid and an along grid held: a structure kept over the move would answer for the old
triangles."""
import numpy as np
import pytest

import mirt
import ordered_along_helpers as A
import ordered_helpers as O
import placed_grid as pg
import placement as pl
import query_helpers as rq
from along_helpers import SHELLS
from devbuf import DeviceArray, to_device
from placed_grid import HITS, KINDS, NSMALL, SCENES, TIE_SCENE, prefix
from test_gpu_along import closest as along_closest
from test_gpu_alongs import closest as alongs_closest
from test_gpu_ordered_hits import ordered, same
from test_gpu_placement import EYE, QUERY_SCENE, auto_stats, brute_stats, built_then_kept, mode, note, only, same_bytes, upload
from test_gpu_ray_grid import intersect, occluded

pytestmark = pytest.mark.gpu

BRUTE, BINNED, AUTO = mirt.QUERY_BRUTE, mirt.QUERY_BINNED, mirt.QUERY_AUTO
PEEL_STEPS = 48                                  # more than any ray of these sets has hits (asserted)
_cases = {}
TOOK = {"ray grid": {}, "along": {}}             # what the runs took, by placement: test_every_class_is_met


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_query_mode(AUTO)
    mirt.set_ray_grid(False)
    mirt.set_profiling(False)
    mirt.set_frames_in_flight(1)
    mirt.shutdown()


def case_of(oracle, pname):
    if pname not in _cases:
        _cases[pname] = pg.PlacedGrid(oracle, pname)
    return _cases[pname]


# ---- the ray grid's statistics ---------------------------------------------------------------------------------------------------------------

def grid_stats_are(st, scene, pname, first, what):
    """mirt_get_ray_grid_stats after a call under the switch, against placement.RAY_GRID; first: the first call since the scene arrived
    (None: either)."""
    cls, plane_pairs, every_rows = pl.RAY_GRID[scene][pname]
    source = (1, 2) if first is None else ((1,) if first else (2,))
    if cls == "binned":
        assert st["mode_used"] == BINNED and st["gave_up"] == 0 and st["source"] in source, (what, st)
        assert st["cells"] == pl.RAY_GRID_CELLS[scene] and st["plane_bins"] == 64 and st["offset_bins"] == 64, (what, st)
        # grid_tri_plane_keys and GRID_EVERY are counted alike by k_grid_pairs and by the CPU program: the same figures
        assert st["plane_pairs"] == plane_pairs and st["every_rows"] == every_rows and st["pairs"] > plane_pairs + every_rows, (what, st)
    elif cls == "gave_up":
        assert st["mode_used"] == BRUTE and st["gave_up"] == 1 and st["source"] in source and st["pairs"] == 0, (what, st)
    else:
        assert st["mode_used"] == BRUTE and st["gave_up"] == 0 and st["source"] == 0, (what, st)
    return cls


def run_ray_grid(case, scene, arrive=upload):
    tris, g = case.tris(scene), case.grid_rays(scene)
    rays, n = g["rays"], len(g["rays"])
    arrive(scene, tris, lambda: intersect(True, "host", rays[:NSMALL], mirt.fresh_hits(NSMALL)))
    calls = 0
    for kind in KINDS:
        incoming, want = case.grid_records(scene, kind)
        for m in (NSMALL, n):
            for form in ("host", "device"):
                what = "%s: ray grid on %s, %s records, %d rays, %s form" % (case.pname, scene, kind, m, form)
                with only(None, "mirt_intersect under the ray grid"):
                    with np.errstate(all="ignore"):
                        got = intersect(True, form, rays[:m], incoming[:m])
                cls = grid_stats_are(mirt.ray_grid_stats(), scene, case.pname, calls == 0, what)
                calls += 1
                rq.same_hits(got, want[:m], what + " vs the oracle")
                if m == NSMALL or form == "host":
                    rq.same_hits(got, intersect(False, form, rays[:m], incoming[:m]), what + " vs the switch off")
    limits, want_lim, want_null = case.grid_limits(scene)
    for lim, want in ((limits, want_lim), (None, want_null)):
        for m in (NSMALL, n):
            for form in ("host", "device"):
                what = "%s: ray grid on %s, occluded, %d rays, %s form, %s" % (case.pname, scene, m, form, "limits" if lim is not None else "NULL limits")
                ln = None if lim is None else np.ascontiguousarray(lim[:m])
                with only("occlusion", "mirt_occluded under the ray grid"):
                    got = occluded(True, form, rays[:m], ln, what)
                grid_stats_are(mirt.ray_grid_stats(), scene, case.pname, False, what)
                same_bytes(got, want[:m], what + " vs the oracle")
                if m == NSMALL:
                    same_bytes(got, occluded(False, form, rays[:m], ln, what), what + " vs the switch off")
    swept = ""
    if cls == "binned":
        # the unfit rays, and no others, sweep
        mirt.set_profiling(True)
        try:
            intersect(True, "host", rays, mirt.fresh_hits(n))
            st = mirt.ray_grid_stats()
            assert st["rays"] == n and st["swept_rays"] == int(g["unfit"].sum()) > 20, (case.pname, scene, st, int(g["unfit"].sum()))
            occluded(True, "device", rays, None, "profiling")
            st = mirt.ray_grid_stats()
            assert st["rays"] == n and st["swept_rays"] == int(g["unfit"].sum()), (case.pname, scene, st)
            offered = st["rows_cells"] + st["rows_planes"] + st["rows_every"]
            swept = "; %d of %d rays swept; rows offered to the others %.3f of the scene" % (st["swept_rays"], n, offered / ((n - st["swept_rays"]) * len(tris)))
        finally:
            mirt.set_profiling(False)
    TOOK["ray grid"].setdefault(case.pname, set()).add(cls)
    st = mirt.ray_grid_stats()
    note(case, "ray grid, %s" % scene, "%s: %s%s" % (cls, "built, kept; %d plane pairs, %d every-ray rows" % (st["plane_pairs"], st["every_rows"]) if cls == "binned"
                                                      else "the sweep answered", swept))


# ---- ordered hits of arbitrary rays -----------------------------------------------------------------------------------------------------------

def full_enumeration(rec):
    want = O.from_table(rec, None, PEEL_STEPS)
    assert want[1].max() < PEEL_STEPS
    return want


def run_ordered(case, scene, arrive=upload):
    tris, g = case.tris(scene), case.grid_rays(scene)
    rays, n = g["rays"], len(g["rays"])
    want8, rec = case.grid_ordered(scene), case.grid_table(scene)
    arrive(scene, tris, lambda: ordered("host", rays[:NSMALL], 1, grid=True))
    with np.errstate(all="ignore"):
        fresh = mirt.intersect(rays)
    first = True
    for grid in (True, False):
        for m in HITS:
            for nr, form in ((NSMALL, "host"), (NSMALL, "device"), (n, "device" if m == 3 else "host")):
                what = "%s: ordered hits on %s, %d rays, max_hits %d, %s form, switch %s" % (case.pname, scene, nr, m, form, "on" if grid else "off")
                with only(None, "mirt_intersect_ordered"):
                    got = ordered(form, rays[:nr], m, grid=grid, what=what)
                if grid:
                    grid_stats_are(mirt.ray_grid_stats(), scene, case.pname, first, what)
                    first = False
                same(got, prefix(want8, nr, m), what)
                # slot 0 is mirt_intersect on a fresh record
                hit = got[1] > 0
                assert np.array_equal(hit, fresh["index"][:nr] >= 0), what
                assert got[0][:, 0][hit].tobytes() == fresh[:nr][hit].tobytes(), what + ": slot 0 is not mirt_intersect's record"
        # `after` records of every kind, on the rays that have a table
        for k, (after, wants) in enumerate(case.after_cases(rec)):
            for m in HITS:
                form = "device" if m == 3 else "host"
                what = "%s: ordered hits on %s behind `after` records (rotation %d), max_hits %d, switch %s" % (case.pname, scene, k, m, "on" if grid else "off")
                same(ordered(form, rays[:NSMALL], m, after=after, grid=grid, what=what), wants[m], what)
        # the in-place peel: max_hits 1, after == hits, until nothing is left; together the steps are the oracle's table in order
        wh, wc = full_enumeration(rec)
        sub = np.ascontiguousarray(rays[:NSMALL])
        start = mirt.fresh_hits(NSMALL)
        start["distance"] = -1.0
        host_rec, cnt = start.copy(), np.zeros(NSMALL, np.int32)
        mirt.set_ray_grid(grid)
        d_rays, d_rec = to_device(sub), to_device(start)
        try:
            with DeviceArray((NSMALL,), np.int32, 0xAA) as d_cnt:
                for step in range(PEEL_STEPS):
                    what = "%s: ordered hits on %s, in-place peel, step %d, switch %s" % (case.pname, scene, step, "on" if grid else "off")
                    mirt.intersect_ordered_device(d_rays.ptr, NSMALL, d_rec.ptr, 1, d_rec.ptr, d_cnt.ptr)
                    got = np.frombuffer(d_rec.read().tobytes(), mirt.HIT_DTYPE)
                    assert got.tobytes() == np.ascontiguousarray(wh[:, step]).tobytes(), what + ", device form"
                    assert np.array_equal(d_cnt.read(), (wc > step).astype(np.int32)), what
                    mirt._check(mirt.load().mirt_intersect_ordered(mirt._ptr(sub), NSMALL, mirt._ptr(host_rec), 1, mirt._ptr(host_rec), mirt._ptr(cnt)))
                    assert host_rec.tobytes() == got.tobytes() and np.array_equal(cnt, (wc > step).astype(np.int32)), what + ", host form"
                    if not cnt.any():
                        break
                assert step == wc.max(), (step, wc.max())
        finally:
            mirt.set_ray_grid(False)
            d_rays.free(); d_rec.free()
    cls = pl.RAY_GRID_CLASS[scene][case.pname]
    TOOK["ray grid"].setdefault(case.pname, set()).add(cls)
    note(case, "ordered hits, %s" % scene, "by sweep, and under the switch %s; the peel took %d steps" % ("through the grid (binned)" if cls == "binned" else "by sweep again (%s)" % cls, step + 1))


# ---- ordered hits along parallel rays ----------------------------------------------------------------------------------------------------------

def run_ordered_along(case, scene, dname, arrive=upload, along_first=False):
    """One direction (dname) or the five of placement.ALONG_DIRS (dname None)."""
    several = dname is None
    a = case.ordered_alongs(scene) if several else case.ordered_along(scene, dname)
    d, of = (a["dirs"], a["of"]) if several else (a["d"], None)
    tris, starts, want, rec = case.tris(scene), a["starts"], a["want"], a["rec"]
    n, nt = len(starts), len(rec)
    cls = pl.alongs_class(scene, case.pname) if several else pl.along_class(scene, case.pname, dname)
    bins = pl.ALONG_BINS.get(scene, 32)
    what = "%s: ordered hits along %s on %s (%s)" % (case.pname, "five directions" if several else dname, scene, cls)
    assert a["planted"].sum() >= 3

    def call(form, m, md, after=None, count=n):
        with only("along", "an ordered-along call"):
            return A.ordered_along(form, d, starts[:count], m, after=after, mode=md, what=what, dir_of=None if of is None else of[:count])

    def closest():
        with only("along", "mirt_intersect_along(s)_device"):
            if several:
                return alongs_closest("device", d, of, starts, BINNED)
            return along_closest("device", d, starts, BINNED)

    def binned_stats(st, first, text):
        if cls == "binned":
            built_then_kept(st, first, text, bins)
            assert st["shells"] == SHELLS, (text, st)
        else:
            brute_stats(st, text)                                   # refused, or gave up: nothing is built, this time or the next

    def slot0_is(got, text):
        hit = want[1] > 0
        assert np.array_equal(got["index"] >= 0, hit) and got[hit].tobytes() == np.ascontiguousarray(want[0][:, 0])[hit].tobytes(), text

    arrive(scene, tris, lambda: call("host", 1, BINNED))
    built = 0
    if along_first:                                                  # the closest-hit call builds, the ordered calls find the grid held
        got, st = closest()
        binned_stats(st, True, what + ", mirt_intersect_along(s)_device first")
        slot0_is(got, what + ": mirt_intersect_along(s)_device")
        built = 1
    for form, m in (("device", 4), ("host", 1), ("host", 8), ("device", 1), ("host", 4), ("device", 8)):
        h, c, st = call(form, m, BINNED)
        binned_stats(st, built == 0, what + ", BINNED, max_hits %d, %s form" % (m, form))
        built += 1
        same((h, c), prefix(want, n, m), what + ", BINNED, max_hits %d, %s form" % (m, form))
    if not along_first:                                              # the other way round
        got, st = closest()
        binned_stats(st, False, what + ", mirt_intersect_along(s)_device behind the ordered calls")
        slot0_is(got, what + ": mirt_intersect_along(s)_device")
    for form, m in (("host", 1), ("device", 4), ("host", 8)):
        h, c, st = call(form, m, BRUTE)
        brute_stats(st, what + ", BRUTE")
        same((h, c), prefix(want, n, m), what + ", BRUTE, max_hits %d, %s form" % (m, form))
    h, c, st = call("device", 4, AUTO)
    took = auto_stats(st, what)
    assert cls == "binned" or took == "brute", (what, st)
    same((h, c), prefix(want, n, 4), what + ", AUTO")
    # `after` records of every kind, on the rays that have a table
    for k, (after, wants) in enumerate(case.after_cases(rec)):
        for m in HITS:
            for md, form in ((BINNED, "device" if m == 3 else "host"), (BRUTE, "host" if m == 3 else "device")):
                h, c, st = call(form, m, md, after=after, count=nt)
                if md == BINNED:
                    binned_stats(st, False, what + ", behind `after` records")
                same((h, c), wants[m], what + ", behind `after` records (rotation %d), max_hits %d, %s" % (k, m, "BINNED" if md == BINNED else "BRUTE"))
    # the in-place peel under BINNED in the device form and under BRUTE in the host form, until nothing is left
    wh, wc = full_enumeration(rec)
    s32 = np.ascontiguousarray(starts[:nt], np.float32)
    of32 = None if of is None else np.ascontiguousarray(of[:nt], np.int32)
    d32 = np.ascontiguousarray(d, np.float32)
    start = mirt.fresh_hits(nt)
    start["distance"] = -1.0
    host_rec, cnt = start.copy(), np.zeros(nt, np.int32)
    lib, P = mirt.load(), mirt._ptr
    held = [to_device(s32), to_device(start)] + ([to_device(of32)] if several else [])
    try:
        with DeviceArray((nt,), np.int32, 0xAA) as d_cnt:
            for step in range(PEEL_STEPS):
                text = "%s, in-place peel, step %d" % (what, step)
                with mode(BINNED):
                    if several:
                        mirt.intersect_ordered_alongs_device(d32, held[2].ptr, held[0].ptr, nt, held[1].ptr, 1, held[1].ptr, d_cnt.ptr)
                    else:
                        mirt.intersect_ordered_along_device(d32, held[0].ptr, nt, held[1].ptr, 1, held[1].ptr, d_cnt.ptr)
                    binned_stats(mirt.along_stats(), False, text)
                    mirt.sync()
                got = np.frombuffer(held[1].read().tobytes(), mirt.HIT_DTYPE)
                assert got.tobytes() == np.ascontiguousarray(wh[:, step]).tobytes(), text + ", BINNED, device form"
                assert np.array_equal(d_cnt.read(), (wc > step).astype(np.int32)), text
                with mode(BRUTE):
                    if several:
                        mirt._check(lib.mirt_intersect_ordered_alongs(P(d32), len(d32), P(of32), P(s32), nt, P(host_rec), 1, P(host_rec), P(cnt)))
                    else:
                        mirt._check(lib.mirt_intersect_ordered_along(P(d32), P(s32), nt, P(host_rec), 1, P(host_rec), P(cnt)))
                assert host_rec.tobytes() == got.tobytes() and np.array_equal(cnt, (wc > step).astype(np.int32)), text + ", BRUTE, host form"
                if not cnt.any():
                    break
            assert step == wc.max(), (step, wc.max())
    finally:
        for x in held:
            x.free()
    TOOK["along"].setdefault(case.pname, set()).add(cls)
    note(case, "ordered along %s, %s" % ("five" if several else dname, scene),
         "%s: BINNED %s; %s; auto %s; the peel took %d steps" % (cls, "built once, kept (B = %d)" % bins if cls == "binned" else "ran the sweep, built nothing",
                                                                 "the closest-hit call first" if along_first else "the ordered call first", took, step + 1))


# ---- the tests: one family and one placement each -------------------------------------------------------------------------------------------------

GRID_PNAMES = list(pl.GRID_PLACEMENTS)
PNAMES = list(pl.PLACEMENTS)


@pytest.mark.parametrize("pname", GRID_PNAMES)
def test_ray_grid(oracle, pname):
    for scene in SCENES:
        run_ray_grid(case_of(oracle, pname), scene)


@pytest.mark.parametrize("pname", GRID_PNAMES)
def test_ordered(oracle, pname):
    for scene in SCENES:
        run_ordered(case_of(oracle, pname), scene)


@pytest.mark.parametrize("pname", PNAMES)
def test_ordered_along_one_direction(oracle, pname):
    for scene in SCENES:
        for k, dname in enumerate(pl.SINGLE_DIRS):
            run_ordered_along(case_of(oracle, pname), scene, dname, along_first=(k == 0) == (scene == QUERY_SCENE))


@pytest.mark.parametrize("pname", PNAMES)
def test_ordered_along_five_directions(oracle, pname):
    for scene in SCENES:
        run_ordered_along(case_of(oracle, pname), scene, None, along_first=scene == TIE_SCENE)


@pytest.mark.parametrize("how", ["scene_transform", "set_objects + pose"])
def test_in_place(oracle, how):
    """The far placement and (10, -7, 5) reached from the unit upload with the unit scene's structures held -- the ray grid by a call
    under the switch, an along grid by an ordered call (each family's first call is made on the unit scene before the move) --: the
    first call of each family rebuilds (the families' own assertions: source 1, cube_source 1; at the far placement the ray grid gives
    up), and every answer equals the oracle on the downloaded rows."""
    for pname in (pl.FAR, "10_-7_5"):
        T, s = pl.PLACEMENTS[pname]
        assert s == 1.0

        def arrive(name, tris, warm):
            unit = pl.unit_scene(name)
            mirt.scene_upload(unit)
            with np.errstate(all="ignore"):
                warm()                                              # (the unit scene's structure, and results nobody looks at)
            if how == "scene_transform":
                mirt.scene_transform(0, len(unit), EYE, T)
            else:
                mirt.scene_set_objects([(0, 0, len(unit))])
                mirt.scene_pose([np.concatenate([EYE, np.asarray(T, np.float32)])])

        rows = {}
        for name in SCENES:
            arrive(name, None, lambda: None)
            got = mirt.scene_download()
            # one rounding a coordinate: the vertices are placement.place's, so the class tables speak of these rows too
            assert np.array_equal(got[:, :9], pl.placed_scene(name, pname)[:, :9]), name
            got.setflags(write=False)
            rows[name] = got
        # (rows that are placement.placed_scene's byte for byte, normals and colours too, have the answers the tests above computed)
        same_rows = all(rows[name].tobytes() == pl.placed_scene(name, pname).tobytes() for name in SCENES)
        case = case_of(oracle, pname) if same_rows else pg.PlacedGrid(oracle, pname, rows)
        for scene in SCENES:
            run_ray_grid(case, scene, arrive)
            run_ordered_along(case, scene, "oblique", arrive)
        run_ordered(case, QUERY_SCENE, arrive)
        run_ordered_along(case, QUERY_SCENE, None, arrive)
        assert pl.RAY_GRID_CLASS[QUERY_SCENE][pname] == ("gave_up" if pname == pl.FAR else "binned")
        assert pl.along_class(QUERY_SCENE, pname, "oblique") == "binned"


def test_every_class_is_met():
    """The classes the runs above took, and the tables they took them from, cover `binned`, `gave_up` and `no_grid` for the along grids
    and `binned` and one of the other two for the ray grid."""
    along = {pl.along_class(s, p, d) for s in SCENES for p in PNAMES for d in pl.SINGLE_DIRS} | {pl.alongs_class(s, p) for s in SCENES for p in PNAMES}
    grid = {pl.RAY_GRID_CLASS[s][p] for s in SCENES for p in GRID_PNAMES}
    assert along == {"binned", "gave_up", "no_grid"}, along
    assert "binned" in grid and grid & {"gave_up", "no_grid"}, grid
    for family, table, names in (("along", along, PNAMES), ("ray grid", grid, GRID_PNAMES)):
        took = set().union(*TOOK[family].values()) if TOOK[family] else set()
        assert took <= table, (family, took)
        if set(names) <= set(TOOK[family]):                          # (every placement ran in this process: the union is the table's)
            assert took == table, (family, took, table)
