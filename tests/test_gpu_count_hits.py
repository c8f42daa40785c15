"""The number of hits along a ray on the GPU: mirt_count_hits* (k_count_wave, k_count_lanes), mirt_count_hits_along* (k_along_count)
and mirt_count_hits_alongs* (k_alongs_count) against the CPU oracle, count for count.

The expectation is the per-triangle table of ordered_helpers.table -- one oracle ClosestIntersection call per (ray, triangle) on a fresh
record -- with the contract's predicate applied in numpy (count_helpers.expected).  Every call goes through a count buffer prefilled
with 0xAA with guard counts behind it: each count of the call is written, and nothing beyond.  The deep scene `plates` (24 squares
behind one another) gives rays of up to 24 hits, three times what mirt_intersect_ordered* holds; tests/test_count_host.py shows on
the oracle alone that the inputs reach the cases they are there for."""
import numpy as np
import pytest

import mirt
import count_helpers as K
import ordered_helpers as O
from along_helpers import OBLIQUE, SHELLS

pytestmark = pytest.mark.gpu

INVALID = -3
BRUTE, BINNED, AUTO = mirt.QUERY_BRUTE, mirt.QUERY_BINNED, mirt.QUERY_AUTO
call = K.count_call
same = K.same_counts


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_query_mode(mirt.QUERY_AUTO)
    mirt.set_ray_grid(False)
    mirt.set_profiling(False)
    mirt.shutdown()


def mode_is(st, mode, what, source=None):
    if mode == BRUTE:
        assert st["mode_used"] == BRUTE and st["cube_source"] == 0 and st["cube_bins"] == 0, (what, st)
    else:
        assert st["mode_used"] == BINNED and st["cube_source"] in ((1, 2) if source is None else (source,)) and st["cube_bins"] >= 8 and st["shells"] == SHELLS, (what, st)


def variants(rec):
    """(label, after, limits) of a case: neither, each alone, and both in two further rotations -- all 11 `after` kinds made from the
    ray's own slot 0 and all 13 limit kinds made from its own distances, rotated over the rays."""
    slot0 = K.slot0_of(rec)
    out = [("plain", None, None), ("after", O.after_records(slot0, 0)[0], None), ("limits", None, K.limits_of(rec, 0)[0])]
    for shift in (3, 7):
        out.append(("after and limits, rotation %d" % shift, O.after_records(slot0, shift)[0], K.limits_of(rec, shift + 2)[0]))
    return out


# ---- 1: the sweep ---------------------------------------------------------------------------------------------------------------------------

SWEEPS = [(name, n) for name in ("plates", "cornell", "soup65x2", "wall") for n in (257, 4097)] + [("soup2000", 1025)]


@pytest.mark.parametrize("name,n", SWEEPS)
def test_the_sweep_equals_the_oracle(oracle, name, n):
    """257 and 1025 rays take the wave-per-ray kernel, 4097 the lane-per-ray kernel; host and device forms; with and without `after`
    and limits; and under mirt_set_ray_grid(1) the same counts with the grid's statistics untouched."""
    rays = K.rays_of(name, n)
    rec = K.table_of(oracle, name, rays)
    plain = K.expected(rec)
    print("%s, %d rays: above 8 hits %d, none %d, most %d" % (name, n, (plain > 8).sum(), (plain == 0).sum(), plain.max()))
    if name == "plates":
        assert (plain > 16).sum() >= n // 11
    mirt.scene_upload(K.scene(name))
    got = {}
    for label, after, limits in variants(rec):
        want = K.expected(rec, after, limits)
        if label != "plain":
            print("  %s: changes %d counts" % (label, (want != plain).sum()))
            assert (want != plain).any(), label + ": the variant changes no count"
        for form in ("host", "device"):
            what = "%s, %d rays, %s, %s form" % (name, n, label, form)
            got[label] = call(form, "rays", None, rays, after=after, limits=limits, what=what)[0]
            same(got[label], want, what)
    # mirt_set_ray_grid(1): a closest-hit call walks the grid and is what its statistics report; the count call sweeps and leaves them
    mirt.set_ray_grid(True)
    try:
        mirt.intersect(rays[:65])
        before = mirt.ray_grid_stats()
        for label, after, limits in variants(rec)[:1] + variants(rec)[-1:]:
            what = "%s, %d rays, %s, under the ray grid" % (name, n, label)
            same(call("device", "rays", None, rays, after=after, limits=limits, what=what)[0], got[label], what)
        assert mirt.ray_grid_stats() == before, "the count call touched the ray grid's statistics"
        if name in O.GRID_SCENES:
            assert before["mode_used"] == BINNED, before
    finally:
        mirt.set_ray_grid(False)


def test_the_wrappers_and_an_empty_call(oracle):
    rays = K.rays_of("plates", 257)
    rec = K.table_of(oracle, "plates", rays)
    mirt.scene_upload(K.scene("plates"))
    limits = K.limits_of(rec, 1)[0]
    after = O.after_records(K.slot0_of(rec), 2)[0]
    c = mirt.count_hits(rays, after=after, max_distance=limits)
    assert c.dtype == np.int32 and c.shape == (257,)
    same(c, K.expected(rec, after, limits), "mirt.count_hits")
    same(mirt.count_hits(rays, max_distance=0.5), K.expected(rec, None, np.full(257, 0.5, np.float32)), "mirt.count_hits, one limit for all")
    assert mirt.count_hits(rays[:0]).shape == (0,)
    d = K.PLATE_DIRS[2]
    tris, starts, planted, rec = K.along_case(oracle, "plates", d, 257)
    for mode in (BRUTE, BINNED):
        mirt.set_query_mode(mode)
        try:
            same(mirt.count_hits_along(d, starts), K.expected(rec), "mirt.count_hits_along")
            same(mirt.count_hits_alongs([d], None, starts, max_distance=1.25), K.expected(rec, None, np.full(257, 1.25, np.float32)),
                 "mirt.count_hits_alongs, one direction, no indices")
        finally:
            mirt.set_query_mode(AUTO)
    assert mirt.count_hits_along(d, starts[:0]).shape == (0,)
    lib = mirt.load()
    assert lib.mirt_count_hits_device(None, 0, None, None, None) == 0 and lib.mirt_count_hits_alongs_device(None, 0, None, None, 0, None, None, None) == 0


def test_invalid_arguments():
    """-3 and a text for every bad argument of all six entry points on an initialised library; nothing is written."""
    mirt.scene_upload(mirt.scene_cornell())
    lib = mirt.load()
    cases, keep, snapshot = K.bad_calls()
    before = snapshot()
    for name, args, why in cases:
        assert getattr(lib, name)(*args) == INVALID, (name, why)
        assert lib.mirt_last_error(), (name, why)
    assert snapshot() == before, "a refused call wrote something"


# ---- 2: along one direction -------------------------------------------------------------------------------------------------------------------

ALONG = [("plates", 0, 257), ("plates", 1, 257), ("plates", 2, 257), ("soup65x2", 1, 257), ("cornell", 1, 257), ("soup2000", 1, 1025)]


@pytest.mark.parametrize("name,which,n", ALONG)
def test_along_equals_the_oracle(oracle, name, which, n):
    """BINNED and BRUTE equal the oracle and each other; the first binned call builds the grid (cube_source 1), a repeat finds it kept
    (2), and AUTO takes a kept grid; the planted unfit starts sweep (fallback_records, with profiling on)."""
    d = K.PLATE_DIRS[which]
    tris, starts, planted, rec = K.along_case(oracle, name, d, n)
    assert planted.sum() >= 3
    mirt.scene_upload(tris)
    first = True
    for label, after, limits in variants(rec):
        want = K.expected(rec, after, limits)
        got = {}
        for mname, mode in (("binned", BINNED), ("brute", BRUTE), ("auto", AUTO)):
            for form in ("device", "host"):
                what = "%s along %r, %d rays, %s, %s form, %s" % (name, d.tolist(), n, label, form, mname)
                got[mname], st = call(form, "along", d, starts, after=after, limits=limits, mode=mode, what=what)
                mode_is(st, BINNED if mode == AUTO else mode, what, source=None if mode == BRUTE else (1 if first else 2))
                first = False
                same(got[mname], want, what)
        same(got["binned"], got["brute"], "%s, %s: BINNED vs BRUTE" % (name, label))
    # a fresh upload, a small AUTO call: nothing is held, the sweep answers
    mirt.scene_upload(tris)
    got, st = call("device", "along", d, starts[:65], mode=AUTO)
    mode_is(st, BRUTE, name + ", AUTO with nothing held")
    same(got, K.expected(rec)[:65], name + ", AUTO with nothing held")
    mirt.set_profiling(True)
    try:
        got, st = call("device", "along", d, starts, mode=BINNED)
        print(name, st)
        assert st["mode_used"] == BINNED and st["cube_source"] == 1 and st["shadow_rays"] == n, st
        assert st["fallback_records"] == int(planted.sum()) > 0, (st, int(planted.sum()))
        assert 0 < st["tests"] <= st["candidates"] and st["candidates"] >= int(planted.sum()) * len(tris), st
        same(got, K.expected(rec), name + ", profiling on")
    finally:
        mirt.set_profiling(False)


def test_a_grid_serves_both_families(oracle):
    """A grid mirt_occluded_along built serves the count call, and the other way round."""
    d = K.PLATE_DIRS[1]
    tris, starts, planted, rec = K.along_case(oracle, "plates", d, 257)
    limits = K.limits_of(rec, 0)[0]
    mirt.set_query_mode(BINNED)
    try:
        mirt.scene_upload(tris)
        occ = mirt.occluded_along(d, starts, limits)
        assert mirt.along_stats()["cube_source"] == 1
        got = mirt.count_hits_along(d, starts, max_distance=limits)
        st = mirt.along_stats()
        assert st["mode_used"] == BINNED and st["cube_source"] == 2, st
        same(got, K.expected(rec, None, limits), "behind mirt_occluded_along's build")
        assert np.array_equal(got > 0, occ == 1)
        mirt.scene_upload(tris)
        got = mirt.count_hits_along(d, starts, max_distance=limits)
        assert mirt.along_stats()["cube_source"] == 1
        same(got, K.expected(rec, None, limits), "its own build")
        assert np.array_equal(mirt.occluded_along(d, starts, limits), occ)
        st = mirt.along_stats()
        assert st["mode_used"] == BINNED and st["cube_source"] == 2, st
    finally:
        mirt.set_query_mode(AUTO)


def edge_on_plates(oracle):
    """Direction (1, 0, 0) on the plates: every plate is edge-on.  (want, {mode name: (counts, along_stats)})."""
    d = np.array([1, 0, 0], np.float32)
    tris, starts, planted, rec = K.along_case(oracle, "plates", d, 257)
    want = K.expected(rec)
    mirt.scene_upload(tris)
    return want, {mname: call("device", "along", d, starts, mode=mode, what="edge-on, " + mname) for mname, mode in (("brute", BRUTE), ("binned", BINNED))}


def test_the_plates_edge_on_counts(oracle):
    """Every plate edge-on: the counts are right under BRUTE and under BINNED (the reference accepts nothing: den is 0 for every row)."""
    want, got = edge_on_plates(oracle)
    print("plates along (1, 0, 0): rays with a hit %d, most %d" % ((want > 0).sum(), want.max()))
    for mname in got:
        same(got[mname][0], want, "edge-on, " + mname)


def test_the_plates_edge_on_sweep(oracle):
    """Every plate is edge-on, so the whole call sweeps and mode_used is BRUTE -- under BINNED too: all 48 triangles go on the grid's
    every-ray list (within its floor of 64 rows, so the build does not give up), no cell holds a row, and a count call takes the sweep
    for such a grid (capi/count.cpp).  mirt_occluded_along keeps walking that grid."""
    want, got = edge_on_plates(oracle)
    for mname in got:
        print(mname, got[mname][1])
    for mname in got:
        mode_is(got[mname][1], BRUTE, "edge-on, " + mname)
    d = np.array([1, 0, 0], np.float32)
    starts = K.starts_of("plates", d, 257)[0]
    mirt.set_query_mode(BINNED)
    try:
        assert not mirt.occluded_along(d, starts).any()
        assert mirt.along_stats()["mode_used"] == BINNED, mirt.along_stats()
        same(mirt.count_hits_along(d, starts), want, "edge-on, behind the occlusion call")
        mode_is(mirt.along_stats(), BRUTE, "edge-on, behind the occlusion call")
    finally:
        mirt.set_query_mode(AUTO)


# ---- 3: along several directions --------------------------------------------------------------------------------------------------------------

def alongs_case(oracle, dirs, n=257):
    """(starts, dir_of, table): ordered_along_helpers.starts_of along the first direction, the directions dealt over the rays in turn."""
    dirs = np.ascontiguousarray(dirs, np.float32)
    starts = K.starts_of("plates", dirs[0], n)[0]
    of = (np.arange(n) % len(dirs)).astype(np.int32)
    return starts, of, K.table_of(oracle, "plates", mirt.make_rays(starts, dirs[of]))


def seventy_directions():
    rng = np.random.default_rng(11)
    base = np.array(K.PLATE_DIRS, np.float32)
    more = base[rng.integers(0, 3, 67)] + rng.uniform(-0.2, 0.2, (67, 3)).astype(np.float32)
    return np.concatenate([base, more.astype(np.float32)])


@pytest.mark.parametrize("ndirs", [3, 70])
def test_alongs_equals_the_oracle(oracle, ndirs):
    """Three directions mixed ray by ray, and 70 directions, which run in passes: BINNED and BRUTE equal the oracle; the first binned
    call builds its groups, a repeat finds them kept."""
    dirs = np.array(K.PLATE_DIRS, np.float32) if ndirs == 3 else seventy_directions()
    assert len(dirs) == ndirs
    starts, of, rec = alongs_case(oracle, dirs)
    plain = K.expected(rec)
    assert (plain > 8).sum() >= 60 and (plain == 0).sum() >= 25, ((plain > 8).sum(), (plain == 0).sum())
    mirt.scene_upload(K.scene("plates"))
    first = True
    for label, after, limits in variants(rec):
        want = K.expected(rec, after, limits)
        got = {}
        for mname, mode in (("binned", BINNED), ("brute", BRUTE)):
            for form in ("device", "host"):
                what = "%d directions, %s, %s form, %s" % (ndirs, label, form, mname)
                got[mname], st = call(form, "alongs", dirs, starts, of=of, after=after, limits=limits, mode=mode, what=what)
                mode_is(st, mode, what, source=None if mode == BRUTE else (1 if first else 2))
                first = False
                same(got[mname], want, what)
        same(got["binned"], got["brute"], "%d directions, %s: BINNED vs BRUTE" % (ndirs, label))


def test_alongs_indices_outside_the_list(oracle):
    """A _device call with two indices outside the list writes those counts 0 and leaves the rest right, binned and swept."""
    dirs = np.array(K.PLATE_DIRS, np.float32)
    starts, of, rec = alongs_case(oracle, dirs)
    want = K.expected(rec)
    stray = [int(np.flatnonzero(want > 8)[0]), int(np.flatnonzero(want > 8)[1])]
    of = of.copy()
    of[stray[0]], of[stray[1]] = -1, 3
    want = want.copy()
    want[stray] = 0
    mirt.scene_upload(K.scene("plates"))
    for mname, mode in (("binned", BINNED), ("brute", BRUTE)):
        got, st = call("device", "alongs", dirs, starts, of=of, mode=mode, what=mname)
        mode_is(st, mode, mname)
        same(got, want, "two indices outside the list, " + mname)


def test_groups_are_shared_with_the_occlusion_calls(oracle):
    dirs = np.array(K.PLATE_DIRS, np.float32)
    starts, of, rec = alongs_case(oracle, dirs)
    limits = K.limits_of(rec, 5)[0]
    mirt.set_query_mode(BINNED)
    try:
        mirt.scene_upload(K.scene("plates"))
        occ = mirt.occluded_alongs(dirs, of, starts, limits)
        assert mirt.along_stats()["cube_source"] == 1
        got = mirt.count_hits_alongs(dirs, of, starts, max_distance=limits)
        st = mirt.along_stats()
        assert st["mode_used"] == BINNED and st["cube_source"] == 2, st
        same(got, K.expected(rec, None, limits), "behind mirt_occluded_alongs' build")
        assert np.array_equal(got > 0, occ == 1)
        mirt.scene_upload(K.scene("plates"))
        mirt.count_hits_alongs(dirs, of, starts)
        assert mirt.along_stats()["cube_source"] == 1
        assert np.array_equal(mirt.occluded_alongs(dirs, of, starts, limits), occ)
        assert mirt.along_stats()["cube_source"] == 2
    finally:
        mirt.set_query_mode(AUTO)


# ---- 4: the three identities, against the library's own ordered and occlusion calls ----------------------------------------------------

def family_calls(family, head, per_ray, of):
    """(count, ordered, occluded) of a family as functions of (after, limits / max_hits)."""
    if family == "rays":
        return (lambda after, lim: mirt.count_hits(per_ray, after, lim), lambda after, m: mirt.intersect_ordered(per_ray, m, after),
                lambda lim: mirt.occluded(per_ray, lim))
    if family == "along":
        return (lambda after, lim: mirt.count_hits_along(head, per_ray, after, lim), lambda after, m: mirt.intersect_ordered_along(head, per_ray, m, after),
                lambda lim: mirt.occluded_along(head, per_ray, lim))
    return (lambda after, lim: mirt.count_hits_alongs(head, of, per_ray, after, lim), lambda after, m: mirt.intersect_ordered_alongs(head, of, per_ray, m, after),
            lambda lim: mirt.occluded_alongs(head, of, per_ray, lim))


# (mirt_count_hits has one path: mirt_set_query_mode does not affect it)
FAMILIES = [("rays", "sweep", AUTO), ("along", "brute", BRUTE), ("along", "binned", BINNED), ("alongs", "brute", BRUTE), ("alongs", "binned", BINNED)]


@pytest.mark.parametrize("family,mname,mode", FAMILIES)
@pytest.mark.parametrize("name", ("plates", "soup65x2"))
def test_identities(oracle, name, family, mname, mode):
    """1: without `after` and limit the count is the number of records repeated mirt_intersect_ordered* peels enumerate.  2: with the
    same `after` and no limit min(count, K) is that call's count for K = 1, 2, 4, 8.  3: without `after`, count > 0 is the byte of
    mirt_occluded* for the same limit, +inf, NaN, 0 and negative limits among them."""
    n = 257
    dirs = np.array(K.PLATE_DIRS, np.float32)
    if family == "rays":
        head, of, per_ray = None, None, K.rays_of(name, n)
        rays = per_ray
    elif family == "along":
        head, of, per_ray = OBLIQUE, None, K.starts_of(name, OBLIQUE, n)[0]
        rays = mirt.make_rays(per_ray, head)
    else:
        head, per_ray = dirs, K.starts_of(name, dirs[0], n)[0]
        of = (np.arange(n) % 3).astype(np.int32)
        rays = mirt.make_rays(per_ray, dirs[of])
    rec = K.table_of(oracle, name, rays)
    count, ordered, occluded = family_calls(family, head, per_ray, of)
    mirt.scene_upload(K.scene(name))
    mirt.set_query_mode(mode)
    try:
        total = count(None, None)
        same(total, K.expected(rec), "%s, %s, %s" % (name, family, mname))
        # 1: peels of eight
        peeled, after = np.zeros(n, np.int64), None
        for rnd in range(8):
            hits, c = ordered(after, 8)
            peeled += c
            if (c < 8).all():
                break
            after = O.last_records(hits, c, 8)
        else:
            raise AssertionError("the enumeration does not end")
        assert np.array_equal(peeled, total), "identity 1: the peels enumerate %d records, the counts sum to %d" % (peeled.sum(), total.sum())
        if name == "plates":
            assert rnd >= 2 and (total > 16).sum() >= 20, "no ray needs a third peel"
        # 2: behind the same `after`
        after = O.after_records(K.slot0_of(rec), 5)[0]
        behind = count(after, None)
        for m in (1, 2, 4, 8):
            assert np.array_equal(np.minimum(behind, m), ordered(after, m)[1]), "identity 2, K = %d" % m
        # 3: the occlusion byte
        for shift in (0, 6):
            limits, kind = K.limits_of(rec, shift)
            assert set(range(K.LIMIT_KINDS)) <= set(kind.tolist())
            assert np.array_equal(count(None, limits) > 0, occluded(limits) == 1), "identity 3"
        assert np.array_equal(total > 0, occluded(None) == 1), "identity 3, no limit"
    finally:
        mirt.set_query_mode(AUTO)
