"""Device-resident scenes on the GPU: mirt_scene_upload_device, mirt_scene_update*, mirt_scene_transform, mirt_scene_download and
mirt_scene_info (capi/scene.cpp; the kernels: scene/scene_kernels.hip) against mirt_scene_upload of the same values and against
the CPU oracle.

"Everything" a scene is compared by (`snapshot`): the triangles read back, finiteness and bounding box, a ray-traced frame under
BRUTE and under BINNED (index, distance, position, rgb, xrgb), a rasterised frame (rgb, 1/z, index, xrgb), and the records of
mirt_intersect, of mirt_direct_light under BINNED and of mirt_intersect_from under BINNED.  All of it bit for bit (uint32 views),
the box by value.  Frames are 96 x 64; scenes hold 30, 65 and 3001 triangles (neither 64 nor 256 divides them): Cornell-box
triangles followed by soup."""
import ctypes as C

import numpy as np
import pytest

import mirt
from devbuf import DeviceArray, to_device
from mirt_oracle import DEFAULT_LIGHT

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 96, 64
RT_CAM, RAS_CAM = (0.0, 0.0, -2.0), (0.0, 0.0, -3.0)
QLIGHTS = np.array([[0, -0.5, -0.75, 1, 1, 1, 14], [0.5, 0.25, -0.875, 1, 0.5, 0.25, 6]], F)   # not the frames' light: a cube of their own
ORIGIN = np.array([0.125, -0.0625, 0.1875], F)
INVALID, NO_SCENE = -3, -4
RT_KEYS = ("index", "dist", "pos", "rgb", "xrgb")
RAS_KEYS = ("rgb", "depth", "index", "xrgb")


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_query_mode(mirt.QUERY_AUTO)
    mirt.set_frames_in_flight(1)
    mirt.shutdown()


# ---- scenes, views, rays ------------------------------------------------------------------------------------------------------

_scenes = {}


def scene(n, seed=11):
    """20 Cornell triangles (the room and the short block) and n - 20 of a soup."""
    if (n, seed) not in _scenes:
        t = np.concatenate([mirt.scene_cornell()[:20], mirt.scene_soup(seed, n - 20, 0.25)])
        assert t.shape == (n, 15)
        t.setflags(write=False)
        _scenes[(n, seed)] = t
    return _scenes[(n, seed)]


def rt_view():
    return mirt.make_view(RT_CAM, mirt.rot_from_yaw(0.1, 1.0), H / 2.0, W, H)


def ras_view():
    return mirt.make_view(RAS_CAM, mirt.rot_from_yaw(0.0, 1.01), float(H), W, H)


def cull_of(tris):
    return mirt.cull(tris, ras_view(), 3)


def query_inputs():
    rng = np.random.default_rng(5)
    target = rng.uniform(-1, 1, (512, 3)).astype(F)
    start = np.array(RT_CAM, F) + rng.uniform(-0.25, 0.25, (512, 3)).astype(F)
    dirs = rng.uniform(-1, 1, (768, 3)).astype(F)
    return mirt.make_rays(start, (target - start).astype(F)), np.ascontiguousarray(dirs)


RAYS, DIRS = query_inputs()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def upload_device(tris, culled=None):
    d_t = to_device(tris)
    d_c = to_device(culled) if culled is not None else None
    try:
        mirt.scene_upload_device(d_t.ptr, len(tris), d_c.ptr if d_c else None)
    finally:                                                  # (the call returns with the scene complete: the source may go)
        d_t.free()
        if d_c:
            d_c.free()


def update(form, first, rows):
    if form == "host":
        mirt.scene_update(first, rows)
    else:
        d = to_device(rows)
        try:
            mirt.scene_update_device(first, len(rows), d.ptr)
        finally:
            d.free()


# ---- what a scene is compared by ---------------------------------------------------------------------------------------------

def queries(mode):
    """(records of mirt_intersect, DirectLight of those that hit, records of the origin fan, the two calls' statistics)."""
    mirt.set_query_mode(mode)
    try:
        hits = mirt.intersect(RAYS)
        lit = mirt.direct_light(hits[hits["index"] >= 0], QLIGHTS)
        qs = mirt.query_stats()
        fan = mirt.intersect_from(ORIGIN, DIRS)
        fs = mirt.fan_stats()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)
    return {"hits": hits, "lit": lit, "fan": fan}, qs, fs


def snapshot():
    info = mirt.scene_info()
    s = {"tris": mirt.scene_download(), "n": info["n"], "finite": info["finite"], "lo": info["bbox_lo"], "hi": info["bbox_hi"]}
    assert s["tris"].shape == (info["n"], 15) and mirt.load().mirt_scene_size() == info["n"]
    for mode in (mirt.RT_BRUTE, mirt.RT_BINNED):
        f = mirt.raytrace(rt_view(), DEFAULT_LIGHT, mode=mode, want_intersection=True)
        s["rt%d" % mode] = {k: f[k] for k in RT_KEYS}
        s["rt%d_mode" % mode] = f["stats"]["mode_used"]
    r = mirt.rasterise(ras_view(), DEFAULT_LIGHT)
    s["ras"] = {k: r[k] for k in RAS_KEYS}
    q, qs, fs = queries(mirt.QUERY_BINNED)
    s["q"] = q
    s["q_modes"] = (qs["mode_used"], fs["mode_used"])
    return s


def assert_same_snapshot(got, want, what):
    assert got["n"] == want["n"] and got["finite"] == want["finite"], (what, got["finite"], want["finite"])
    assert np.array_equal(got["lo"], want["lo"]) and np.array_equal(got["hi"], want["hi"]), (what, got["lo"], want["lo"], got["hi"], want["hi"])
    assert np.array_equal(bits(got["tris"]), bits(want["tris"])), "%s: the triangles read back differ" % what
    for mode in (mirt.RT_BRUTE, mirt.RT_BINNED):
        assert got["rt%d_mode" % mode] == want["rt%d_mode" % mode], what
        for k in RT_KEYS:
            assert np.array_equal(bits(got["rt%d" % mode][k]), bits(want["rt%d" % mode][k])), "%s: ray-traced %s, mode %d" % (what, k, mode)
    for k in RAS_KEYS:
        assert np.array_equal(bits(got["ras"][k]), bits(want["ras"][k])), "%s: rasterised %s" % (what, k)
    assert got["q_modes"] == want["q_modes"], what
    for k in ("hits", "lit", "fan"):
        assert got["q"][k].tobytes() == want["q"][k].tobytes(), "%s: query %s" % (what, k)


_oracle_frames = {}


def oracle_frames(oracle, tris, culled):
    key = (tris.tobytes(), None if culled is None else culled.tobytes())
    if key not in _oracle_frames:
        rt = oracle.raytrace(tris, RT_CAM, oracle.rot_from_yaw(0.1, 1.0), H / 2.0, W, H, DEFAULT_LIGHT, threads=16)
        ras = oracle.rasterise(tris, culled, RAS_CAM, oracle.rot_from_yaw(0.0, 1.01), float(H), W, H, DEFAULT_LIGHT)
        _oracle_frames[key] = (rt, ras)
    return _oracle_frames[key]


def assert_rt_equals_oracle(frame, ref, what):
    for k in RT_KEYS:
        assert np.array_equal(bits(frame[k]), bits(ref[k])), "%s: ray-traced %s differs from the oracle in %d words" % (
            what, k, int((bits(frame[k]) != bits(ref[k])).sum()))


def assert_equals_oracle(oracle, snap, tris, culled, what):
    rt, ras = oracle_frames(oracle, tris, culled)
    for mode in (mirt.RT_BRUTE, mirt.RT_BINNED):
        assert_rt_equals_oracle(snap["rt%d" % mode], rt, "%s, mode %d" % (what, mode))
    for k in RAS_KEYS:
        assert np.array_equal(bits(snap["ras"][k]), bits(ras[k])), "%s: rasterised %s differs from the oracle" % (what, k)


_host_snapshots = {}


def host_snapshot(tris, culled):
    """Everything after mirt_scene_upload of the array: once per array, shared, never changed."""
    key = (tris.tobytes(), None if culled is None else culled.tobytes())
    if key not in _host_snapshots:
        mirt.scene_upload(tris, culled)
        _host_snapshots[key] = snapshot()
    return _host_snapshots[key]


# ---- 1. device upload == host upload -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_cull", [False, True])
@pytest.mark.parametrize("n", [30, 65, 3001])
def test_device_upload_equals_host_upload(oracle, n, with_cull):
    tris = scene(n)
    culled = cull_of(tris) if with_cull else None
    if with_cull:
        assert 0 < int(culled.sum()) < n
    want = host_snapshot(tris, culled)
    if n == 3001:
        assert want["rt%d_mode" % mirt.RT_BINNED] == mirt.RT_BINNED and want["q_modes"] == (mirt.QUERY_BINNED, mirt.QUERY_BINNED)
    assert want["finite"] == 1
    mirt.scene_upload(scene(n, seed=12))                      # something else is on the device when the upload arrives
    v0 = mirt.scene_info()["version"]
    upload_device(tris, culled)
    assert mirt.scene_info()["version"] != v0
    got = snapshot()
    assert np.array_equal(bits(got["tris"]), bits(tris))
    assert np.array_equal(got["lo"], tris[:, :9].reshape(-1, 3).min(axis=0)) and np.array_equal(got["hi"], tris[:, :9].reshape(-1, 3).max(axis=0))
    assert_same_snapshot(got, want, "device upload, n = %d" % n)
    assert_equals_oracle(oracle, got, tris, culled, "device upload, n = %d" % n)
    if with_cull:
        assert np.array_equal(mirt.scene_get_culled(), culled)
    else:
        assert not mirt.scene_get_culled().any()


def test_device_upload_with_a_new_n_reallocates(oracle):
    for n in (3001, 30, 65):
        upload_device(scene(n))
        assert mirt.scene_info()["n"] == n
        assert_same_snapshot(snapshot(), host_snapshot(scene(n), None), "n = %d after another n" % n)


# ---- 2. partial updates --------------------------------------------------------------------------------------------------------

RANGES = [(3001, 255, 770), (3001, 0, 3001), (3001, 3000, 1), (3001, 0, 1), (65, 63, 2)]


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("n,first,count", RANGES)
def test_partial_update(oracle, n, first, count, form):
    tris = scene(n)
    culled = cull_of(tris)
    rows = scene(n, seed=13)[first:first + count]
    spliced = np.array(tris)
    spliced[first:first + count] = rows
    mirt.scene_upload(tris, culled)
    v0 = mirt.scene_info()["version"]
    update(form, first, rows)
    assert mirt.scene_info()["version"] != v0 and mirt.scene_info()["n"] == n
    assert np.array_equal(bits(mirt.scene_download(0, n)), bits(spliced))
    assert np.array_equal(bits(mirt.scene_download(first, count)), bits(rows))
    got = snapshot()
    assert np.array_equal(mirt.scene_get_culled(), culled)    # n and the cull flags stay as they are
    assert_same_snapshot(got, host_snapshot(spliced, culled), "update [%d, %d + %d) of %d, %s form" % (first, first, count, n, form))
    assert_equals_oracle(oracle, got, spliced, culled, "update [%d, %d + %d) of %d" % (first, first, count, n))


# ---- 3. nothing stale survives -------------------------------------------------------------------------------------------------

def binned_frame():
    f = mirt.raytrace(rt_view(), DEFAULT_LIGHT, mode=mirt.RT_BINNED, want_intersection=True)
    assert f["stats"]["mode_used"] == mirt.RT_BINNED
    return f


@pytest.mark.parametrize("change", ["update", "transform"])
def test_nothing_stale_survives(oracle, change):
    n, first, count = 3001, 255, 770
    tris = scene(n)
    mirt.set_frames_in_flight(1)
    mirt.scene_upload(tris)
    binned_frame()
    assert binned_frame()["stats"]["bins_reused"] == 1        # a standing view keeps its pass
    queries(mirt.QUERY_BINNED)
    _, qs, fs = queries(mirt.QUERY_BINNED)
    assert qs["cube_source"] == 2 and fs["cube_source"] == 2  # ... and the queries their cubes
    if change == "update":
        new = np.array(tris)
        new[first:first + count] = scene(n, seed=14)[first:first + count]
        mirt.scene_update(first, new[first:first + count])
    else:
        rot, tr = mirt.rot_from_yaw(0.6, 1.0), (0.1, -0.2, 0.3)
        new = np.array(tris)
        new[first:first + count] = mirt.transform(tris[first:first + count], rot, tr)
        mirt.scene_transform(first, count, rot, tr)
    ref, _ = oracle_frames(oracle, new, None)
    old, _ = oracle_frames(oracle, tris, None)
    assert not np.array_equal(ref["index"], old["index"]), "the change does not change the picture"
    f = binned_frame()
    assert f["stats"]["bins_reused"] == 0
    assert_rt_equals_oracle(f, ref, "first frame after the %s" % change)
    got, qs, fs = queries(mirt.QUERY_BINNED)
    assert qs["mode_used"] == mirt.QUERY_BINNED and fs["mode_used"] == mirt.QUERY_BINNED
    assert qs["cube_source"] == 1 and fs["cube_source"] == 1  # built again, for the new scene
    want, _, _ = queries(mirt.QUERY_BRUTE)
    for k in ("hits", "lit", "fan"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert binned_frame()["stats"]["bins_reused"] == 1


# ---- 4. transform ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,first,count", [(3001, 0, 3001), (3001, 255, 770), (3001, 1500, 1), (65, 63, 2)])
def test_transform_equals_the_host_arithmetic(oracle, n, first, count):
    tris = np.array(scene(n))
    deg = first + count // 2
    tris[deg, 3:6] = tris[deg, 0:3]                           # one degenerate triangle in the range: v1 == v0
    mirt.scene_upload(tris)
    want = tris
    for rot, tr in [(mirt.rot_from_yaw(0.7, 1.01), (0.25, -0.5, 1.0)), (mirt.rot_from_yaw(-0.4, 1.0), (-0.2, 0.4, -0.9))]:
        v0 = mirt.scene_info()["version"]
        mirt.scene_transform(first, count, rot, tr)
        assert mirt.scene_info()["version"] != v0
        want = np.array(want)
        want[first:first + count] = mirt.transform(want[first:first + count], rot, tr)
        got = mirt.scene_download()
        assert np.isnan(got[deg, 9:12]).all() and np.isnan(want[deg, 9:12]).all()
        keep = np.ones(got.shape, bool)
        keep[deg, 9:12] = False
        assert np.array_equal(bits(got)[keep], bits(want)[keep]), int((bits(got)[keep] != bits(want)[keep]).sum())
        assert not np.isnan(got[keep]).any()
    info = mirt.scene_info()
    assert info["finite"] == 0                                # the NaN normal counts, as in the host scan of mirt_scene_upload
    assert np.array_equal(info["bbox_lo"], want[:, :9].reshape(-1, 3).min(axis=0)) and np.array_equal(info["bbox_hi"], want[:, :9].reshape(-1, 3).max(axis=0))
    # frames on the moved scene (the degenerate triangle made whole again, so that the binned path is taken) equal the oracle on
    # the host-moved array
    whole = np.array(want[deg])
    whole[3:6] = whole[0:3] + F(0.125)
    whole = mirt.transform(whole, np.eye(3, dtype=F).ravel(), (0, 0, 0))[0]
    mirt.scene_update(deg, whole)
    want[deg] = whole
    snap = snapshot()
    assert snap["finite"] == 1
    assert np.array_equal(bits(snap["tris"]), bits(want))
    assert_same_snapshot(snap, host_snapshot(want, None), "transformed [%d, %d + %d) of %d" % (first, first, count, n))
    assert_equals_oracle(oracle, snap, want, None, "transformed [%d, %d + %d) of %d" % (first, first, count, n))


# ---- 5. bounds and finiteness follow the data both ways -----------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["host", "device"])
def test_bounds_and_finiteness_follow_the_data(oracle, form):
    n, t = 3001, 1234
    tris = scene(n)
    mirt.scene_upload(tris)
    box0 = mirt.scene_info()
    assert box0["finite"] == 1
    lo0, hi0 = tris[:, :9].reshape(-1, 3).min(axis=0), tris[:, :9].reshape(-1, 3).max(axis=0)
    assert np.array_equal(box0["bbox_lo"], lo0) and np.array_equal(box0["bbox_hi"], hi0)
    assert tris[t, 3] < hi0[0]
    for k, value in [(3, F(1e9)), (3, F("inf")), (3, F("nan")), (13, F("nan"))]:          # v1.x three times, then a colour component
        row = np.array(tris[t:t + 1])
        row[0, k] = value
        new = np.array(tris)
        new[t] = row[0]
        # the host rule: fminf / fmaxf skip a NaN, an infinity counts -- 1e9 and inf widen the box, NaN does not
        lo, hi = np.fmin.reduce(new[:, :9].reshape(-1, 3), axis=0), np.fmax.reduce(new[:, :9].reshape(-1, 3), axis=0)
        assert np.array_equal(lo, lo0) and (hi[0] == value if k == 3 and not np.isnan(value) else np.array_equal(hi, hi0))
        update(form, t, row)
        info = mirt.scene_info()
        assert info["finite"] == 0, (k, value)
        assert np.array_equal(info["bbox_lo"], lo) and np.array_equal(info["bbox_hi"], hi), (k, value, info["bbox_lo"], info["bbox_hi"])
        f = mirt.raytrace(rt_view(), DEFAULT_LIGHT, mode=mirt.RT_BINNED, want_intersection=True)
        assert f["stats"]["mode_used"] == mirt.RT_BRUTE       # a scene that is not finite takes the brute path
        assert_rt_equals_oracle(f, oracle_frames(oracle, new, None)[0], "float %d = %s" % (k, value))
        # ... and the values are the ones a host upload of the same array decides with
        mirt.scene_upload(new)
        want = mirt.scene_info()
        assert want["finite"] == 0 and np.array_equal(want["bbox_lo"], info["bbox_lo"]) and np.array_equal(want["bbox_hi"], info["bbox_hi"])
    update(form, t, tris[t:t + 1])                            # back: the box shrinks again
    info = mirt.scene_info()
    assert info["finite"] == 1
    assert np.array_equal(bits(info["bbox_lo"]), bits(box0["bbox_lo"])) and np.array_equal(bits(info["bbox_hi"]), bits(box0["bbox_hi"]))
    f = mirt.raytrace(rt_view(), DEFAULT_LIGHT, mode=mirt.RT_BINNED, want_intersection=True)
    assert f["stats"]["mode_used"] == mirt.RT_BINNED
    assert_rt_equals_oracle(f, oracle_frames(oracle, tris, None)[0], "the triangle put back")


def test_an_axis_without_a_number_stays_infinite():
    tris = np.array(scene(30))
    tris[:, 1:9:3] = F("nan")                                 # every y
    upload_device(tris)
    info = mirt.scene_info()
    assert info["finite"] == 0 and info["bbox_lo"][1] == F("inf") and info["bbox_hi"][1] == F("-inf")
    assert info["bbox_lo"][0] == tris[:, 0:9:3].min() and info["bbox_hi"][2] == tris[:, 2:9:3].max()
    mirt.scene_upload(tris)
    want = mirt.scene_info()
    assert want["finite"] == 0 and np.array_equal(want["bbox_lo"], info["bbox_lo"]) and np.array_equal(want["bbox_hi"], info["bbox_hi"])


# ---- 6. frames in flight ----------------------------------------------------------------------------------------------------------

def test_frames_in_flight_finish_on_the_old_scene(oracle):
    n, first, count = 3001, 255, 770
    tris = scene(n)
    new = np.array(tris)
    new[first:first + count] = scene(n, seed=14)[first:first + count]
    old_ref, new_ref = oracle_frames(oracle, tris, None)[0]["xrgb"], oracle_frames(oracle, new, None)[0]["xrgb"]
    assert not np.array_equal(old_ref, new_ref)
    planes = [DeviceArray((H, W), np.uint32, 0) for _ in range(8)]
    d_rows = to_device(new[first:first + count])
    try:
        mirt.scene_upload(tris)
        mirt.set_frames_in_flight(4)
        view = rt_view()
        for p in planes[:4]:
            mirt.raytrace_device(view, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, p.ptr, W * 4)
        mirt.scene_update_device(first, count, d_rows.ptr)    # no mirt_sync in between
        for p in planes[4:]:
            mirt.raytrace_device(view, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, p.ptr, W * 4)
        mirt.sync()
        for i, p in enumerate(planes):
            want = old_ref if i < 4 else new_ref
            assert np.array_equal(p.read()[1:-1, 1:-1], want[1:-1, 1:-1]), "frame %d" % i
    finally:
        mirt.set_frames_in_flight(1)
        d_rows.free()
        for p in planes:
            p.free()


# ---- 7. arguments -------------------------------------------------------------------------------------------------------------------

def test_arguments():
    lib = mirt.load()
    n = 65
    tris = scene(n)
    mirt.scene_upload(tris)
    host = np.zeros((n + 1, 15), F)
    hp = host.ctypes.data
    dev = DeviceArray(((n + 1) * 15,), F)
    dp = dev.ptr.value
    eye, zero = np.eye(3, dtype=F).ravel(), np.zeros(3, F)
    r, z = eye.ctypes.data_as(C.c_void_p), zero.ctypes.data_as(C.c_void_p)
    v0 = mirt.scene_info()["version"]
    try:
        calls = {
            "update_device": lambda first, count, p=dp: lib.mirt_scene_update_device(first, count, C.c_void_p(p) if p else None),
            "update": lambda first, count, p=hp: lib.mirt_scene_update(first, count, C.c_void_p(p) if p else None),
            "download": lambda first, count, p=hp: lib.mirt_scene_download(first, count, C.c_void_p(p) if p else None),
            "transform": lambda first, count, p=None: lib.mirt_scene_transform(first, count, r, z),
        }
        for name, call in calls.items():
            for first, count in [(-1, 1), (0, n + 1), (n, 1), (1, n), (60, 6), (0, -1), (n, -1), (2 ** 31 - 1, 2 ** 31 - 1)]:
                assert call(first, count) == INVALID, (name, first, count)
            if name != "transform":
                assert call(0, 1, 0) == INVALID, name                        # a NULL array with count > 0
                base = dp if name == "update_device" else hp
                for off in (1, 2, 3):
                    assert call(0, 1, base + off) == INVALID, (name, off)    # not 4-byte aligned
                assert b"aligned" in lib.mirt_last_error()
            assert call(0, 0) == 0 and call(n, 0) == 0 and call(17, 0) == 0, name     # count == 0 does nothing
            if name != "transform":
                assert call(3, 0, 0) == 0, name
        assert lib.mirt_scene_transform(0, 1, None, z) == INVALID and lib.mirt_scene_transform(0, 1, r, None) == INVALID
        assert lib.mirt_scene_info(None) == INVALID
        assert lib.mirt_scene_upload_device(None, None, n) == INVALID and lib.mirt_scene_upload_device(C.c_void_p(dp), None, 0) == INVALID
        assert lib.mirt_scene_upload_device(C.c_void_p(dp + 2), None, n) == INVALID
        assert mirt.scene_info()["version"] == v0 and mirt.scene_info()["n"] == n
        assert np.array_equal(bits(mirt.scene_download()), bits(tris)) and not host.any()
        # a valid call for contrast
        assert calls["update"](n - 1, 1) == 0 and mirt.scene_info()["version"] != v0
        # before any scene
        mirt.shutdown()
        mirt.init(0)
        for name, call in calls.items():
            assert call(0, 1) == NO_SCENE, name
        assert lib.mirt_scene_info(C.byref(mirt.SceneInfo())) == NO_SCENE
        assert b"no scene uploaded" in lib.mirt_last_error()
        assert calls["update"](-1, 1) == INVALID              # ... what is wrong without a scene too comes first
    finally:
        dev.free()
