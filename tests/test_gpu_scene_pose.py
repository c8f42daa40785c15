"""Posed scenes on the GPU: mirt_scene_set_objects and mirt_scene_pose (capi/scene.cpp, capi/object_plan.hpp; the kernel:
scene/scene_kernels.hip, k_scene_range under SCENE_POSE).

The yardstick is always a HOST UPLOAD of the rows mirt_pose produced on a host mirror: the posed device scene must be
indistinguishable from it by everything a scene is compared by (`snapshot`, as tests/test_gpu_scene_device.py takes it): the
triangles read back, finiteness and bounding box, a ray-traced frame under BRUTE and under BINNED (index, distance, position, rgb,
xrgb), a rasterised frame (rgb, 1/z, index, xrgb), and the records of mirt_intersect, of mirt_direct_light under BINNED and of
mirt_intersect_from under BINNED.  All of it bit for bit (uint32 views; of the triangles read back: where the yardstick is not
NaN), the box by value.  Frames are 96 x 64; scenes hold 30, 65 and 3001 triangles: Cornell-box triangles followed by soup."""
import ctypes as C

import numpy as np
import pytest

import mirt
from devbuf import DeviceArray
from mirt_oracle import DEFAULT_LIGHT

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 96, 64
RT_CAM, RAS_CAM = (0.0, 0.0, -2.0), (0.0, 0.0, -3.0)
QLIGHTS = np.array([[0, -0.5, -0.75, 1, 1, 1, 14], [0.5, 0.25, -0.875, 1, 0.5, 0.25, 6]], F)
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


# ---- scenes, transforms, views, rays ------------------------------------------------------------------------------------------

_scenes = {}


def scene(n, seed=11):
    """20 Cornell triangles (the room and the short block) and n - 20 of a soup."""
    if (n, seed) not in _scenes:
        t = np.concatenate([mirt.scene_cornell()[:20], mirt.scene_soup(seed, n - 20, 0.25)])
        assert t.shape == (n, 15)
        t.setflags(write=False)
        _scenes[(n, seed)] = t
    return _scenes[(n, seed)]


def xform(yaw, m11, tr):
    return np.concatenate([mirt.rot_from_yaw(yaw, m11), np.asarray(tr, F)]).astype(F)


IDENTITY = xform(0.0, 1.0, (0.0, 0.0, 0.0))
XFORMS = np.stack([xform(0.7, 1.01, (0.25, -0.5, 0.5)), xform(-0.4, 1.0, (-0.2, 0.4, -0.3)), xform(2.5, 0.75, (0.0, 0.0, 0.0)),
                   xform(0.05, 1.0, (0.5, 0.125, -0.25)), xform(-1.3, 1.25, (0.0, -0.25, 0.5)), xform(3.0, 1.0, (-0.75, 0.0, 0.0))])
# objects of 1, 255, 256, 257 and 513 rows at offsets that are no multiples of 256, and an empty one between two others
SIZES = [(3, 1), (27, 255), (300, 256), (601, 257), (900, 0), (1001, 513)]
# instances of one 300-row rest mesh; the last object's rest range ends at nrest and its scene range at n = 3001
INSTANCES = [(0, 25, 300), (0, 1305, 300), (0, 2000, 300), (100, 2801, 200)]


def rt_view():
    return mirt.make_view(RT_CAM, mirt.rot_from_yaw(0.1, 1.0), H / 2.0, W, H)


def ras_view():
    return mirt.make_view(RAS_CAM, mirt.rot_from_yaw(0.0, 1.01), float(H), W, H)


def query_inputs():
    rng = np.random.default_rng(5)
    target = rng.uniform(-1, 1, (512, 3)).astype(F)
    start = np.array(RT_CAM, F) + rng.uniform(-0.25, 0.25, (512, 3)).astype(F)
    dirs = rng.uniform(-1, 1, (768, 3)).astype(F)
    return mirt.make_rays(start, (target - start).astype(F)), np.ascontiguousarray(dirs)


RAYS, DIRS = query_inputs()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


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
    # (bit for bit where the yardstick holds a number: which NaN an invalid operation makes -- its sign, its payload -- is the
    # processor's choice, and the mirror was computed on the host)
    nan = np.isnan(want["tris"])
    assert np.array_equal(np.isnan(got["tris"]), nan), "%s: the NaNs of the triangles read back" % what
    assert np.array_equal(bits(got["tris"])[~nan], bits(want["tris"])[~nan]), "%s: the triangles read back differ in %d words" % (
        what, int((bits(got["tris"])[~nan] != bits(want["tris"])[~nan]).sum()))
    for mode in (mirt.RT_BRUTE, mirt.RT_BINNED):
        assert got["rt%d_mode" % mode] == want["rt%d_mode" % mode], what
        for k in RT_KEYS:
            assert np.array_equal(bits(got["rt%d" % mode][k]), bits(want["rt%d" % mode][k])), "%s: ray-traced %s, mode %d" % (what, k, mode)
    for k in RAS_KEYS:
        assert np.array_equal(bits(got["ras"][k]), bits(want["ras"][k])), "%s: rasterised %s" % (what, k)
    assert got["q_modes"] == want["q_modes"], what
    for k in ("hits", "lit", "fan"):
        assert got["q"][k].tobytes() == want["q"][k].tobytes(), "%s: query %s" % (what, k)


_host_snapshots = {}


def host_snapshot(tris):
    """Everything after mirt_scene_upload of the array: once per array, shared, never changed.  (The upload forgets the declared
    objects: the tests take their yardsticks before they declare any.)"""
    key = tris.tobytes()
    if key not in _host_snapshots:
        mirt.scene_upload(tris)
        _host_snapshots[key] = snapshot()
    return _host_snapshots[key]


def assert_is_binned(snap):
    assert snap["rt%d_mode" % mirt.RT_BINNED] == mirt.RT_BINNED and snap["q_modes"] == (mirt.QUERY_BINNED, mirt.QUERY_BINNED)


def binned_frame():
    f = mirt.raytrace(rt_view(), DEFAULT_LIGHT, mode=mirt.RT_BINNED, want_intersection=True)
    assert f["stats"]["mode_used"] == mirt.RT_BINNED
    return f


# ---- 1. snapshot objects --------------------------------------------------------------------------------------------------------

def test_snapshot_objects_of_every_size():
    tris = scene(3001)
    objects = [(sf, sf, cnt) for sf, cnt in SIZES]
    mirror = mirt.pose(None, objects, XFORMS, tris)
    assert not np.array_equal(bits(mirror[1001:1514]), bits(tris[1001:1514]))
    want = host_snapshot(mirror)
    assert_is_binned(want)
    assert want["finite"] == 1
    mirt.scene_upload(tris)
    v0 = mirt.scene_info()["version"]
    mirt.scene_set_objects(objects)
    mirt.scene_pose(XFORMS)
    assert mirt.scene_info()["version"] != v0
    assert_same_snapshot(snapshot(), want, "snapshot objects")
    # the snapshot is the rest pose from now on: the same pose again changes nothing, whatever the live rows hold
    mirt.scene_pose(XFORMS)
    assert np.array_equal(bits(mirt.scene_download()), bits(mirror))


# ---- 2. instancing --------------------------------------------------------------------------------------------------------------

def test_instances_of_a_host_rest_mesh():
    tris, rest = scene(3001), mirt.scene_soup(21, 300, 0.25)
    mirror = mirt.pose(rest, INSTANCES, XFORMS[:4], tris)
    want = host_snapshot(mirror)
    assert_is_binned(want)
    mirt.scene_upload(tris)
    mirt.scene_set_objects(INSTANCES, rest)
    mirt.scene_pose(XFORMS[:4])
    got = snapshot()
    assert np.array_equal(bits(got["tris"][2801:]), bits(mirt.transform(rest[100:], XFORMS[3][:9], XFORMS[3][9:])))
    assert_same_snapshot(got, want, "instances")


# ---- 3. subsets, and what is not listed -----------------------------------------------------------------------------------------

def test_a_subset_and_what_persists():
    tris, rest = scene(3001), mirt.scene_soup(21, 300, 0.25)
    first = mirt.pose(rest, INSTANCES, XFORMS[:2], tris, which=[2, 0])
    mirror = mirt.pose(rest, INSTANCES, XFORMS[2:3], first, which=[1])
    want_first, want = host_snapshot(first), host_snapshot(mirror)
    mirt.scene_upload(tris)
    mirt.scene_set_objects(INSTANCES, rest)
    mirt.scene_pose(XFORMS[:2], which=[2, 0])
    got = mirt.scene_download()
    assert np.array_equal(bits(got), bits(first))
    assert np.array_equal(bits(got[1305:1605]), bits(tris[1305:1605])) and np.array_equal(bits(got[2801:]), bits(tris[2801:]))   # not listed
    assert_same_snapshot(snapshot(), want_first, "objects 2 and 0")
    mirt.scene_pose(XFORMS[2:3], which=[1])
    got = snapshot()
    assert_same_snapshot(got, want, "then object 1")         # objects 2 and 0 keep their last pose
    no_object = np.ones(3001, bool)
    for _, sf, cnt in INSTANCES:
        no_object[sf:sf + cnt] = False
    assert no_object.sum() == 3001 - 1100 and np.array_equal(bits(got["tris"][no_object]), bits(tris[no_object]))


# ---- 4. never cumulative --------------------------------------------------------------------------------------------------------

def test_pose_is_not_cumulative():
    tris = scene(3001)
    objects = [(sf, sf, cnt) for sf, cnt in SIZES]
    a, b = XFORMS, XFORMS[::-1]
    want = host_snapshot(mirt.pose(None, objects, b, tris))
    mirt.scene_upload(tris)
    mirt.scene_set_objects(objects)
    v0 = mirt.scene_info()["version"]
    mirt.scene_pose(a)
    v1 = mirt.scene_info()["version"]
    assert not np.array_equal(bits(mirt.scene_download()), bits(want["tris"]))
    mirt.scene_pose(b)
    v2 = mirt.scene_info()["version"]
    assert v1 != v0 and v2 != v1 and v2 != v0
    assert_same_snapshot(snapshot(), want, "pose A, then pose B")


# ---- 5. nothing stale survives --------------------------------------------------------------------------------------------------

def test_nothing_stale_survives_a_pose():
    tris, rest = scene(3001), mirt.scene_soup(21, 300, 0.25)
    mirror = mirt.pose(rest, INSTANCES, XFORMS[:4], tris)
    want, old = host_snapshot(mirror), host_snapshot(tris)
    assert not np.array_equal(want["rt%d" % mirt.RT_BINNED]["index"], old["rt%d" % mirt.RT_BINNED]["index"]), "the pose does not change the picture"
    mirt.set_frames_in_flight(1)
    mirt.scene_upload(tris)
    mirt.scene_set_objects(INSTANCES, rest)
    binned_frame()
    assert binned_frame()["stats"]["bins_reused"] == 1        # a standing view keeps its pass
    queries(mirt.QUERY_BINNED)
    _, qs, fs = queries(mirt.QUERY_BINNED)
    assert qs["cube_source"] == 2 and fs["cube_source"] == 2  # ... and the queries their cubes
    mirt.scene_pose(XFORMS[:4])
    f = binned_frame()
    assert f["stats"]["bins_reused"] == 0
    for k in RT_KEYS:
        assert np.array_equal(bits(f[k]), bits(want["rt%d" % mirt.RT_BINNED][k])), k
    got, qs, fs = queries(mirt.QUERY_BINNED)
    assert qs["mode_used"] == mirt.QUERY_BINNED and fs["mode_used"] == mirt.QUERY_BINNED
    assert qs["cube_source"] == 1 and fs["cube_source"] == 1  # built again, for the new scene
    for k in ("hits", "lit", "fan"):
        assert got[k].tobytes() == want["q"][k].tobytes(), k
    assert binned_frame()["stats"]["bins_reused"] == 1


# ---- 6. bounds and finiteness follow the data both ways -------------------------------------------------------------------------

def test_bounds_follow_the_data():
    tris = scene(3001)
    objects = [(1001, 1001, 513), (27, 27, 255)]
    out, far = xform(0.0, 1.0, (5.0, 0.0, 0.0)), xform(0.0, 1.0, (1.0e9, 0.0, 0.0))
    mirrors = [mirt.pose(None, objects, [x], tris) for x in (out, IDENTITY, far)]
    wants = [host_snapshot(m) for m in mirrors]
    box0 = host_snapshot(tris)
    assert wants[0]["hi"][0] > box0["hi"][0] + 3.0 and wants[0]["finite"] == 1
    assert np.array_equal(wants[1]["lo"], box0["lo"]) and np.array_equal(wants[1]["hi"], box0["hi"])
    assert wants[2]["finite"] == 0 and wants[2]["rt%d_mode" % mirt.RT_BINNED] == mirt.RT_BRUTE
    mirt.scene_upload(tris)
    mirt.scene_set_objects(objects)
    for x, want, what in zip((out, IDENTITY, far, IDENTITY), wants + wants[1:2], ("outwards", "back", "1e9 away", "back again")):
        mirt.scene_pose([x])                                  # object 0 alone
        assert_same_snapshot(snapshot(), want, what)          # the box grows, shrinks; a scene that is not finite takes the brute path


def test_a_rest_row_that_is_not_a_number():
    tris, rest = scene(3001), np.array(mirt.scene_soup(21, 300, 0.25))
    rest[7, 4] = F("nan")                                     # v1.y of one rest row
    mirror = mirt.pose(rest, INSTANCES, XFORMS[:4], tris)
    want = host_snapshot(mirror)
    assert want["finite"] == 0 and np.isnan(mirror[32, 3:6]).all() and np.isfinite(want["lo"]).all() and np.isfinite(want["hi"]).all()
    mirt.scene_upload(tris)
    mirt.scene_set_objects(INSTANCES, rest)
    mirt.scene_pose(XFORMS[:4])
    assert_same_snapshot(snapshot(), want, "a NaN vertex in the rest pose")


# ---- 7. what set_objects does and does not do -----------------------------------------------------------------------------------

def test_set_objects_invalidates_nothing_and_an_upload_forgets():
    lib = mirt.load()
    tris, rest = scene(3001), mirt.scene_soup(21, 300, 0.25)
    x = np.ascontiguousarray(XFORMS[:4])
    xp = x.ctypes.data_as(C.c_void_p)
    mirror = mirt.pose(rest, INSTANCES, x, tris)
    want = host_snapshot(mirror)
    mirt.set_frames_in_flight(1)
    mirt.scene_upload(tris)
    binned_frame()
    queries(mirt.QUERY_BINNED)
    v0 = mirt.scene_info()["version"]
    mirt.scene_set_objects([(sf, sf, cnt) for sf, cnt in SIZES])          # a snapshot
    mirt.scene_set_objects(INSTANCES, rest)                              # ... replaced by a host rest pose
    assert mirt.scene_info()["version"] == v0
    assert binned_frame()["stats"]["bins_reused"] == 1
    _, qs, fs = queries(mirt.QUERY_BINNED)
    assert qs["cube_source"] == 2 and fs["cube_source"] == 2
    assert np.array_equal(bits(mirt.scene_download()), bits(tris))
    # no objects: nothing to pose
    mirt.scene_set_objects([])
    assert lib.mirt_scene_pose(None, 1, xp) == INVALID and b"no objects" in lib.mirt_last_error()
    # an upload forgets them, either form
    mirt.scene_set_objects(INSTANCES, rest)
    assert lib.mirt_scene_pose(None, 0, xp) == 0
    mirt.scene_upload(tris)
    assert lib.mirt_scene_pose(None, 1, xp) == INVALID and b"no objects" in lib.mirt_last_error()
    assert mirt.scene_info()["version"] != v0 and np.array_equal(bits(mirt.scene_download()), bits(tris))
    # an update changes live rows only: the next pose of the object restores the rows derived from the rest pose
    mirt.scene_set_objects(INSTANCES, rest)
    mirt.scene_pose(x)
    mirt.scene_update(1305, scene(3001, seed=13)[1305:1605])
    mirt.scene_transform(2000, 300, XFORMS[5][:9], XFORMS[5][9:])
    assert not np.array_equal(bits(mirt.scene_download()), bits(mirror))
    mirt.scene_pose(x[1:3], which=[1, 2])
    assert_same_snapshot(snapshot(), want, "posed again after an update and a transform")


def test_device_upload_forgets_the_objects():
    lib = mirt.load()
    tris = scene(65)
    x = np.ascontiguousarray(XFORMS[:1])
    mirt.scene_upload(tris)
    mirt.scene_set_objects([(0, 0, 65)])
    with DeviceArray((65 * 15,), F) as d:
        mirt.scene_upload_device(d.ptr, 65)
    assert lib.mirt_scene_pose(None, 1, x.ctypes.data_as(C.c_void_p)) == INVALID and b"no objects" in lib.mirt_last_error()


# ---- 8. frames in flight --------------------------------------------------------------------------------------------------------

def test_frames_in_flight_finish_on_the_old_scene():
    tris, rest = scene(3001), mirt.scene_soup(21, 300, 0.25)
    mirror = mirt.pose(rest, INSTANCES, XFORMS[:4], tris)
    old_ref, new_ref = host_snapshot(tris)["rt%d" % mirt.RT_BINNED]["xrgb"], host_snapshot(mirror)["rt%d" % mirt.RT_BINNED]["xrgb"]
    assert not np.array_equal(old_ref, new_ref)
    planes = [DeviceArray((H, W), np.uint32, 0) for _ in range(5)]
    try:
        mirt.scene_upload(tris)
        mirt.scene_set_objects(INSTANCES, rest)
        mirt.set_frames_in_flight(4)
        view = rt_view()
        for p in planes[:4]:
            mirt.raytrace_device(view, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, p.ptr, W * 4)
        mirt.scene_pose(XFORMS[:4])                           # no mirt_sync in between
        mirt.raytrace_device(view, DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, planes[4].ptr, W * 4)
        mirt.sync()
        for i, p in enumerate(planes):
            want = old_ref if i < 4 else new_ref
            assert np.array_equal(p.read()[1:-1, 1:-1], want[1:-1, 1:-1]), "frame %d" % i
    finally:
        mirt.set_frames_in_flight(1)
        for p in planes:
            p.free()


# ---- 9. small scenes ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which_object", ["whole", "last"])
@pytest.mark.parametrize("n", [30, 65])
def test_small_scenes(n, which_object):
    tris = scene(n)
    objects = [(0, 0, n)] if which_object == "whole" else [(n - 1, n - 1, 1)]
    x = xform(0.3, 1.0, (0.125, -0.125, 0.25))
    mirror = mirt.pose(None, objects, [x], tris)
    want = host_snapshot(mirror)
    mirt.scene_upload(tris)
    mirt.scene_set_objects(objects)
    mirt.scene_pose([x])
    assert_same_snapshot(snapshot(), want, "n = %d, %s" % (n, which_object))


# ---- 10. arguments --------------------------------------------------------------------------------------------------------------

def test_arguments():
    lib = mirt.load()
    n, nrest = 65, 10
    tris, rest = scene(n), mirt.scene_soup(2, nrest, 0.2)
    x = np.ascontiguousarray(XFORMS[:3])
    xp, rp = x.ctypes.data_as(C.c_void_p), rest.ctypes.data_as(C.c_void_p)

    def set_objects(objects, rest_p=rp, nrest=nrest, nobjects=None):
        o = None if objects is None else np.ascontiguousarray(objects, np.int32).reshape(-1, 3)
        return lib.mirt_scene_set_objects(None if o is None else o.ctypes.data_as(C.c_void_p), len(o) if nobjects is None else nobjects, rest_p, nrest)

    def pose(which, count, x_p=xp):
        w = None if which is None else np.ascontiguousarray(which, np.int32)
        return lib.mirt_scene_pose(None if w is None else w.ctypes.data_as(C.c_void_p), count, x_p)

    good = [[0, 0, 10], [0, 10, 10], [5, 60, 5]]
    mirt.scene_upload(tris)
    v0 = mirt.scene_info()["version"]
    # set_objects: the arrays ...
    assert set_objects(good, nobjects=-1) == INVALID and set_objects(good, nrest=-1) == INVALID
    assert set_objects(None, nobjects=3) == INVALID and set_objects(good, rest_p=None) == INVALID
    for off in (1, 2, 3):
        assert set_objects(good, rest_p=C.c_void_p(rest.ctypes.data + off)) == INVALID
    assert b"aligned" in lib.mirt_last_error()
    # ... then the list: a negative field, a rest range, a scene range, an overlap
    for objects in ([[0, -1, 1]], [[-1, 0, 1]], [[0, 0, -1]], [[0, 0, 11]], [[10, 0, 1]], [[0, 56, 10]], [[0, 65, 1]], [[0, 0, 10], [0, 9, 10]],
                    [[0, 9, 10], [0, 0, 10]], [[2 ** 31 - 1, 0, 2 ** 31 - 1]], [[0, 2 ** 31 - 1, 2 ** 31 - 1]]):
        assert set_objects(objects) == INVALID, objects
    assert set_objects([[60, 0, 6]], rest_p=None, nrest=0) == INVALID     # the snapshot's rest range is checked against n
    assert pose(None, 1) == INVALID and b"no objects" in lib.mirt_last_error()   # nothing above declared anything
    assert set_objects([[60, 0, 5], [0, 5, 60], [3, 65, 0]], rest_p=None, nrest=0) == 0
    assert set_objects(good) == 0
    # pose: the arguments, then the list
    assert pose(None, -1) == INVALID and pose(None, 1, None) == INVALID and pose([0], 1, None) == INVALID
    assert pose(None, 4) == INVALID
    for which in ([0, 1, 3], [0, -1, 2], [2, 0, 2], [1, 1, 1]):
        assert pose(which, 3) == INVALID, which
    assert pose(None, 0) == 0 and pose(None, 0, None) == 0 and pose([2], 0) == 0      # count == 0 does nothing
    assert set_objects([[0, 0, 0], [3, 65, 0]]) == 0 and pose(None, 2) == 0             # ... and so do objects without rows
    assert mirt.scene_info()["version"] == v0 and np.array_equal(bits(mirt.scene_download()), bits(tris))
    # a valid call for contrast
    assert set_objects(good) == 0 and pose([2, 0], 2) == 0 and mirt.scene_info()["version"] != v0
    assert np.array_equal(bits(mirt.scene_download()), bits(mirt.pose(rest, good, x[:2], tris, which=[2, 0])))
    # before any scene: what is wrong without a scene too comes first
    mirt.shutdown()
    mirt.init(0)
    assert set_objects(good) == NO_SCENE and set_objects([], rest_p=None, nrest=0) == NO_SCENE and pose(None, 1) == NO_SCENE
    assert b"no scene uploaded" in lib.mirt_last_error()
    assert set_objects(good, nobjects=-1) == INVALID and set_objects(good, rest_p=None) == INVALID
    assert pose(None, -1) == INVALID and pose(None, 1, None) == INVALID
