#!/usr/bin/env python3
"""tools/scene_update_bench.py [--out profiles/scene_update_bench.txt] [--reps 15] [--section all|pose]

What it costs to put triangles on the device and to change them there (capi/scene.cpp, scene/scene_kernels.hip): the median host time
around one call + mirt_sync, at n = 100 000 and n = 1 000 000 (soup100k's and soup1m8k's scenes), for

  mirt_scene_upload            the yardstick: pageable host memory, two host scans (its code is the parent's, measured in the same run)
  mirt_scene_upload_device     the same triangles from device memory
  mirt_scene_update_device     the full range, and 1 % of the scene
  mirt_scene_update            1 % of the scene from host memory (staged through the device)
  mirt_scene_transform         the full range, and 1 % of the scene
  loop                         "move 1 % of the scene, then one binned 1080p frame" against "re-upload everything, then the same frame"
  pose                         K in {1, 8, 32, 128} equal objects covering 1 % and 100 % of the scene, moved three ways: one
                               mirt_scene_pose of all K; K mirt_scene_transform calls on the same ranges (the yardstick: code the posed
                               scenes do not touch); K mirt_transform calls on the host, each followed by a mirt_scene_update of its range
                               (the drift-free route without a rest pose on the device).  Per cell the three medians, and (min .. max) of
                               the 15 runs

Every timed call is followed by mirt_scene_info as a check that the scene is the size it was; the scenes of both loops are read back
once and compared with mirt_transform on the host array, and the posed scene of every cell with mirt_pose on a host mirror.
--section pose measures the pose blocks alone and replaces them in the file, whose other lines stay as they are.  One process, one GPU; a step that fails ends the run."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cpp-raytracer-rasterizer_amd"))

import mirt  # noqa: E402

W, H, CAM, FOCAL = 1920, 1080, (0.0, 0.0, -2.0), 540.0
SCENES = (("soup100k", 1, 100000, 0.05), ("soup1m8k", 2, 1000000, 0.02))

_hip = None


def hip():
    global _hip
    if _hip is None:
        h = C.CDLL("libamdhip64.so")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipFree.argtypes = [C.c_void_p]
        _hip = h
    return _hip


def device_copy(arr):
    a = np.ascontiguousarray(arr)
    p = C.c_void_p()
    assert hip().hipMalloc(C.byref(p), max(a.nbytes, 16)) == 0
    assert hip().hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
    assert hip().hipDeviceSynchronize() == 0
    return p


def median_ms(call, reps, warm=2):
    """Median host milliseconds of call() + mirt_sync over `reps` runs after `warm` unmeasured ones."""
    ts = []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        call()
        mirt.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts[warm:]), min(ts[warm:])


def spread_ms(call, reps, warm=2):
    """(median, min, max) host milliseconds of call() + mirt_sync over `reps` runs after `warm` unmeasured ones."""
    ts = []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        call()
        mirt.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts[warm:]), min(ts[warm:]), max(ts[warm:])


POSE_K = (1, 8, 32, 128)


def pose_section(say, tris, n, reps):
    """One pose of K objects against K transform calls and against K host transforms + updates, K equal objects over 1 % and 100 %."""
    rot, tr = mirt.rot_from_yaw(0.001, 1.0), (0.0005, 0.0, 0.0)
    x12 = np.concatenate([rot, np.asarray(tr, np.float32)]).astype(np.float32)
    say("pose: K equal objects; median ms (min .. max) of one mirt_scene_pose | K x mirt_scene_transform | K x (mirt_transform on the host + mirt_scene_update)")
    for share, covered, first in (("1 %", max(n // 100, 1), n // 3), ("100 %", n, 0)):
        for K in POSE_K:
            per = covered // K
            objects = [(first + k * per, first + k * per, per if k < K - 1 else covered - per * (K - 1)) for k in range(K)]
            xforms = np.tile(x12, (K, 1))
            mirt.scene_upload(tris)
            mirt.scene_set_objects(objects)                   # a snapshot: the rest pose is the scene as uploaded
            posed = spread_ms(lambda: mirt.scene_pose(xforms), reps)
            got = mirt.scene_download(first, covered)
            want = mirt.pose(None, [(rf - first, sf - first, c) for rf, sf, c in objects], xforms, tris[first:first + covered])
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "device pose differs from mirt_pose"

            def transforms():
                for _, sf, c in objects:
                    mirt.scene_transform(sf, c, rot, tr)

            def host_updates():
                for _, sf, c in objects:
                    mirt.scene_update(sf, mirt.transform(tris[sf:sf + c], rot, tr))

            moved = spread_ms(transforms, reps)
            mirt.scene_upload(tris)
            updated = spread_ms(host_updates, reps)
            assert mirt.scene_info()["n"] == n
            say("%-5s K = %3d: pose %9.3f (%9.3f .. %9.3f) | transforms %9.3f (%9.3f .. %9.3f) | host + update %9.3f (%9.3f .. %9.3f)"
                % ((share, K) + posed + moved + updated))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_update_bench.txt"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--section", choices=("all", "pose"), default="all")
    args = ap.parse_args()
    lines, pose_lines = [], []

    def say(s="", to=None):
        print(s, flush=True)
        (lines if to is None else to).append(s)

    def say_pose(s=""):
        say(s, pose_lines)

    mirt.init(0)
    d_xrgb = C.c_void_p()
    assert hip().hipMalloc(C.byref(d_xrgb), W * H * 4) == 0
    view = mirt.make_view(CAM, mirt.rot_from_yaw(0.0, 1.0), FOCAL, W, H)
    frame = mirt.prepared_raytrace_device(view, mirt.DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_BINNED, 0, H, 0, d_xrgb, W * 4)
    rot, tr = mirt.rot_from_yaw(0.001, 1.0), (0.0005, 0.0, 0.0)
    say("median (min) host ms around call + mirt_sync, %d runs each; frame = one RT_BINNED %d x %d frame of the scene" % (args.reps, W, H))
    try:
        for name, seed, n, s in SCENES:
            tris = mirt.scene_soup(seed, n, s)
            part = max(n // 100, 1)
            first = n // 3
            d_tris = device_copy(tris)
            d_part = C.c_void_p(d_tris.value + 60 * first)
            if args.section == "all":
                say()
                say("== %s: n = %d (%.1f MB), 1 %% = %d triangles from %d ==" % (name, n, tris.nbytes / 1e6, part, first))
                rows = {}

                def step(label, call):
                    med, lo = median_ms(call, args.reps)
                    assert mirt.scene_info()["n"] == n
                    rows[label] = med
                    say("%-46s %9.3f ms  (min %9.3f)" % (label, med, lo))

                step("mirt_scene_upload (host, yardstick)", lambda: mirt.scene_upload(tris))
                step("mirt_scene_upload_device", lambda: mirt.scene_upload_device(d_tris, n))
                step("mirt_scene_update_device, full range", lambda: mirt.scene_update_device(0, n, d_tris))
                step("mirt_scene_update_device, 1 %", lambda: mirt.scene_update_device(first, part, d_part))
                step("mirt_scene_update (host), 1 %", lambda: mirt.scene_update(first, tris[first:first + part]))
                step("mirt_scene_transform, full range", lambda: mirt.scene_transform(0, n, rot, tr))
                mirt.scene_upload(tris)
                step("mirt_scene_transform, 1 %", lambda: mirt.scene_transform(first, part, rot, tr))
                # the device scene after the warm and timed calls == the host arithmetic applied as often
                want = tris[first:first + part]
                for _ in range(2 + args.reps):
                    want = mirt.transform(want, rot, tr)
                got = mirt.scene_download(first, part)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "device transform differs from mirt_transform"
                mirt.scene_upload(tris)
                frame()
                mirt.sync()
                step("frame alone (standing view)", frame)

                def moved_frame():
                    mirt.scene_transform(first, part, rot, tr)
                    frame()

                def reuploaded_frame():
                    mirt.scene_upload(tris)
                    frame()

                step("loop: transform 1 %, then the frame", moved_frame)
                step("loop: re-upload, then the frame", reuploaded_frame)
                say("device upload / host upload: %.3f;  1 %% transform + frame / re-upload + frame: %.3f" % (
                    rows["mirt_scene_upload_device"] / rows["mirt_scene_upload (host, yardstick)"],
                    rows["loop: transform 1 %, then the frame"] / rows["loop: re-upload, then the frame"]))
            say_pose()
            say_pose("== pose, %s: n = %d ==" % (name, n))
            pose_section(say_pose, tris, n, args.reps)
            assert hip().hipFree(d_tris) == 0
    finally:
        mirt.sync()
        hip().hipFree(d_xrgb)
        mirt.shutdown()
    if args.section == "pose" and os.path.exists(args.out):   # the file's other lines stay: everything in front of its pose blocks
        lines = []
        for line in open(args.out).read().split("\n"):
            if line.startswith("== pose"):
                break
            lines.append(line)
        while lines and not lines[-1]:
            lines.pop()
    with open(args.out, "w") as f:
        f.write("\n".join(lines + pose_lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
