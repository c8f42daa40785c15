#!/usr/bin/env python3
"""tools/many_lights_bench.py [--out profiles/many_lights_bench.txt] [--steps query,frames] [--append] [--baseline-pkg DIR]

What soft shadows past 32 light positions cost (query/light_passes.hpp, lights/many_lights.hip), written to one text file.  Every
figure is a median of 15 runs, host clock around call + mirt_sync, after a warm-up call of the same shape.

  query    mirt_direct_light_device with 4 x 16 = 64 positions over the closest hits of soup100k's 1080p primary rays, BINNED, every
           cube held (two passes, the carry between them), beside the two 32-position calls that make up the same shadow work on the
           single-pass kernels (positions 0 .. 31 and 32 .. 63, each with its cube held), in the same process; and a device-to-device
           copy of the carry's size, which prices the 48 bytes per record the two passes add (24 stored by the first, 24 loaded by
           the second).  The two-call route does not compute the same colours (it has no carry); it is the same rays through the same bins.
  frames   a 2 x 16 = 32-position frame on cornell1080 and soup100k through the fused kernels and, in a process started with
           MIRT_MANY_LIGHTS_MIN=1, through the deferred path -- the price of deferral against kernels it leaves unchanged; then
           48-position and 256-position frames on both scenes with every cube held and with every cube rebuilt (all positions move
           between frames).  MIRT_RT_AUTO throughout.
  memory   (inside the two steps) device memory taken by one kept 32-position cube at 100 000 triangles and by a stream's
           deferred-frame scratch at 1080p: hipMemGetInfo around the first calls that need them.

  aa       (--steps aa, usually with --append) supersampled frames past 32 positions, each carried record shaded once
           (lights/aa_many_lights.hip): cornell1080 and soup100k at 1080p, 3 x 16 = 48 positions, 3 samples, cubes held and every
           position moved; beside each, 9 x the plain deferred frame of the same positions (the cost of shading every sub-ray),
           hit_subrays / records_shaded of mirt_get_supersample_stats, and what the fill and DirectLight over a list of records that
           were never appended cost (a memset of the lists' bytes; mirt_direct_light_device over a chunk's capacity of index -1
           records).  Then 2 x 16 = 32 positions, 3 samples: the fused frame, and the new path under MIRT_AA_DEFER_MIN=1.  The
           plain deferred and the fused frames run from --baseline-pkg (a build of the commit to compare against; default: this tree).

The knob is read once per process, so every GPU step is a child process of its own, under its own `timeout`; a step that fails ends
the run."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("MIRT_BENCH_PKG") or os.path.join(ROOT, "cpp-raytracer-rasterizer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ray_query_bench import CAM, FOCAL, H, W, closest_records, dev_alloc, hip, timed   # noqa: E402

REPS = 15
INDIRECT = (0.2, 0.2, 0.2)


def lights_of(n):
    rng = np.random.default_rng(11)
    L = np.zeros((n, 7), np.float32)
    L[:, 0:3] = np.round(rng.uniform(-0.75, 0.75, (n, 3)) * 64) / 64
    L[:, 2] = -np.abs(L[:, 2]) - 0.25                        # in front of the scenes' centre, like the reference's light
    L[:, 3:6] = 1.0
    L[:, 6] = 14.0
    return L


def jitter_of(L, samples, seed=3):
    rng = np.random.default_rng(seed)
    return (np.repeat(L[:, 0:3], samples, axis=0) + rng.uniform(-0.05, 0.05, (len(L) * samples, 3))).astype(np.float32)


def free_bytes(h):
    free, total = C.c_size_t(), C.c_size_t()
    assert h.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def child_query():
    import mirt
    h = hip()
    mirt.init(0)
    d_hits, count = closest_records(mirt, h, 100000, 0.05)
    d_rgb = dev_alloc(h, count * 12)
    L = lights_of(4)
    jit = jitter_of(L, 16)
    mirt.set_query_mode(mirt.QUERY_BINNED)

    def call(lights, positions):
        mirt.set_soft_shadows(16, positions)
        return lambda: mirt.direct_light_device(d_hits, count, lights, d_rgb)

    def held(lights, positions, want_source=2):
        fn = call(lights, positions)
        fn(); mirt.sync()                                    # builds what is missing
        ms = timed(mirt, fn, REPS)
        st = mirt.query_stats()
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == want_source, st
        return ms, st
    before = free_bytes(h)
    first, _ = held(L[:2], jit[:32])
    cube_bytes = before - free_bytes(h)
    second, _ = held(L[2:], jit[32:])
    both, st = held(L, jit)
    first2, _ = held(L[:2], jit[:32])
    second2, _ = held(L[2:], jit[32:])
    both2, _ = held(L, jit)
    # the carry's traffic at the copy rate: 24 bytes per record stored and 24 loaded
    d_a, d_b = dev_alloc(h, count * 24), dev_alloc(h, count * 24)
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def copy():
        assert h.hipMemcpy(d_b, d_a, count * 24, 3) == 0
        assert h.hipDeviceSynchronize() == 0
    copy()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        copy()
        ts.append((time.perf_counter() - t0) * 1e3)
    copy_ms = float(np.median(ts))
    print("RESULT records %d (closest hits of soup100k's primary rays at 1080p), 100000 triangles, BINNED, cubes held, medians of %d" % (count, REPS))
    print("RESULT one call, 4 x 16 = 64 positions in two passes: %.3f ms (again after the two-call runs: %.3f ms); cube grid %d, %d shells"
          % (both, both2, st["cube_bins"], st["shells"]))
    print("RESULT two calls, positions 0..31: %.3f ms + positions 32..63: %.3f ms = %.3f ms (again: %.3f + %.3f = %.3f ms)"
          % (first, second, first + second, first2, second2, first2 + second2))
    print("RESULT device-to-device copy of %d x 24 bytes (reads and writes as much as the carry's store plus its load): %.3f ms" % (count, copy_ms))
    gap = min(both, both2) - min(first + second, first2 + second2)
    print("RESULT one call - two calls = %+.3f ms; allowed: the copy's %.3f ms + 2 %% of the two calls (%.3f ms) = %.3f ms"
          % (gap, copy_ms, 0.02 * (first + second), copy_ms + 0.02 * (first + second)))
    print("RESULT memory: the first 32-position binned call took %.1f MiB of device memory (its kept cube and the stream's build scratch)" % (cube_bytes / 2.0 ** 20))
    mirt.shutdown()


def child_frames(scene):
    import mirt
    h = hip()
    mirt.init(0)
    forced = os.environ.get("MIRT_MANY_LIGHTS_MIN") is not None
    mirt.scene_upload(mirt.scene_cornell() if scene == "cornell1080" else mirt.scene_soup(1, 100000, 0.05))
    view = mirt.make_view(CAM, mirt.rot_from_yaw(0.0, 1.0), FOCAL, W, H)
    d_x = dev_alloc(h, W * H * 4)
    L = lights_of(16)

    def frame(nl):
        return lambda: mirt.raytrace_device(view, L[:nl], INDIRECT, mirt.RT_AUTO, 0, H, 0, d_x, W * 4)
    for nl in ((2,) if forced else (2, 3, 16)):
        jit = jitter_of(L[:nl], 16)
        mirt.set_soft_shadows(16, jit)
        before = free_bytes(h)
        frame(nl)(); mirt.sync(); frame(nl)(); mirt.sync()   # (cubes settle, scratch is there)
        taken = before - free_bytes(h)
        ms = timed(mirt, frame(nl), REPS)
        mode = mirt.stats()["mode_used"]
        path = "deferred" if (forced or nl * 16 > 32) else "fused"
        print("RESULT %-11s %3d positions  %-8s primary mode %d  cubes held: %8.3f ms" % (scene, nl * 16, path, mode, ms))
        if path == "deferred" and not forced:
            if nl == 3:
                print("RESULT %-11s first deferred frames took %.1f MiB of device memory (stream scratch at 1080p, and the cubes)" % (scene, taken / 2.0 ** 20))
            ts = []
            for rep in range(REPS + 1):
                mirt.set_soft_shadows(16, (jit + np.float32(2.0 ** -12) * (rep + 1)).astype(np.float32))
                t0 = time.perf_counter()
                frame(nl)(); mirt.sync()
                ts.append((time.perf_counter() - t0) * 1e3)
            print("RESULT %-11s %3d positions  %-8s every position moved each frame: %8.3f ms" % (scene, nl * 16, path, float(np.median(ts[1:]))))
        sys.stdout.flush()
    mirt.shutdown()


AA = 3
AA_BYTES_PER_PIXEL = AA * AA * (20 + 12 + 24 + 8) + 4        # capi/aa_plan.hpp


def scene_tris(mirt, scene):
    return mirt.scene_cornell() if scene == "cornell1080" else mirt.scene_soup(1, 100000, 0.05)


def child_aa_baseline(scene):
    """The frames this work is compared against, on whatever package MIRT_BENCH_PKG names: the plain deferred frame of 48 positions
    (x 9 = shading every sub-ray of a 3 x 3 frame) and the fused 32-position frame at 3 samples."""
    import mirt
    h = hip()
    mirt.init(0)
    mirt.scene_upload(scene_tris(mirt, scene))
    view = mirt.make_view(CAM, mirt.rot_from_yaw(0.0, 1.0), FOCAL, W, H)
    d_x = dev_alloc(h, W * H * 4)
    L = lights_of(16)

    def frame(nl):
        return lambda: mirt.raytrace_device(view, L[:nl], INDIRECT, mirt.RT_AUTO, 0, H, 0, d_x, W * 4)
    jit = jitter_of(L[:3], 16)
    mirt.set_soft_shadows(16, jit)
    frame(3)(); mirt.sync(); frame(3)(); mirt.sync()
    held = timed(mirt, frame(3), REPS)
    ts = []
    for rep in range(REPS + 1):
        mirt.set_soft_shadows(16, (jit + np.float32(2.0 ** -12) * (rep + 1)).astype(np.float32))
        t0 = time.perf_counter()
        frame(3)(); mirt.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    moved = float(np.median(ts[1:]))
    print("RESULT %-11s  48 positions, no supersampling, plain deferred: cubes held %8.3f ms (x %d = %9.3f ms); every position moved %8.3f ms (x %d = %9.3f ms)"
          % (scene, held, AA * AA, held * AA * AA, moved, AA * AA, moved * AA * AA))
    mirt.set_soft_shadows(16, jitter_of(L[:2], 16))
    mirt.set_antialiasing(AA)
    frame(2)(); mirt.sync(); frame(2)(); mirt.sync()
    print("RESULT %-11s  32 positions, %d samples, fused kernels: %8.3f ms" % (scene, AA, timed(mirt, frame(2), REPS)))
    mirt.shutdown()


def child_aa(scene):
    import mirt
    h = hip()
    mirt.init(0)
    forced = os.environ.get("MIRT_AA_DEFER_MIN") is not None
    mirt.scene_upload(scene_tris(mirt, scene))
    view = mirt.make_view(CAM, mirt.rot_from_yaw(0.0, 1.0), FOCAL, W, H)
    d_x = dev_alloc(h, W * H * 4)
    L = lights_of(16)
    mirt.set_supersampled_many_lights(True)
    mirt.set_antialiasing(AA)

    def frame(nl):
        return lambda: mirt.raytrace_device(view, L[:nl], INDIRECT, mirt.RT_AUTO, 0, H, 0, d_x, W * 4)
    if forced:
        mirt.set_soft_shadows(16, jitter_of(L[:2], 16))
        frame(2)(); mirt.sync(); frame(2)(); mirt.sync()
        ms = timed(mirt, frame(2), REPS)
        s = mirt.supersample_stats()
        print("RESULT %-11s  32 positions, %d samples, each record once (MIRT_AA_DEFER_MIN=1): %8.3f ms; hit sub-rays / records shaded = %d / %d = %.2f"
              % (scene, AA, ms, s["hit_subrays"], s["records_shaded"], s["hit_subrays"] / max(s["records_shaded"], 1)))
        mirt.shutdown()
        return
    jit = jitter_of(L[:3], 16)
    mirt.set_soft_shadows(16, jit)
    before = free_bytes(h)
    frame(3)(); mirt.sync(); frame(3)(); mirt.sync()
    taken = before - free_bytes(h)
    held = timed(mirt, frame(3), REPS)
    st, s = mirt.stats(), mirt.supersample_stats()
    ts = []
    for rep in range(REPS + 1):
        mirt.set_soft_shadows(16, (jit + np.float32(2.0 ** -12) * (rep + 1)).astype(np.float32))
        t0 = time.perf_counter()
        frame(3)(); mirt.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    moved = float(np.median(ts[1:]))
    print("RESULT %-11s  48 positions, %d samples, each record once, primary mode %d: cubes held %8.3f ms; every position moved %8.3f ms"
          % (scene, AA, st["mode_used"], held, moved))
    print("RESULT %-11s  hit sub-rays / records shaded = %d / %d = %.2f; the first frames took %.1f MiB of device memory (stream scratch, and the cubes)"
          % (scene, s["hit_subrays"], s["records_shaded"], s["hit_subrays"] / max(s["records_shaded"], 1), taken / 2.0 ** 20))
    # the fill, and DirectLight over records that were never appended: the chunks of the frame (capi/aa_plan.hpp, the default budget)
    rows = max(1, min(H, (256 << 20) // (W * AA_BYTES_PER_PIXEL)))
    chunks = (H + rows - 1) // rows
    cap = W * rows * AA * AA
    d_rec, d_rgb = dev_alloc(h, cap * 20), dev_alloc(h, cap * 12)
    h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]

    def fill():
        assert h.hipMemset(d_rec, 0xFF, cap * 20) == 0
        assert h.hipDeviceSynchronize() == 0
    fill()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fill()
        ts.append((time.perf_counter() - t0) * 1e3)
    fill_ms = float(np.median(ts)) * W * H * AA * AA / cap      # (the frame's lists together)
    mirt.set_soft_shadows(16, jit)
    mirt.set_query_mode(mirt.QUERY_BINNED if scene != "cornell1080" else mirt.QUERY_BRUTE)   # (what the frame's AUTO rule chooses for its passes)
    empty = lambda: mirt.direct_light_device(d_rec, cap, L[:3], d_rgb)
    empty(); mirt.sync()
    empty_ms = timed(mirt, empty, REPS) * W * H * AA * AA / cap
    unappended = 1.0 - s["records_shaded"] / float(W * H * AA * AA)
    print("RESULT %-11s  %d chunks of %d rows; filling the lists: %.3f ms; DirectLight over lists of index -1 records only: %.3f ms, of which the "
          "unappended share %.2f is %.3f ms: together %.1f %% of the frame with cubes held"
          % (scene, chunks, rows, fill_ms, empty_ms, unappended, empty_ms * unappended, 100.0 * (fill_ms + empty_ms * unappended) / held))
    mirt.shutdown()


def run_child(p, args, env, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True)
    for line in r.stdout.split("\n"):
        if line.startswith("RESULT "):
            p(line[7:])
    if r.returncode != 0:
        p("step %s failed with status %d" % (" ".join(args), r.returncode))
        sys.stderr.write(r.stderr[-4000:])
        sys.exit(1)                      # nothing more is started on the GPU
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "many_lights_bench.txt"))
    ap.add_argument("--steps", default="query,frames")
    ap.add_argument("--append", action="store_true", help="add the steps' sections to --out instead of rewriting it")
    ap.add_argument("--baseline-pkg", default=None, help="package directory the aa step's baseline frames run from (default: this tree's)")
    ap.add_argument("--child", nargs="+")
    a = ap.parse_args()
    if a.child:
        return {"query": child_query, "frames": lambda: child_frames(a.child[1]), "aa": lambda: child_aa(a.child[1]),
                "aa_baseline": lambda: child_aa_baseline(a.child[1])}[a.child[0]]()
    lines = []

    def p(s):
        print(s)
        sys.stdout.flush()
        lines.append(s)
    steps = a.steps.split(",")
    try:
        if "query" in steps:
            p("== query: one 64-position mirt_direct_light_device call in two passes beside two 32-position calls (and the kept cube's memory) ==")
            run_child(p, ["--child", "query"], {}, 300)
            p("")
        if "frames" in steps:
            p("== frames: 1920 x 1080, MIRT_RT_AUTO, 16 samples per light; bytes of stream scratch per pixel: 76 (DESIGN.md 5.1) ==")
            for scene in ("cornell1080", "soup100k"):
                run_child(p, ["--child", "frames", scene], {}, 300)
                p("with MIRT_MANY_LIGHTS_MIN=1:")
                run_child(p, ["--child", "frames", scene], {"MIRT_MANY_LIGHTS_MIN": "1"}, 300)
            p("")
        if "aa" in steps:
            p("== aa: 1920 x 1080, MIRT_RT_AUTO, 16 samples per light, 3 x 3 sub-rays: each carried record shaded once (lights/aa_many_lights.hip) ==")
            base_env = {"MIRT_BENCH_PKG": os.path.abspath(a.baseline_pkg)} if a.baseline_pkg else {}
            p("baseline frames from %s:" % (a.baseline_pkg or "this tree"))
            for scene in ("cornell1080", "soup100k"):
                run_child(p, ["--child", "aa_baseline", scene], base_env, 600)
            p("this tree:")
            for scene in ("cornell1080", "soup100k"):
                run_child(p, ["--child", "aa", scene], {}, 600)
                run_child(p, ["--child", "aa", scene], {"MIRT_AA_DEFER_MIN": "1"}, 600)
            p("")
    finally:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
