#!/usr/bin/env python3
"""tools/ray_query_bench.py [--out profiles/ray_query_bench.txt] [--steps issue,occupancy,throughput,sweep,directlight,fan,fans,occluded,mask,along,alongs,grid,ordered,ordered_along,count]

The measurements of the ray-query kernels (query/rt_query.hip), written to one text file:

  issue + throughput   the lane-per-ray kernel over the 2 073 600 primary rays of soup100k at 1080p (generated on the host, through
                       mirt_intersect_device) beside one BRUTE frame of the same view in the same process (k_rt_brute).  The EXPECTED
                       ratio of the two comes from the code: the vector instructions every test executes -- from a row's LDS reads to
                       the filter's branch -- of either kernel, priced with the issue classes of tools/issue_mix.py.
  sweep                time against the number of rays, 1 .. 2^20 in powers of two, at n = 100 000 and n = 2 000, with
                       MIRT_QUERY_WAVE_RAYS = 0 (lane per ray) and huge (wave per ray): where the curves cross is the knob's default.
  occupancy            tools/check_spills.py's lines for the query kernels: VGPRs, scratch, waves per SIMD.
  directlight          mirt_direct_light_device over the closest-hit records of soup100k's primary rays at 1080p (mirt_intersect_device
                       of the view's rays) and the default light: MIRT_QUERY_BRUTE, MIRT_QUERY_BINNED with the cube built by the call
                       (the light moves by one ulp between the calls) and with the cube kept; every run's colours hashed and
                       compared.  Then the record count swept in powers of two at n = 100 000 and n = 2 000: the smallest call from
                       which binned-with-build stays ahead of brute force is where MIRT_QUERY_AUTO should switch.
  fan                  the primary rays of soup100k at 1080p as a fan from the camera: mirt_intersect_device on {camera, dir} rays (the
                       yardstick), mirt_intersect_from_device under MIRT_QUERY_BRUTE, under MIRT_QUERY_BINNED with the cube built by
                       the call (the origin moves by one ulp between the calls) and with the cube kept; all records of every run
                       hashed and compared.  Then the ray count swept in powers of two at n = 100 000 and n = 2 000 (rays of the
                       frame in a fixed shuffled order): the smallest call from which binned-with-build stays ahead of the fan's own
                       sweep is where MIRT_QUERY_AUTO should switch for fans (it starts from the frame path's 4e7, unmeasured).
  fans                 mirt_intersect_fans_device on soup100k and on the soup of 2000: K = 1, 4, 32, 128 origins inside the scene x 64,
                       4096, 65536 rays per origin (grouped by origin), under MIRT_QUERY_BINNED with every pass's cube built by the call
                       (origin 0 moves by one ulp between the calls), with the cube kept (K <= 32) and under MIRT_QUERY_BRUTE, beside
                       the yardstick: K consecutive mirt_intersect_from_device calls on the same rays.  One digest over all records of
                       every variant; where the one call is behind the K calls, and where AUTO's rule is behind brute force, is listed.
  occluded             mirt_occluded_device and mirt_occluded_fans_device (K = 1, 4, 32 origins; BRUTE, BINNED with the cubes built by
                       the call, BINNED with the cube held) over 1 .. 2^20 rays in powers of four at n = 100 000 and n = 2 000, without
                       limits (a ray stops at its first occluder) and with limits at half the closest distance (nothing stops a ray),
                       each beside what a caller had to do before for the same answer, in the same run: mirt_intersect_device /
                       mirt_intersect_fans_device from fresh records on the same rays.  The answers are compared first; the cells
                       where an occlusion call is behind, and where binning with the builds crosses the brute path, are listed.
  ordered              mirt_intersect_ordered_device, max_hits 1, 2, 4, 8, on the grid step's scenes and ray sets, 1 .. 2^20 rays in powers of
                       four, the switch of mirt_set_ray_grid off, on with the build and on with the structure held, beside
                       mirt_intersect_device from fresh records and beside max_hits in-place peels of the max_hits == 1 call, in the same
                       run on the same rays.  The answers are compared first; the cells where max_hits == 1 is behind mirt_intersect_device
                       and where max_hits == N is behind N peels are listed.
  ordered_along        mirt_intersect_ordered_along_device, max_hits 1, 2, 4, 8, on the along step's grid of starts looking down the soup of
                       2000 and of 100 000 triangles, 1 .. 2^20 rays in powers of four, with its build and with the grid held, beside
                       mirt_intersect_ordered_device on the same rays written out -- the switch of mirt_set_ray_grid off, and on with the
                       ray grid held -- and, for max_hits 1, beside mirt_intersect_along_device, in the same run.  The answers are compared
                       first; every cell is recorded and the cells where the new call is behind a yardstick by more than 2 % are listed.
  count                mirt_count_hits_along_device on the along step's grid of starts (BRUTE, BINNED with its build and with the grid held) and
                       mirt_count_hits_device on the grid step's ray sets, 1 .. 2^20 rays in powers of four at n = 100 000 and n = 2 000, without
                       `after` and limits, beside what a caller had to do before for the same numbers, in the same run: peels of
                       mirt_intersect_ordered_along_device / mirt_intersect_ordered_device at max_hits 8 through host memory until no ray is
                       full -- and beside ONE such call, and one mirt_occluded*_device call as the floor of a walk that may stop early.  The
                       answers are compared first; the cells where one count call is behind one max_hits 8 call are listed.
  mask                 mirt_shadow_mask_device and mirt_direct_light_masked_device beside mirt_direct_light_device on the same records, lights
                       and cubes, the three calls in turn: 2^10 .. 2^21 records x 1, 2, 32, 64, 256 positions x 2000 and 100 000
                       triangles, under MIRT_QUERY_BRUTE (cells beyond 2e11 row tests are named, not run) and MIRT_QUERY_BINNED with the
                       cubes held.  One cell measured seven times over gives the run-to-run spread; the cells where the mask call is
                       behind mirt_direct_light_device by more than that are listed, and for the masked call its ratio to
                       mirt_direct_light_device and the bytes it must move over its time as a share of the HBM peak.  Mask + relight
                       is compared with mirt_direct_light_device's colours in every cell.

  along                mirt_intersect_along_device and mirt_occluded_along_device for a square grid of starts looking down the scene
                       (an orthographic camera above it, dir = +z): 1 .. 2^20 rays in powers of four at n = 100 000 and n = 2 000, under
                       MIRT_QUERY_BINNED with the grid built by the call (the direction tilts by one subnormal between the calls) and
                       with the grid held, beside mirt_intersect_device / mirt_occluded_device from fresh records on the same rays
                       written out, in the same run.  The answers are compared first; the cells where the new call is behind are listed,
                       and from the rows the ray count from which the call with its build stays ahead: whether AUTO's starting rule
                       (the fans') is confirmed or moved.
  alongs               mirt_intersect_alongs_device and mirt_occluded_alongs_device for N points (the same grid of starts) x K = 1, 4, 15,
                       16, 32, 64 directions up to 35 degrees off +z, N = 64 .. 65 536 in powers of four, at n = 100 000 and n = 2 000, the
                       directions mixed within every wave: under MIRT_QUERY_BINNED with the groups built by the call (the list's bits
                       change between the calls) and with them held, beside two yardsticks on the same rays in the same run -- (a) K
                       mirt_*_along_device calls over the rays sorted by direction, what a caller does today, and (b)
                       mirt_intersect_device / mirt_occluded_device.  The answers are compared first; every cell is recorded, the cells
                       where the new call is behind either yardstick by more than 2 % are listed, and per scene where binning with
                       its builds is ahead of (b): what AUTO's rule for the call rests on.
  grid                 mirt_intersect_device and mirt_occluded_device under mirt_set_ray_grid(1) -- the structure built by the call, and
                       held -- beside the same call with the switch off, in the same run on the same rays: mirror reflections of the
                       1080p primary hits, 16 cosine-distributed hemisphere rays per hit point and uniform segments in the box, 1 .. 2^20
                       rays in powers of four at n = 100 000 and n = 2 000.  The answers are compared first; every cell is recorded, the
                       cells where the grid is behind by more than 2 % are listed, and from which ray count the build pays.

The knob is read once per process, so every GPU step is a child process of its own, under its own `timeout`; a step that fails
ends the run."""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cpp-raytracer-rasterizer_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HUGE = "2000000000"
W, H, CAM, FOCAL = 1920, 1080, (0.0, 0.0, -2.0), 540.0


# ---- static: the per-test instructions of a kernel ---------------------------------------------------------------------

def test_segments(asm_kernel_lines):
    """The straight-line code every test runs: from the first ds_read_b128 of a row to the next branch (what follows is the exact
    path, entered only by the lanes the filter lets through).  Returns [(valu, packed, issue cycles)] in text order."""
    import issue_mix as im
    out, cur = [], None
    for t in asm_kernel_lines:
        t = t.strip()
        if t.startswith("ds_read_b128") and cur is None:
            cur = {"valu": 0, "packed": 0, "cycles": 0.0}
        elif cur is not None and t.startswith(("s_cbranch", "s_branch")):
            out.append((cur["valu"], cur["packed"], cur["cycles"]))
            cur = None
        elif cur is not None and t.startswith("v_"):
            cur["valu"] += 1
            cur["packed"] += t.startswith("v_pk_")
            cur["cycles"] += im.CYCLES[im.classify(t)]
    return out


def kernel_text(path, flags, want):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run(["hipcc"] + flags + ["-c", path, "-o", out], check=True, capture_output=True)
        lines = open(out).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*%s\S*:" % want, l))
    end = next(i for i in range(start, len(lines)) if ".Lfunc_end" in lines[i])
    return lines[start:end]


def step_issue(p):
    import issue_mix as im
    q = test_segments(kernel_text(os.path.join(PKG, "query", "rt_query.hip"), im.FLAGS, "k_query_closestILi2"))
    b = test_segments(kernel_text(os.path.join(PKG, "csrc", "rt_kernels.hip"), im.FLAGS, "k_rt_bruteILi2"))
    p("== issue: vector instructions per test of two rays (one LDS row, both rays of the lane; static, from the assembly) ==")
    p("k_query_closest<2>   segments (valu, packed, issue cycles): %s" % ", ".join("(%d, %d, %.1f)" % s for s in q))
    p("k_rt_brute<2>        segments (valu, packed, issue cycles): %s" % ", ".join("(%d, %d, %.1f)" % s for s in b))
    # the loops that run the filter are the packed ones; k_rt_brute's text holds them for the primary and the shadow sweep of
    # either supersampling variant, and exact-only variants without a packed instruction
    qf = [s for s in q if s[1] > 0]
    bf = [s for s in b if s[1] > 0]
    # ... of which the shadow sweep carries a `live` mask besides: the primary sweep, which the throughput step times, is the shortest
    qs, bs = min(qf, key=lambda s: s[2]), min(bf, key=lambda s: s[2])
    qc, bc = qs[2], bs[2]
    p("filtered test of the primary sweep: query %.1f issue cycles (%d valu, %d packed), brute %.1f (%d valu, %d packed)" % (qc, qs[0], qs[1], bc, bs[0], bs[1]))
    p("expected_ratio query/brute per test = %.2f" % (qc / bc))
    p("")
    return qc / bc


# ---- occupancy -------------------------------------------------------------------------------------------------------------

def step_occupancy(p):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_spills.py")], capture_output=True, text=True, check=True)
    p("== occupancy (tools/check_spills.py) ==")
    for line in r.stdout.split("\n"):
        if "k_query_" in line or "k_rt_brute" in line or "k_rt_wave" in line or line.startswith("no kernel spills"):
            p(line)
    p("")


# ---- GPU steps (children) --------------------------------------------------------------------------------------------------

def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def dev_alloc(h, nbytes, src=None):
    ptr = C.c_void_p()
    assert h.hipMalloc(C.byref(ptr), max(int(nbytes), 16)) == 0
    if src is not None:
        assert h.hipMemcpy(ptr, src.ctypes.data_as(C.c_void_p), src.nbytes, 1) == 0
    assert h.hipDeviceSynchronize() == 0
    return ptr


def primary_rays(mirt, rot):
    """Draw()'s rays (raytracer.cpp:579-580) in float32, operation by operation: d = (x - W/2, y - H/2, f), dir = R * d."""
    x = (np.arange(W, dtype=np.float32) - np.float32(W) / np.float32(2))[None, :].repeat(H, 0)
    y = (np.arange(H, dtype=np.float32) - np.float32(H) / np.float32(2))[:, None].repeat(W, 1)
    f = np.float32(FOCAL)
    rays = np.zeros(W * H, mirt.RAY_DTYPE)
    rays["start"] = np.asarray(CAM, np.float32)
    for r in range(3):
        rays["dir"][:, r] = (rot[r] * x + rot[3 + r] * y + rot[6 + r] * f).ravel()
    return rays


def timed(mirt, fn, reps):
    fn(); mirt.sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn(); mirt.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def child_throughput():
    import mirt
    h = hip()
    mirt.init(0)
    mirt.scene_upload(mirt.scene_soup(1, 100000, 0.05))
    rot = mirt.rot_from_yaw(0.0, 1.0)
    view = mirt.make_view(CAM, rot, FOCAL, W, H)
    rays = primary_rays(mirt, rot)
    fresh = mirt.fresh_hits(len(rays))
    d_rays, d_hits = dev_alloc(h, rays.nbytes, rays), dev_alloc(h, fresh.nbytes, fresh)
    d_x, d_idx = dev_alloc(h, W * H * 4), dev_alloc(h, W * H * 4)

    def query():
        assert h.hipMemcpy(d_hits, fresh.ctypes.data_as(C.c_void_p), fresh.nbytes, 1) == 0
        t0 = time.perf_counter()
        mirt.intersect_device(d_rays, len(rays), d_hits); mirt.sync()
        return (time.perf_counter() - t0) * 1e3
    query()
    q_ms = float(np.median([query() for _ in range(3)]))
    b_ms = timed(mirt, lambda: mirt.raytrace_device(view, np.zeros((0, 7), np.float32), (0.2, 0.2, 0.2), mirt.RT_BRUTE, 0, H, 0, d_x, W * 4, None, d_idx), 3)
    lit_ms = timed(mirt, lambda: mirt.raytrace_device(view, mirt.DEFAULT_LIGHT, (0.2, 0.2, 0.2), mirt.RT_BRUTE, 0, H, 0, d_x, W * 4, None, d_idx), 2)
    got, idx = np.zeros(len(rays), mirt.HIT_DTYPE), np.zeros(W * H, np.int32)
    assert h.hipMemcpy(got.ctypes.data_as(C.c_void_p), d_hits, got.nbytes, 2) == 0
    assert h.hipMemcpy(idx.ctypes.data_as(C.c_void_p), d_idx, idx.nbytes, 2) == 0
    assert np.array_equal(got["index"], idx), "query and frame disagree"
    tests = len(rays) * 100000.0
    print("RESULT rays %d triangles 100000 knob %s" % (len(rays), os.environ.get("MIRT_QUERY_WAVE_RAYS", "default")))
    print("RESULT k_query_closest<2>: %.2f ms (%.1f G tests/s), every index equal to the frame's" % (q_ms, tests / q_ms * 1e-6))
    print("RESULT BRUTE frame without lights (k_prep_origin + k_rt_brute<2>, primary rays only): %.2f ms (%.1f G tests/s)" % (b_ms, tests / b_ms * 1e-6))
    print("RESULT BRUTE frame with the default light (primary + shadow sweep): %.2f ms" % lit_ms)
    print("RESULT measured_ratio query/brute(primary only) = %.3f" % (q_ms / b_ms))
    mirt.shutdown()


def child_sweep(n):
    import mirt
    h = hip()
    mirt.init(0)
    mirt.scene_upload(mirt.scene_soup(1, n, 0.05 if n >= 50000 else 0.2))
    rng = np.random.default_rng(7)
    top = 1 << 20
    start = rng.uniform(-1.5, 1.5, (top, 3)).astype(np.float32)
    target = rng.uniform(-1.0, 1.0, (top, 3)).astype(np.float32)
    rays = mirt.make_rays(start, target - start)
    d_rays, d_hits = dev_alloc(h, rays.nbytes, rays), dev_alloc(h, top * 20, mirt.fresh_hits(top))
    k = 1
    while k <= top:
        reps = 9 if k <= 65536 else 3
        ms = timed(mirt, lambda: mirt.intersect_device(d_rays, k, d_hits), reps)
        print("RESULT n %6d knob %-10s rays %8d  %9.4f ms" % (n, os.environ.get("MIRT_QUERY_WAVE_RAYS"), k, ms))
        sys.stdout.flush()
        k *= 2
    mirt.shutdown()


def closest_records(mirt, h, n, s):
    """soup(1, n, s) uploaded, and the closest-hit records of the view's primary rays on the device: (d_hits, count)."""
    mirt.scene_upload(mirt.scene_soup(1, n, s))
    rays = primary_rays(mirt, mirt.rot_from_yaw(0.0, 1.0))
    fresh = mirt.fresh_hits(len(rays))
    d_rays, d_hits = dev_alloc(h, rays.nbytes, rays), dev_alloc(h, fresh.nbytes, fresh)
    mirt.intersect_device(d_rays, len(rays), d_hits); mirt.sync()
    h.hipFree(d_rays)
    return d_hits, len(rays)


def nudged(light, i):
    """The default light, its x moved by i ulps: another cube key, the same work."""
    l = np.array(light, np.float32).copy()
    for _ in range(i):
        l[0, 0] = np.nextafter(l[0, 0], np.float32(1))
    return l


def child_directlight(mode):
    import hashlib
    import mirt
    h = hip()
    mirt.init(0)
    d_hits, count = closest_records(mirt, h, 100000, 0.05)
    d_rgb = dev_alloc(h, count * 12)
    rgb = np.zeros((count, 3), np.float32)

    def digest():
        assert h.hipMemcpy(rgb.ctypes.data_as(C.c_void_p), d_rgb, rgb.nbytes, 2) == 0
        return hashlib.sha1(rgb.tobytes()).hexdigest()[:16]
    mirt.set_query_mode(mirt.QUERY_BRUTE if mode == "brute" else mirt.QUERY_BINNED)
    if mode == "brute":
        ms = timed(mirt, lambda: mirt.direct_light_device(d_hits, count, mirt.DEFAULT_LIGHT, d_rgb), 2)
        assert mirt.query_stats()["mode_used"] == mirt.QUERY_BRUTE
        print("RESULT records %d triangles 100000 lights 1" % count)
        print("RESULT BRUTE  (k_prep_origin + k_query_direct_light<2>): %.3f ms  digest %s" % (ms, digest()))
    else:
        built = []
        for i in range(1, 6):                    # a cube of its own per call
            l = nudged(mirt.DEFAULT_LIGHT, i)
            t0 = time.perf_counter()
            mirt.direct_light_device(d_hits, count, l, d_rgb); mirt.sync()
            built.append((time.perf_counter() - t0) * 1e3)
            assert mirt.query_stats()["cube_source"] == 1
        mirt.direct_light_device(d_hits, count, mirt.DEFAULT_LIGHT, d_rgb); mirt.sync()
        kept = timed(mirt, lambda: mirt.direct_light_device(d_hits, count, mirt.DEFAULT_LIGHT, d_rgb), 9)
        st = mirt.query_stats()
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2
        dg = digest()
        mirt.set_profiling(True)
        mirt.direct_light_device(d_hits, count, mirt.DEFAULT_LIGHT, d_rgb)
        st = mirt.query_stats()
        mirt.set_profiling(False)
        print("RESULT BINNED, cube built by the call (median of %d, first %.3f ms): %.3f ms" % (len(built), built[0], float(np.median(built[1:]))))
        print("RESULT BINNED, cube kept: %.3f ms  digest %s" % (kept, dg))
        print("RESULT cube %d bins per side, %d shells; shadow rays %d, rows offered %d (%.1f per ray, of 100000), tests %d, fallback records %d"
              % (st["cube_bins"], st["shells"], st["shadow_rays"], st["candidates"], st["candidates"] / max(st["shadow_rays"], 1), st["tests"], st["fallback_records"]))
    mirt.shutdown()


def child_dlsweep(mode, n):
    import mirt
    h = hip()
    mirt.init(0)
    d_hits, count = closest_records(mirt, h, n, 0.05 if n >= 50000 else 0.2)
    # records in pixel order would make a small call one corner of the frame: a fixed shuffle instead, so that every call samples the frame
    rec = np.zeros(count, mirt.HIT_DTYPE)
    assert h.hipMemcpy(rec.ctypes.data_as(C.c_void_p), d_hits, rec.nbytes, 2) == 0
    rec = np.ascontiguousarray(rec[np.random.default_rng(5).permutation(count)])
    assert h.hipMemcpy(d_hits, rec.ctypes.data_as(C.c_void_p), rec.nbytes, 1) == 0
    d_rgb = dev_alloc(h, count * 12)
    mirt.set_query_mode(mirt.QUERY_BRUTE if mode == "brute" else mirt.QUERY_BINNED)
    k, nudge = 1, 0
    while k <= count:
        reps = 5 if k <= 65536 else 3
        if mode == "built":
            ts = []
            for _ in range(reps + 1):
                nudge += 1
                l = nudged(mirt.DEFAULT_LIGHT, 1 + nudge % 7)            # (never the key of the call before: the one cube held is another's)
                t0 = time.perf_counter()
                mirt.direct_light_device(d_hits, k, l, d_rgb); mirt.sync()
                ts.append((time.perf_counter() - t0) * 1e3)
                assert mirt.query_stats()["cube_source"] == 1
            ms = float(np.median(ts[1:]))
        else:
            ms = timed(mirt, lambda: mirt.direct_light_device(d_hits, k, mirt.DEFAULT_LIGHT, d_rgb), reps)
        print("RESULT dl n %6d mode %-6s records %8d  %9.4f ms" % (n, mode, k, ms))
        sys.stdout.flush()
        k *= 2
    mirt.shutdown()


def step_directlight(p):
    p("== directlight: mirt_direct_light_device over the closest hits of soup100k's primary rays at 1080p, one light (host clock around call + mirt_sync) ==")
    outs = [run_child(p, ["--child", "directlight", m], {}, 300) for m in ("brute", "binned")]
    b = re.search(r"BRUTE .*?: ([0-9.]+) ms  digest (\w+)", outs[0])
    bb = re.search(r"cube built by the call .*?: ([0-9.]+) ms\n", outs[1])
    bk = re.search(r"cube kept: ([0-9.]+) ms  digest (\w+)", outs[1])
    if b and bb and bk:
        p("colours bit-identical (sha1 of all %s): %s" % ("records", "yes" if b.group(2) == bk.group(2) else "NO: %s vs %s" % (b.group(2), bk.group(2))))
        p("ratio brute / binned with the build = %.1f; brute / binned with the cube kept = %.1f" % (float(b.group(1)) / float(bb.group(1)), float(b.group(1)) / float(bk.group(1))))
        if b.group(2) != bk.group(2):
            sys.exit(1)
    p("")
    p("== directlight sweep: ms per call against the record count (records of the frame in a fixed shuffled order) ==")
    table = {}
    for n in (100000, 2000):
        for mode in ("brute", "built", "kept"):
            out = run_child(lambda s: None, ["--child", "dlsweep", mode, str(n)], {}, 420)
            for m in re.finditer(r"RESULT dl n\s+(\d+) mode (\S+)\s+records\s+(\d+)\s+([0-9.]+) ms", out):
                table[(int(m.group(1)), m.group(2), int(m.group(3)))] = float(m.group(4))
    for n in (100000, 2000):
        p("n = %d triangles, 1 light" % n)
        p("%10s %14s %14s %14s   records x lights x n" % ("records", "brute", "binned+build", "binned kept"))
        k, cross = 1, None
        while (n, "brute", k) in table:
            a, b2, c = table[(n, "brute", k)], table[(n, "built", k)], table[(n, "kept", k)]
            p("%10d %11.4f ms %11.4f ms %11.4f ms   %.1e%s" % (k, a, b2, c, float(k) * n, "   binned+build ahead" if b2 < a else ""))
            if b2 >= a:
                cross = None
            elif cross is None:
                cross = k
            k *= 2
        p("binned with the build stays ahead from %s records on: records x lights x n = %s" % (cross, "%.1e" % (float(cross) * n) if cross else "never"))
        p("")


def nudged_origin(i):
    """The camera position, its x moved by i ulps: another cube key, the same work."""
    o = np.array(CAM, np.float32)
    for _ in range(i):
        o[0] = np.nextafter(o[0], np.float32(1))
    return o


def fan_inputs(mirt, h, n, s, shuffle):
    """soup(1, n, s) uploaded; the view's primary rays as rays and as bare directions on the device, and fresh records on the host."""
    mirt.scene_upload(mirt.scene_soup(1, n, s))
    rays = primary_rays(mirt, mirt.rot_from_yaw(0.0, 1.0))
    if shuffle:                              # rays in pixel order would make a small call one corner of the frame
        rays = np.ascontiguousarray(rays[np.random.default_rng(5).permutation(len(rays))])
    dirs = np.ascontiguousarray(rays["dir"])
    fresh = mirt.fresh_hits(len(rays))
    return dev_alloc(h, rays.nbytes, rays), dev_alloc(h, dirs.nbytes, dirs), dev_alloc(h, fresh.nbytes, fresh), fresh


def child_fan(mode):
    import hashlib
    import mirt
    h = hip()
    mirt.init(0)
    d_rays, d_dirs, d_hits, fresh = fan_inputs(mirt, h, 100000, 0.05, False)
    count = len(fresh)
    got = np.zeros(count, mirt.HIT_DTYPE)
    cam = np.array(CAM, np.float32)

    def reset():
        assert h.hipMemcpy(d_hits, fresh.ctypes.data_as(C.c_void_p), fresh.nbytes, 1) == 0

    def run(fn):
        reset()
        t0 = time.perf_counter()
        fn(); mirt.sync()
        return (time.perf_counter() - t0) * 1e3

    def digest():
        assert h.hipMemcpy(got.ctypes.data_as(C.c_void_p), d_hits, got.nbytes, 2) == 0
        return hashlib.sha1(got.tobytes()).hexdigest()[:16], float((got["index"] >= 0).mean())
    if mode == "query":
        f = lambda: mirt.intersect_device(d_rays, count, d_hits)
        run(f)
        ms = float(np.median([run(f) for _ in range(3)]))
        print("RESULT rays %d triangles 100000, one origin" % count)
        print("RESULT mirt_intersect_device (k_query_closest<2>, the yardstick): %.3f ms  digest %s  hit share %.3f" % ((ms,) + digest()))
    elif mode == "brute":
        mirt.set_query_mode(mirt.QUERY_BRUTE)
        f = lambda: mirt.intersect_from_device(cam, d_dirs, count, d_hits)
        run(f)
        ms = float(np.median([run(f) for _ in range(3)]))
        assert mirt.fan_stats()["mode_used"] == mirt.QUERY_BRUTE
        print("RESULT fan BRUTE  (k_prep_origin + k_query_fan<2>): %.3f ms  digest %s" % ((ms,) + digest()[:1]))
    else:
        mirt.set_query_mode(mirt.QUERY_BINNED)
        built = []
        for i in range(1, 6):                    # a cube of its own per call
            o = nudged_origin(i)
            built.append(run(lambda: mirt.intersect_from_device(o, d_dirs, count, d_hits)))
            assert mirt.fan_stats()["cube_source"] == 1
        f = lambda: mirt.intersect_from_device(cam, d_dirs, count, d_hits)
        run(f)
        kept = float(np.median([run(f) for _ in range(9)]))
        st = mirt.fan_stats()
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_source"] == 2
        dg = digest()[0]
        mirt.set_profiling(True)
        run(f)
        st = mirt.fan_stats()
        mirt.set_profiling(False)
        print("RESULT fan BINNED, cube built by the call (median of %d, first %.3f ms): %.3f ms" % (len(built) - 1, built[0], float(np.median(built[1:]))))
        print("RESULT fan BINNED, cube kept: %.3f ms  digest %s" % (kept, dg))
        print("RESULT cube %d bins per side, %d shells; rays %d, rows stepped over %d (%.2f per ray, of 100000), rows tested %d, rays that swept %d"
              % (st["cube_bins"], st["shells"], st["shadow_rays"], st["candidates"], st["candidates"] / max(st["shadow_rays"], 1), st["tests"], st["fallback_records"]))
    mirt.shutdown()


def child_fansweep(mode, n):
    import mirt
    h = hip()
    mirt.init(0)
    d_rays, d_dirs, d_hits, fresh = fan_inputs(mirt, h, n, 0.05 if n >= 50000 else 0.2, True)
    count = len(fresh)
    cam = np.array(CAM, np.float32)
    mirt.set_query_mode(mirt.QUERY_BINNED if mode in ("built", "kept") else mirt.QUERY_BRUTE)
    k, nudge = 1, 0
    while k <= count:
        reps = 5 if k <= 65536 else 3
        ts = []
        for _ in range(reps + 1):
            assert h.hipMemcpy(d_hits, fresh.ctypes.data_as(C.c_void_p), 20 * k, 1) == 0
            nudge += 1
            o = nudged_origin(1 + nudge % 7) if mode == "built" else cam      # (never the key of the call before: the one cube held is another's)
            t0 = time.perf_counter()
            if mode == "query":
                mirt.intersect_device(d_rays, k, d_hits)
            else:
                mirt.intersect_from_device(o, d_dirs, k, d_hits)
            mirt.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
            if mode == "built":
                assert mirt.fan_stats()["cube_source"] == 1
        print("RESULT fan n %6d mode %-6s rays %8d  %9.4f ms" % (n, mode, k, float(np.median(ts[1:]))))
        sys.stdout.flush()
        k *= 2
    mirt.shutdown()


def step_fan(p):
    p("== fan: the 2 073 600 primary rays of soup100k at 1080p as a fan from the camera (host clock around call + mirt_sync) ==")
    outs = [run_child(p, ["--child", "fan", m], {}, 300) for m in ("query", "brute", "binned")]
    q = re.search(r"yardstick\): ([0-9.]+) ms  digest (\w+)", outs[0])
    b = re.search(r"fan BRUTE .*?: ([0-9.]+) ms  digest (\w+)", outs[1])
    bb = re.search(r"cube built by the call .*?: ([0-9.]+) ms\n", outs[2])
    bk = re.search(r"cube kept: ([0-9.]+) ms  digest (\w+)", outs[2])
    if q and b and bb and bk:
        same = q.group(2) == b.group(2) == bk.group(2)
        p("records bit-identical (sha1 of all records): %s" % ("yes" if same else "NO: %s / %s / %s" % (q.group(2), b.group(2), bk.group(2))))
        p("mirt_intersect_device / fan: brute %.1f, binned with the build %.1f, binned with the cube kept %.1f"
          % (float(q.group(1)) / float(b.group(1)), float(q.group(1)) / float(bb.group(1)), float(q.group(1)) / float(bk.group(1))))
        if not same:
            sys.exit(1)
    p("")
    p("== fan sweep: ms per call against the ray count (rays of the frame in a fixed shuffled order) ==")
    table = {}
    modes = ("query", "brute", "built", "kept")
    for n in (100000, 2000):
        for mode in modes:
            out = run_child(lambda s: None, ["--child", "fansweep", mode, str(n)], {}, 420)
            for m in re.finditer(r"RESULT fan n\s+(\d+) mode (\S+)\s+rays\s+(\d+)\s+([0-9.]+) ms", out):
                table[(int(m.group(1)), m.group(2), int(m.group(3)))] = float(m.group(4))
    for n in (100000, 2000):
        p("n = %d triangles" % n)
        p("%10s %16s %14s %14s %14s   rays x n" % ("rays", "mirt_intersect", "fan brute", "binned+build", "binned kept"))
        k, cross = 1, None
        while (n, "brute", k) in table:
            q2, a, b2, c = (table[(n, m, k)] for m in modes)
            p("%10d %13.4f ms %11.4f ms %11.4f ms %11.4f ms   %.1e%s" % (k, q2, a, b2, c, float(k) * n, "   binned+build ahead" if b2 < a else ""))
            if b2 >= a:
                cross = None
            elif cross is None:
                cross = k
            k *= 2
        p("binned with the build stays ahead of the fan's sweep from %s rays on: rays x n = %s" % (cross, "%.1e" % (float(cross) * n) if cross else "never"))
        p("")


FANS_K = (1, 4, 32, 128)
FANS_R = (64, 4096, 65536)


def child_fans(n):
    """mirt_intersect_fans_device against K consecutive mirt_intersect_from_device calls on the same rays, grouped by origin."""
    import hashlib
    import mirt
    h = hip()
    mirt.init(0)
    mirt.scene_upload(mirt.scene_soup(1, n, 0.05 if n >= 50000 else 0.2))
    rng = np.random.default_rng(9)
    all_origins = rng.uniform(-0.5, 0.5, (max(FANS_K), 3)).astype(np.float32)          # inside the scene
    for K in FANS_K:
        for R in FANS_R:
            origins = np.ascontiguousarray(all_origins[:K])
            count = K * R
            of = np.repeat(np.arange(K, dtype=np.int32), R)
            dirs = np.ascontiguousarray(rng.uniform(-1.0, 1.0, (count, 3)).astype(np.float32) - origins[of])
            fresh = mirt.fresh_hits(count)
            d_of, d_dirs, d_hits = dev_alloc(h, of.nbytes, of), dev_alloc(h, dirs.nbytes, dirs), dev_alloc(h, fresh.nbytes, fresh)
            got = np.zeros(count, mirt.HIT_DTYPE)
            reps = 5 if count <= 1 << 18 else 3

            def nudged(i):
                """Origin 0 moved by i ulps: other cube keys, the same work."""
                o = origins.copy()
                for _ in range(i):
                    o[0, 0] = np.nextafter(o[0, 0], np.float32(1))
                return o

            def one_call(o):
                mirt.intersect_fans_device(o, d_of, d_dirs, count, d_hits)

            def k_calls(o):
                for k in range(K):
                    mirt.intersect_from_device(o[k], C.c_void_p(d_dirs.value + 12 * k * R), R, C.c_void_p(d_hits.value + 20 * k * R))

            def run(fn, o):
                assert h.hipMemcpy(d_hits, fresh.ctypes.data_as(C.c_void_p), fresh.nbytes, 1) == 0
                t0 = time.perf_counter()
                fn(o); mirt.sync()
                return (time.perf_counter() - t0) * 1e3

            def digest():
                assert h.hipMemcpy(got.ctypes.data_as(C.c_void_p), d_hits, got.nbytes, 2) == 0
                return hashlib.sha1(got.tobytes()).hexdigest()[:16]

            ms, dg = {}, {}
            mirt.set_query_mode(mirt.QUERY_BINNED)
            ts = []
            for i in range(reps + 1):                   # (never the keys of the call before: every pass builds its cube)
                ts.append(run(one_call, nudged(1 + i)))
                assert mirt.fan_stats()["cube_source"] == 1
            ms["built"] = float(np.median(ts[1:]))
            run(one_call, origins)
            st = mirt.fan_stats()
            dg["built"] = digest()
            if K <= mirt.MAX_LIGHTS:                     # (the kept cubes are timed for one pass; a call of up to eight passes keeps them all)
                ts = [run(one_call, origins) for _ in range(reps + 1)]
                assert mirt.fan_stats()["cube_source"] == 2
                ms["kept"] = float(np.median(ts[1:]))
                dg["kept"] = digest()
            mirt.set_query_mode(mirt.QUERY_BRUTE)
            ts = [run(one_call, origins) for _ in range(reps + 1)]
            assert mirt.fan_stats()["mode_used"] == mirt.QUERY_BRUTE
            ms["brute"] = float(np.median(ts[1:]))
            dg["brute"] = digest()
            mirt.set_query_mode(mirt.QUERY_AUTO)         # the yardstick as a caller of the single fan meets it
            ts = [run(k_calls, nudged(1 + i)) for i in range(reps + 1)]
            ms["yard"] = float(np.median(ts[1:]))
            run(k_calls, origins)
            yard_mode = mirt.fan_stats()["mode_used"]
            dg["yard"] = digest()
            same = len(set(dg.values())) == 1
            print("RESULT fans n %6d K %3d rays/origin %6d grid %3d  built %10.4f  kept %s  brute %10.4f  K calls (%s) %10.4f ms  digest %s %s"
                  % (n, K, R, st["cube_bins"], ms["built"], "%10.4f" % ms["kept"] if "kept" in ms else "         -", ms["brute"],
                     "binned" if yard_mode == mirt.QUERY_BINNED else "brute", ms["yard"], dg["yard"], "same" if same else "DIFFERENT %r" % dg))
            sys.stdout.flush()
            for d in (d_of, d_dirs, d_hits):
                h.hipFree(d)
            if not same:
                sys.exit(1)
    mirt.shutdown()


def step_fans(p):
    p("== fans: mirt_intersect_fans_device, K origins inside the scene x rays per origin, rays grouped by origin (host clock around call + mirt_sync, medians) ==")
    p("built: BINNED, every pass builds its cube; kept: BINNED, the cube held (K <= 32); brute: BRUTE (expansion + mirt_intersect_device's kernels);")
    p("K calls: the yardstick, K consecutive mirt_intersect_from_device calls under AUTO, a cube built per call.  One digest over all records of every variant.")
    out = "".join(run_child(p, ["--child", "fans", str(n)], {}, 540) for n in (100000, 2000))
    fans_summary(out, p)


FANS_ROW = re.compile(r"fans n\s+(\d+) K\s+(\d+) rays/origin\s+(\d+) grid\s+\d+  built\s+([0-9.]+)  kept\s+\S+  brute\s+([0-9.]+)  K calls \(\w+\)\s+([0-9.]+) ms")


def fans_summary(text, p):
    """Where the one call is behind the K calls, and where binning with the builds is behind the brute path -- apart for the calls
    AUTO bins without a cube held (more than MIRT_QUERY_WAVE_RAYS = 4096 rays at these scene sizes) and those it does not."""
    rows = [(int(m.group(1)), int(m.group(2)), int(m.group(3)), float(m.group(4)), float(m.group(5)), float(m.group(6))) for m in FANS_ROW.finditer(text)]
    cell = lambda n, K, R: "n %d K %d rays/origin %d" % (n, K, R)
    behind = ["%s: %.3f ms against %.3f ms" % (cell(n, K, R), b, y) for n, K, R, b, _, y in rows if K > 1 and b > y]
    p("one call with its builds behind the K calls (K > 1), of %d cells: %s" % (len(rows), "; ".join(behind) if behind else "nowhere"))
    small = [(n, K, R, b, br) for n, K, R, b, br, _ in rows if K * R <= 4096]
    large = [(n, K, R, b, br) for n, K, R, b, br, _ in rows if K * R > 4096]
    p("calls of at most 4096 rays (AUTO takes the brute path unless the cubes are held): brute ahead of binning with the builds in %d of %d cells"
      % (sum(br < b for _, _, _, b, br in small), len(small)))
    wrong = ["%s: built %.3f ms, brute %.3f ms" % (cell(n, K, R), b, br) for n, K, R, b, br in large if b > br]
    p("calls of more than 4096 rays (AUTO bins): binning with the builds behind brute at: %s" % ("; ".join(wrong) if wrong else "nowhere"))
    p("")


# ---- occlusion queries: mirt_occluded*_device beside what a caller had to do before them ------------------------------------------

OCC_K = (1, 4, 32)


def half_limits(hits):
    """Half the ray's closest distance (1.0 where it hit nothing): nothing is nearer, so no ray meets an occluder."""
    return np.ascontiguousarray(np.where(hits["index"] >= 0, hits["distance"] * np.float32(0.5), np.float32(1.0)).astype(np.float32))


def child_occsweep(n):
    """mirt_occluded_device (no limits: a ray stops at its first occluder; limits at half the closest distance: nothing stops a
    ray) beside mirt_intersect_device from fresh records on the same rays -- the rays of the `sweep` step."""
    import mirt
    h = hip()
    mirt.init(0)
    mirt.scene_upload(mirt.scene_soup(1, n, 0.05 if n >= 50000 else 0.2))
    rng = np.random.default_rng(7)
    top = 1 << 20
    start = rng.uniform(-1.5, 1.5, (top, 3)).astype(np.float32)
    target = rng.uniform(-1.0, 1.0, (top, 3)).astype(np.float32)
    rays = mirt.make_rays(start, target - start)
    fresh = mirt.fresh_hits(top)
    d_rays, d_hits, d_occ = dev_alloc(h, rays.nbytes, rays), dev_alloc(h, fresh.nbytes, fresh), dev_alloc(h, top)
    mirt.intersect_device(d_rays, top, d_hits); mirt.sync()
    hits, occ = np.zeros(top, mirt.HIT_DTYPE), np.zeros(top, np.uint8)
    assert h.hipMemcpy(hits.ctypes.data_as(C.c_void_p), d_hits, hits.nbytes, 2) == 0
    lim = half_limits(hits)
    d_lim = dev_alloc(h, lim.nbytes, lim)
    # the answers first: no limits is "hit anything at all", half the closest distance is 0 everywhere
    for d_l, want in ((None, (hits["index"] >= 0).astype(np.uint8)), (d_lim, np.zeros(top, np.uint8))):
        mirt.occluded_device(d_rays, top, d_l, d_occ); mirt.sync()
        assert h.hipMemcpy(occ.ctypes.data_as(C.c_void_p), d_occ, top, 2) == 0
        assert np.array_equal(occ, want), "mirt_occluded_device disagrees with mirt_intersect_device"
    print("RESULT occ n %6d: %d rays, %.3f of them hit something; both answers equal to mirt_intersect_device's" % (n, top, float((hits["index"] >= 0).mean())))

    def closest(k):
        assert h.hipMemcpy(d_hits, fresh.ctypes.data_as(C.c_void_p), 20 * k, 1) == 0
        t0 = time.perf_counter()
        mirt.intersect_device(d_rays, k, d_hits); mirt.sync()
        return (time.perf_counter() - t0) * 1e3
    k = 1
    while k <= top:
        reps = 7 if k <= 65536 else 3
        closest(k)
        c_ms = float(np.median([closest(k) for _ in range(reps)]))
        o_ms = timed(mirt, lambda: mirt.occluded_device(d_rays, k, None, d_occ), reps)
        l_ms = timed(mirt, lambda: mirt.occluded_device(d_rays, k, d_lim, d_occ), reps)
        print("RESULT occ n %6d rays %8d  intersect %10.4f  occluded %10.4f  occluded, half limits %10.4f ms" % (n, k, c_ms, o_ms, l_ms))
        sys.stdout.flush()
        k *= 4
    mirt.shutdown()


def child_occfans(n):
    """mirt_occluded_fans_device beside mirt_intersect_fans_device from fresh records on the same rays: K origins inside the scene,
    rays dealt to them at random, under BRUTE, under BINNED with every cube built by the call (origin 0 moves by one ulp between the
    calls) and under BINNED with the cube held."""
    import mirt
    h = hip()
    mirt.init(0)
    mirt.scene_upload(mirt.scene_soup(1, n, 0.05 if n >= 50000 else 0.2))
    rng = np.random.default_rng(9)
    top = 1 << 20
    for K in OCC_K:
        origins = np.ascontiguousarray(rng.uniform(-0.5, 0.5, (K, 3)).astype(np.float32))
        of = rng.integers(0, K, top).astype(np.int32)
        dirs = np.ascontiguousarray(rng.uniform(-1.0, 1.0, (top, 3)).astype(np.float32) - origins[of])
        fresh = mirt.fresh_hits(top)
        d_of, d_dirs, d_hits, d_occ = dev_alloc(h, of.nbytes, of), dev_alloc(h, dirs.nbytes, dirs), dev_alloc(h, fresh.nbytes, fresh), dev_alloc(h, top)
        mirt.set_query_mode(mirt.QUERY_BRUTE)
        mirt.intersect_fans_device(origins, d_of, d_dirs, top, d_hits); mirt.sync()
        hits, occ = np.zeros(top, mirt.HIT_DTYPE), np.zeros(top, np.uint8)
        assert h.hipMemcpy(hits.ctypes.data_as(C.c_void_p), d_hits, hits.nbytes, 2) == 0
        lim = half_limits(hits)
        d_lim = dev_alloc(h, lim.nbytes, lim)
        for mode in (mirt.QUERY_BRUTE, mirt.QUERY_BINNED):
            mirt.set_query_mode(mode)
            for d_l, want in ((None, (hits["index"] >= 0).astype(np.uint8)), (d_lim, np.zeros(top, np.uint8))):
                mirt.occluded_fans_device(origins, d_of, d_dirs, top, d_l, d_occ); mirt.sync()
                assert h.hipMemcpy(occ.ctypes.data_as(C.c_void_p), d_occ, top, 2) == 0
                assert np.array_equal(occ, want), "mirt_occluded_fans_device disagrees with mirt_intersect_fans_device"

        def nudged(i):
            o = origins.copy()
            for _ in range(i):
                o[0, 0] = np.nextafter(o[0, 0], np.float32(1))
            return o

        def run(fn, o, k):
            assert h.hipMemcpy(d_hits, fresh.ctypes.data_as(C.c_void_p), 20 * k, 1) == 0
            t0 = time.perf_counter()
            fn(o, k); mirt.sync()
            return (time.perf_counter() - t0) * 1e3
        calls = (("intersect", lambda o, k: mirt.intersect_fans_device(o, d_of, d_dirs, k, d_hits), mirt.fan_stats),
                 ("occluded", lambda o, k: mirt.occluded_fans_device(o, d_of, d_dirs, k, None, d_occ), mirt.occlusion_stats),
                 ("half", lambda o, k: mirt.occluded_fans_device(o, d_of, d_dirs, k, d_lim, d_occ), mirt.occlusion_stats))
        k, nudge = 1, 0
        while k <= top:
            reps = 5 if k <= 65536 else 3
            ms = {}
            for name, fn, stats in calls:
                mirt.set_query_mode(mirt.QUERY_BRUTE)
                ms[name, "brute"] = float(np.median([run(fn, origins, k) for _ in range(reps + 1)][1:]))
                mirt.set_query_mode(mirt.QUERY_BINNED)
                ts = []
                for _ in range(reps + 1):                # (never the key of the call before: the one cube held is another's)
                    nudge += 1
                    ts.append(run(fn, nudged(1 + nudge % 7), k))
                    assert stats()["cube_source"] == 1
                ms[name, "built"] = float(np.median(ts[1:]))
                ts = [run(fn, origins, k) for _ in range(reps + 2)]
                assert stats()["cube_source"] == 2
                ms[name, "kept"] = float(np.median(ts[2:]))
            print("RESULT occfans n %6d K %2d rays %8d  " % (n, K, k)
                  + "  ".join("%s %s" % (name, " ".join("%9.4f" % ms[name, m] for m in ("brute", "built", "kept"))) for name, _, _ in calls) + " ms")
            sys.stdout.flush()
            k *= 4
        for d in (d_of, d_dirs, d_hits, d_occ, d_lim):
            h.hipFree(d)
    mirt.shutdown()


OCC_ROW = re.compile(r"occ n\s+(\d+) rays\s+(\d+)  intersect\s+([0-9.]+)  occluded\s+([0-9.]+)  occluded, half limits\s+([0-9.]+) ms")
OCCFANS_ROW = re.compile(r"occfans n\s+(\d+) K\s+(\d+) rays\s+(\d+)  intersect\s+([0-9.]+)\s+([0-9.]+)\s+([0-9.]+)  occluded\s+([0-9.]+)\s+([0-9.]+)\s+([0-9.]+)"
                         r"  half\s+([0-9.]+)\s+([0-9.]+)\s+([0-9.]+) ms")


def occluded_summary(text, p):
    """Where an occlusion call is behind the closest-hit call a caller had to make for the same answer (same rays, same mode, same
    run), and where binning with the builds crosses the brute path for the many-origin form."""
    behind, far = [], lambda v, c: v > 1.02 * c
    for m in OCC_ROW.finditer(text):
        n, k, c, o, l = int(m.group(1)), int(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5))
        behind += ["n %d rays %d %s: %.4f ms against %.4f ms" % (n, k, what, v, c) for what, v in (("no limits", o), ("half limits", l)) if far(v, c)]
    rows = [(int(m.group(1)), int(m.group(2)), int(m.group(3))) + tuple(float(x) for x in m.groups()[3:]) for m in OCCFANS_ROW.finditer(text)]
    for n, K, k, *v in rows:
        for j, mode in enumerate(("brute", "built", "kept")):
            behind += ["n %d K %d rays %d %s, %s: %.4f ms against %.4f ms" % (n, K, k, mode, what, v[off + j], v[j])
                       for what, off in (("no limits", 3), ("half limits", 6)) if far(v[off + j], v[j])]
    p("an occlusion call behind the closest-hit call on the same rays under the same mode by more than 2 %% of its time (the medians of one "
      "cell differ by that much from run to run): %s" % ("; ".join(behind) if behind else "nowhere"))
    for what, off in (("no limits", 3), ("half limits", 6)):
        small = [r for r in rows if r[2] <= 4096]
        large = [r for r in rows if r[2] > 4096]
        p("mirt_occluded_fans_device, %s: brute ahead of binning with the builds in %d of %d cells of at most 4096 rays (AUTO: brute unless held); "
          "binning with the builds behind brute beyond 4096 rays (AUTO: binned) at: %s"
          % (what, sum(r[3 + off] < r[3 + off + 1] for r in small), len(small),
             "; ".join("n %d K %d rays %d (%.4f against %.4f ms)" % (r[0], r[1], r[2], r[3 + off + 1], r[3 + off]) for r in large if r[3 + off + 1] > r[3 + off]) or "nowhere"))
    p("")


def step_occluded(p):
    p("== occluded: mirt_occluded_device beside mirt_intersect_device from fresh records, the same rays (host clock around call + mirt_sync, medians) ==")
    p("occluded: no limits, a ray stops at its first occluder; half limits: limits at half the closest distance, nothing stops a ray")
    out = "".join(run_child(p, ["--child", "occsweep", str(n)], {}, 300) for n in (100000, 2000))
    p("")
    p("== occluded fans: mirt_occluded_fans_device beside mirt_intersect_fans_device from fresh records, K origins inside the scene, rays dealt at random ==")
    p("three columns each: BRUTE; BINNED, every cube built by the call; BINNED, the cube held")
    out += "".join(run_child(p, ["--child", "occfans", str(n)], {}, 420) for n in (100000, 2000))
    occluded_summary(out, p)


# ---- ray queries along one direction: an orthographic grid of starts looking down the scene ------------------------------------------

def along_grid(k):
    """k = side x side starts over [-1.2, 1.2]^2 at z = -1.5, row by row."""
    side = int(round(k ** 0.5))
    assert side * side == k
    c = (np.arange(side, dtype=np.float64) + 0.5) / side * 2.4 - 1.2
    s = np.empty((side, side, 3), np.float32)
    s[:, :, 0], s[:, :, 1], s[:, :, 2] = c[None, :], c[:, None], -1.5
    return np.ascontiguousarray(s.reshape(-1, 3))


def child_along(n):
    """mirt_intersect_along_device / mirt_occluded_along_device (no limits) beside mirt_intersect_device / mirt_occluded_device from
    fresh records on the same rays: BINNED with the grid built by the call, BINNED with the grid held, and the yardsticks."""
    import mirt
    h = hip()
    mirt.init(0)
    mirt.scene_upload(mirt.scene_soup(1, n, 0.05 if n >= 50000 else 0.2))
    top = 1 << 20
    down = np.array([0, 0, 1], np.float32)
    fresh = mirt.fresh_hits(top)
    d_starts, d_rays, d_hits, d_occ = dev_alloc(h, 12 * top), dev_alloc(h, 24 * top), dev_alloc(h, fresh.nbytes, fresh), dev_alloc(h, top)

    def tilted(i):
        d = down.copy()
        d[0] = np.float32(i) * np.finfo(np.float32).smallest_subnormal
        return d

    def run(fn, k):
        assert h.hipMemcpy(d_hits, fresh.ctypes.data_as(C.c_void_p), 20 * k, 1) == 0
        t0 = time.perf_counter()
        fn(k); mirt.sync()
        return (time.perf_counter() - t0) * 1e3

    k, nudge = 1, 0
    while k <= top:
        starts = along_grid(k)
        rays = mirt.make_rays(starts, down)
        assert h.hipMemcpy(d_starts, starts.ctypes.data_as(C.c_void_p), starts.nbytes, 1) == 0
        assert h.hipMemcpy(d_rays, rays.ctypes.data_as(C.c_void_p), rays.nbytes, 1) == 0
        # the answers first
        want, got = np.zeros(k, mirt.HIT_DTYPE), np.zeros(k, mirt.HIT_DTYPE)
        wocc, gocc = np.zeros(k, np.uint8), np.zeros(k, np.uint8)
        run(lambda q: mirt.intersect_device(d_rays, q, d_hits), k)
        assert h.hipMemcpy(want.ctypes.data_as(C.c_void_p), d_hits, want.nbytes, 2) == 0
        mirt.occluded_device(d_rays, k, None, d_occ); mirt.sync()
        assert h.hipMemcpy(wocc.ctypes.data_as(C.c_void_p), d_occ, k, 2) == 0
        mirt.set_query_mode(mirt.QUERY_BINNED)
        run(lambda q: mirt.intersect_along_device(down, d_starts, q, d_hits), k)
        assert h.hipMemcpy(got.ctypes.data_as(C.c_void_p), d_hits, got.nbytes, 2) == 0
        mirt.occluded_along_device(down, d_starts, k, None, d_occ); mirt.sync()
        assert h.hipMemcpy(gocc.ctypes.data_as(C.c_void_p), d_occ, k, 2) == 0
        st = mirt.along_stats()
        assert st["mode_used"] == mirt.QUERY_BINNED, st
        assert got.tobytes() == want.tobytes() and np.array_equal(gocc, wocc), "the calls along a direction disagree with mirt_intersect_device / mirt_occluded_device"
        reps = 5 if k <= 65536 else 3
        ms = {}
        for name, yard, fn in (("intersect", lambda q: mirt.intersect_device(d_rays, q, d_hits), lambda d, q: mirt.intersect_along_device(d, d_starts, q, d_hits)),
                               ("occluded", lambda q: mirt.occluded_device(d_rays, q, None, d_occ), lambda d, q: mirt.occluded_along_device(d, d_starts, q, None, d_occ))):
            ms[name, "yard"] = float(np.median([run(yard, k) for _ in range(reps + 1)][1:]))
            ts = []
            for _ in range(reps + 1):                    # (never the key of the call before)
                nudge += 1
                ts.append(run(lambda q: fn(tilted(1 + nudge % 7), q), k))
                assert mirt.along_stats()["cube_source"] == 1
            ms[name, "built"] = float(np.median(ts[1:]))
            ts = [run(lambda q: fn(down, q), k) for _ in range(reps + 2)]
            assert mirt.along_stats()["cube_source"] == 2
            ms[name, "kept"] = float(np.median(ts[2:]))
        mirt.set_query_mode(mirt.QUERY_AUTO)
        print("RESULT along n %6d rays %8d B %3d hit %.3f  " % (n, k, st["cube_bins"], float((want["index"] >= 0).mean()))
              + "  ".join("%s %s" % (name, " ".join("%10.4f" % ms[name, m] for m in ("yard", "built", "kept"))) for name in ("intersect", "occluded")) + " ms")
        sys.stdout.flush()
        k *= 4
    mirt.shutdown()


ALONG_ROW = re.compile(r"along n\s+(\d+) rays\s+(\d+) B\s+\d+ hit [0-9.]+  intersect\s+([0-9.]+)\s+([0-9.]+)\s+([0-9.]+)  occluded\s+([0-9.]+)\s+([0-9.]+)\s+([0-9.]+) ms")


def step_along(p):
    p("== along: mirt_intersect_along_device / mirt_occluded_along_device, a square grid of starts looking down the scene (dir = +z), beside")
    p("   mirt_intersect_device / mirt_occluded_device from fresh records on the same rays (host clock around call + mirt_sync, medians) ==")
    p("AUTO starts with the fans' rule: bin from 2000 triangles on, or from MIRT_BIN_THRESHOLD triangles with rays x n >= 4e7, or when the grid is held;")
    p("under it every cell below would bin (both scenes have 2000 triangles or more): what the rows say of that follows them")
    p("three columns each: the yardstick; BINNED, the grid built by the call; BINNED, the grid held")
    out = "".join(run_child(p, ["--child", "along", str(n)], {}, 420) for n in (100000, 2000))
    along_summary(out, p)


def along_summary(text, p):
    """What the rows say: the cells where the new call is behind its yardstick (by more than the 2 % two runs differ by), with the
    grid built by the call and with it held, and -- per triangle count and call -- the ray count from which the call with its build
    stays ahead, which is where AUTO's rule would have to switch when the grid is not held."""
    rows = [(int(m.group(1)), int(m.group(2)), [float(x) for x in m.groups()[2:]]) for m in ALONG_ROW.finditer(text)]
    behind = {"built": [], "held": []}
    for n, k, v in rows:
        for what, off in (("intersect", 0), ("occluded", 3)):
            for j, mode in ((1, "built"), (2, "held")):
                if v[off + j] > 1.02 * v[off]:
                    behind[mode].append("n %d rays %d %s: %.4f ms against %.4f ms" % (n, k, what, v[off + j], v[off]))
    p("the new call behind its yardstick by more than 2 %, grid built by the call: " + ("; ".join(behind["built"]) or "nowhere"))
    p("the new call behind its yardstick by more than 2 %, grid held: " + ("; ".join(behind["held"]) or "nowhere"))
    crossings = []
    for n in sorted({r[0] for r in rows}, reverse=True):
        for what, off in (("intersect", 0), ("occluded", 3)):
            cells = sorted((k, v[off + 1] <= v[off]) for nn, k, v in rows if nn == n)
            lost = [k for k, ahead in cells if not ahead]
            first = min([k for k, _ in cells if not lost or k > max(lost)], default=None)
            crossings.append((n, what, len(lost), len(cells), first))
            p("n %d %s, grid built by the call: behind in %d of %d cells; ahead in every cell from %s rays on"
              % (n, what, len(lost), len(cells), first if first is not None else "no count measured"))
    starts = {c[4] for c in crossings}
    if all(c[2] == 0 for c in crossings):
        p("verdict: the fans' rule is confirmed -- with its build the call is ahead in every cell")
    elif len(starts) == 1 and None not in starts:
        p("verdict: the fans' rule is moved -- unless the grid is held, binning pays from %d rays on in every series (the cell before: %d rays)"
          % (starts.pop(), max(k for n, k, v in rows if k < min(c[4] for c in crossings))))
    else:
        p("verdict: the series disagree on where binning with its build starts to pay (%s): no single ray count moves the rule"
          % ", ".join("n %d %s from %s" % (c[0], c[1], c[4]) for c in crossings))
    p("")


# ---- arbitrary rays through the cell grid: mirt_intersect_device / mirt_occluded_device under mirt_set_ray_grid -----------------------------

GRID_SETS = ("mirror", "hemisphere", "segments")
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)


def grid_rays(mirt, h, tris, which, top):
    """Up to `top` rays of a set: mirror reflections of the 1080p primary hits; 16 cosine-distributed rays over the hemisphere of each
    hit point; uniform random segments in the box."""
    rng = np.random.default_rng(11)
    if which == "segments":
        a, b = rng.uniform(-1, 1, (top, 3)), rng.uniform(-1, 1, (top, 3))
        return mirt.make_rays(a.astype(np.float32), (b - a).astype(np.float32))
    prim = primary_rays(mirt, mirt.rot_from_yaw(0.0, 1.0))
    hits = mirt.fresh_hits(len(prim))
    d_r, d_h = dev_alloc(h, prim.nbytes, prim), dev_alloc(h, hits.nbytes, hits)
    mirt.intersect_device(d_r, len(prim), d_h); mirt.sync()
    assert h.hipMemcpy(hits.ctypes.data_as(C.c_void_p), d_h, hits.nbytes, 2) == 0
    h.hipFree(d_r); h.hipFree(d_h)
    hit = hits["index"] >= 0
    pos = hits["position"][hit].astype(np.float64)
    nrm = np.asarray(tris, np.float64).reshape(-1, 15)[hits["index"][hit], 9:12]
    d = prim["dir"][hit].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    nrm = np.where((nrm * d).sum(axis=1, keepdims=True) > 0, -nrm, nrm)            # towards the camera's side
    if which == "mirror":
        out = d - 2.0 * (d * nrm).sum(axis=1, keepdims=True) * nrm
    else:
        k = min(len(pos), top // 16)
        pos, nrm = np.repeat(pos[:k], 16, axis=0), np.repeat(nrm[:k], 16, axis=0)
        u1, u2 = rng.uniform(0, 1, len(pos)), rng.uniform(0, 2 * np.pi, len(pos))
        t1 = np.cross(nrm, np.where(np.abs(nrm[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]]))
        t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
        t2 = np.cross(nrm, t1)
        r = np.sqrt(u1)[:, None]
        out = r * np.cos(u2)[:, None] * t1 + r * np.sin(u2)[:, None] * t2 + np.sqrt(1 - u1)[:, None] * nrm
    rays = mirt.make_rays((pos + 1e-4 * nrm).astype(np.float32), out.astype(np.float32))
    return rays[:top]


def child_grid(n, which):
    """mirt_intersect_device / mirt_occluded_device (no limits) from fresh records under mirt_set_ray_grid(1) -- the structure built by
    the call (the scene version moved on by an identity transform outside the clock: the scene's rows are rebuilt inside it too), and
    held -- beside the same call with the switch off, on the same rays; results compared before any time is taken."""
    import mirt
    h = hip()
    mirt.init(0)
    tris = mirt.scene_soup(1, n, 0.05 if n >= 50000 else 0.2)
    mirt.scene_upload(tris)
    rays = grid_rays(mirt, h, tris, which, 1 << 20)
    top = len(rays)
    fresh = mirt.fresh_hits(top)
    d_rays, d_hits, d_occ = dev_alloc(h, rays.nbytes, rays), dev_alloc(h, fresh.nbytes, fresh), dev_alloc(h, top)

    def run(fn, k, rebuild=False):
        assert h.hipMemcpy(d_hits, fresh.ctypes.data_as(C.c_void_p), 20 * k, 1) == 0
        if rebuild:
            mirt.scene_transform(0, n, IDENTITY); mirt.sync()
        t0 = time.perf_counter()
        fn(k); mirt.sync()
        return (time.perf_counter() - t0) * 1e3

    calls = (("intersect", lambda q: mirt.intersect_device(d_rays, q, d_hits)), ("occluded", lambda q: mirt.occluded_device(d_rays, q, None, d_occ)))
    k = 1
    while k <= top:
        want, got = np.zeros(k, mirt.HIT_DTYPE), np.zeros(k, mirt.HIT_DTYPE)
        wocc, gocc = np.zeros(k, np.uint8), np.zeros(k, np.uint8)
        for on, rec, occ in ((False, want, wocc), (True, got, gocc)):
            mirt.set_ray_grid(on)
            run(calls[0][1], k)
            assert h.hipMemcpy(rec.ctypes.data_as(C.c_void_p), d_hits, rec.nbytes, 2) == 0
            calls[1][1](k); mirt.sync()
            assert h.hipMemcpy(occ.ctypes.data_as(C.c_void_p), d_occ, k, 2) == 0
        st = mirt.ray_grid_stats()
        assert st["mode_used"] == mirt.QUERY_BINNED and st["gave_up"] == 0, st
        assert got.tobytes() == want.tobytes() and np.array_equal(gocc, wocc), "the grid disagrees with the sweep"
        reps = 5 if k <= 65536 else 3
        ms = {}
        for name, fn in calls:
            mirt.set_ray_grid(False)
            ms[name, "yard"] = float(np.median([run(fn, k) for _ in range(reps + 1)][1:]))
            mirt.set_ray_grid(True)
            ts = []
            for _ in range(reps):
                ts.append(run(fn, k, rebuild=True))
                assert mirt.ray_grid_stats()["source"] == 1
            ms[name, "built"] = float(np.median(ts))
            ts = [run(fn, k) for _ in range(reps + 1)]
            assert mirt.ray_grid_stats()["source"] == 2
            ms[name, "kept"] = float(np.median(ts[1:]))
        mirt.set_ray_grid(False)
        print("RESULT grid n %6d %-10s rays %8d G %3d hit %.3f  " % (n, which, k, st["cells"], float((want["index"] >= 0).mean()))
              + "  ".join("%s %s" % (name, " ".join("%10.4f" % ms[name, m] for m in ("yard", "built", "kept"))) for name in ("intersect", "occluded")) + " ms")
        sys.stdout.flush()
        k = k * 4 if k * 4 <= top or k == top else top
    print("RESULT grid n %6d structure: %d rows (%d of the plane index, %d triangles for every ray)" % (n, st["pairs"], st["plane_pairs"], st["every_rows"]))
    mirt.shutdown()


GRID_ROW = re.compile(r"grid n\s+(\d+) (\w+)\s+rays\s+(\d+) G\s+\d+ hit [0-9.]+  intersect\s+([0-9.]+)\s+([0-9.]+)\s+([0-9.]+)  occluded\s+([0-9.]+)\s+([0-9.]+)\s+([0-9.]+) ms")


def step_grid(p):
    p("== grid: mirt_intersect_device / mirt_occluded_device under mirt_set_ray_grid(1) beside the same call with the switch off (the sweep: the")
    p("   parent's code unchanged), same run, same rays, from fresh records, no limits (host clock around call + mirt_sync, medians) ==")
    p("ray sets: mirror reflections of the 1080p primary hits; 16 cosine-distributed hemisphere rays per hit point; uniform segments in the box")
    p("three columns each: the switch off; on, the structure built by the call; on, the structure held")
    out = "".join(run_child(p, ["--child", "grid", str(n), which], {}, 420) for n in (100000, 2000) for which in GRID_SETS)
    grid_summary(out, p)


def grid_summary(text, p):
    """What the rows say: the cells where the grid is behind the sweep (by more than the 2 % two runs differ by), with the structure
    built by the call and with it held, and per scene, ray set and call the ray count from which the call with its build stays ahead."""
    out = text
    rows = [(int(m.group(1)), m.group(2), int(m.group(3)), [float(x) for x in m.groups()[3:]]) for m in GRID_ROW.finditer(out)]
    for mode, j in (("built by the call", 1), ("held", 2)):
        behind = ["n %d %s rays %d %s: %.4f ms against %.4f ms" % (n, w, k, what, v[off + j], v[off])
                  for n, w, k, v in rows for what, off in (("intersect", 0), ("occluded", 3)) if v[off + j] > 1.02 * v[off]]
        p("the grid behind the sweep by more than 2 %%, structure %s: %s" % (mode, "%d of %d cells" % (len(behind), 2 * len(rows)) if behind else "nowhere"))
        for line in behind:
            p("  " + line)
    for n in sorted({r[0] for r in rows}, reverse=True):
        for w in GRID_SETS:
            for what, off in (("intersect", 0), ("occluded", 3)):
                cells = sorted((k, v[off + 1] <= v[off]) for nn, ww, k, v in rows if nn == n and ww == w)
                lost = [k for k, ahead in cells if not ahead]
                first = min([k for k, _ in cells if not lost or k > max(lost)], default=None)
                p("n %d %s %s: with its build the grid pays from %s rays on" % (n, w, what, first if first is not None else "no count measured"))
    p("")


# ---- every hit along a ray, in order: mirt_intersect_ordered_device ------------------------------------------------------------------------

ORDERED_HITS = (1, 2, 4, 8)


def child_ordered(n, which):
    """mirt_intersect_ordered_device for max_hits 1, 2, 4 and 8 on the grid section's ray sets, the switch of mirt_set_ray_grid off and on
    (the structure built by the call -- the scene version moved on by an identity transform outside the clock --, and held), beside two
    yardsticks in the same run on the same rays: mirt_intersect_device from fresh records (what one hit costs today), and max_hits
    in-place peels of the max_hits == 1 call (after == hits; what the single walk saves).  Answers are compared before any time is
    taken: the switch on against off, slot 0 against mirt_intersect_device, and the eight peels against the max_hits == 8 call."""
    import mirt
    h = hip()
    mirt.init(0)
    tris = mirt.scene_soup(1, n, 0.05 if n >= 50000 else 0.2)
    mirt.scene_upload(tris)
    rays = grid_rays(mirt, h, tris, which, 1 << 20)
    top = len(rays)
    fresh = mirt.fresh_hits(top)
    behind = fresh.copy()
    behind["distance"] = -1.0                                       # the record every hit lies behind: where a peel starts
    d_rays, d_rec, d_hits, d_cnt = dev_alloc(h, rays.nbytes, rays), dev_alloc(h, fresh.nbytes, fresh), dev_alloc(h, 8 * fresh.nbytes), dev_alloc(h, 4 * top)

    def run(fn, k, start=fresh, rebuild=False):
        assert h.hipMemcpy(d_rec, start.ctypes.data_as(C.c_void_p), 20 * k, 1) == 0
        if rebuild:
            mirt.scene_transform(0, n, IDENTITY); mirt.sync()
        t0 = time.perf_counter()
        fn(k); mirt.sync()
        return (time.perf_counter() - t0) * 1e3

    def intersect(q):
        mirt.intersect_device(d_rays, q, d_rec)

    def ordered(m):
        return lambda q: mirt.intersect_ordered_device(d_rays, q, None, m, d_hits, d_cnt)

    def peels(m):
        def fn(q):
            for _ in range(m):
                mirt.intersect_ordered_device(d_rays, q, d_rec, 1, d_rec, d_cnt)
        return fn

    def back(ptr, count, dtype):
        out = np.zeros(count, dtype)
        assert h.hipMemcpy(out.ctypes.data_as(C.c_void_p), ptr, out.nbytes, 2) == 0
        return out

    k = 1
    while k <= top:
        res = {}
        for on in (False, True):
            mirt.set_ray_grid(on)
            run(intersect, k)
            res[on, 0] = back(d_rec, k, mirt.HIT_DTYPE)
            for m in ORDERED_HITS:
                run(ordered(m), k)
                res[on, m] = back(d_hits, k * m, mirt.HIT_DTYPE).reshape(k, m), back(d_cnt, k, np.int32)
        st = mirt.ray_grid_stats()
        assert st["mode_used"] == mirt.QUERY_BINNED and st["gave_up"] == 0, st
        for m in ORDERED_HITS:
            assert res[True, m][0].tobytes() == res[False, m][0].tobytes() and np.array_equal(res[True, m][1], res[False, m][1]), "the grid disagrees with the sweep"
            hit = res[False, m][1] > 0
            assert np.array_equal(hit, res[False, 0]["index"] >= 0) and res[False, m][0][:, 0][hit].tobytes() == res[False, 0][hit].tobytes(), "slot 0 is not mirt_intersect_device's record"
        mirt.set_ray_grid(False)
        assert h.hipMemcpy(d_rec, behind.ctypes.data_as(C.c_void_p), 20 * k, 1) == 0
        for s in range(8):
            peels(1)(k); mirt.sync()
            assert back(d_rec, k, mirt.HIT_DTYPE).tobytes() == np.ascontiguousarray(res[False, 8][0][:, s]).tobytes(), "peel %d differs from slot %d" % (s, s)
        reps = 5 if k <= 16384 else 3
        ms = {}
        for state in ("off", "built", "kept"):
            mirt.set_ray_grid(state != "off")
            calls = [("int", intersect, fresh)] + [("ord%d" % m, ordered(m), fresh) for m in ORDERED_HITS]
            if state != "built":
                calls += [("peel%d" % m, peels(m), behind) for m in ORDERED_HITS[1:]]
            for name, fn, start in calls:
                ts = [run(fn, k, start, rebuild=state == "built") for _ in range(reps + 1)]
                if state != "off":
                    assert mirt.ray_grid_stats()["source"] == (1 if state == "built" else 2)
                ms[state, name] = float(np.median(ts[1:]))
        mirt.set_ray_grid(False)
        two = float((res[False, 2][1] >= 2).mean())
        print("RESULT ordered n %6d %-10s rays %8d hit %.3f two %.3f eight %.3f  " % (n, which, k, float((res[False, 1][1] > 0).mean()), two, float((res[False, 8][1] == 8).mean()))
              + "  ".join("%s %s" % (state, " ".join("%10.4f" % ms[state, c] for c in ORDERED_COLS[state])) for state in ("off", "built", "kept")) + " ms")
        sys.stdout.flush()
        k = k * 4 if k * 4 <= top or k == top else top
    mirt.shutdown()


ORDERED_COLS = {"off": ("int", "ord1", "ord2", "ord4", "ord8", "peel2", "peel4", "peel8"), "built": ("int", "ord1", "ord2", "ord4", "ord8"),
                "kept": ("int", "ord1", "ord2", "ord4", "ord8", "peel2", "peel4", "peel8")}
ORDERED_ROW = re.compile(r"ordered n\s+(\d+) (\w+)\s+rays\s+(\d+) hit [0-9.]+ two [0-9.]+ eight [0-9.]+  off((?:\s+[0-9.]+){8})  built((?:\s+[0-9.]+){5})  kept((?:\s+[0-9.]+){8}) ms")


def step_ordered(p):
    p("== ordered: mirt_intersect_ordered_device, max_hits 1, 2, 4, 8, after NULL, on the grid section's scenes and ray sets, beside two yardsticks in the")
    p("   same run on the same rays: mirt_intersect_device from fresh records (int), and max_hits in-place peels of the max_hits == 1 call (peelN:")
    p("   N calls with after == hits, one mirt_sync); host clock around call + mirt_sync, medians; answers compared first ==")
    p("three groups: the switch of mirt_set_ray_grid off (columns int ord1 ord2 ord4 ord8 peel2 peel4 peel8); on, the structure built by the call (int ord1 ord2")
    p("ord4 ord8); on, the structure held (as off).  hit / two / eight: the share of rays with a hit, with two or more, with eight or more")
    out = "".join(run_child(p, ["--child", "ordered", str(n), which], {}, 420) for n in (100000, 2000) for which in GRID_SETS)
    ordered_summary(out, p)


def ordered_summary(text, p):
    """Where max_hits == 1 stands against mirt_intersect_device and max_hits == N against N peels, per switch state: the spread of the
    ratios and every cell that is behind by more than the 2 % two runs differ by."""
    rows = []
    for m in ORDERED_ROW.finditer(text):
        v = {}
        for state, g in (("off", 4), ("built", 5), ("kept", 6)):
            v.update({(state, c): float(x) for c, x in zip(ORDERED_COLS[state], m.group(g).split())})
        rows.append((int(m.group(1)), m.group(2), int(m.group(3)), v))
    pairs = [("max_hits 1 against mirt_intersect_device", "ord1", "int", ("off", "built", "kept"))]
    pairs += [("max_hits %d against %d peels" % (m, m), "ord%d" % m, "peel%d" % m, ("off", "kept")) for m in ORDERED_HITS[1:]]
    for what, a, b, states in pairs:
        for state in states:
            ratio = [(v[state, a] / v[state, b], n, w, k, v[state, a], v[state, b]) for n, w, k, v in rows]
            if not ratio:
                continue
            rs = sorted(r[0] for r in ratio)
            behind = [r for r in ratio if r[0] > 1.02]
            p("%s, switch %s: time ratio min %.2f median %.2f max %.2f; behind by more than 2 %% in %d of %d cells" % (what, state, rs[0], rs[len(rs) // 2], rs[-1], len(behind), len(ratio)))
            for r, n, w, k, x, y in behind:
                p("  n %d %s rays %d: %.4f ms against %.4f ms" % (n, w, k, x, y))
    p("")


# ---- every hit along parallel rays: mirt_intersect_ordered_along_device ------------------------------------------------------------------

def child_ordered_along(n):
    """mirt_intersect_ordered_along_device for max_hits 1, 2, 4 and 8 on the along section's grid of starts looking down the scene:
    BINNED with the grid built by the call (a direction never used before: dir tilted by a few subnormals) and with the grid held,
    beside what a caller does today on the same rays written out, in the same run: mirt_intersect_ordered_device with the switch of
    mirt_set_ray_grid off (the sweep) and on with the ray grid held -- and, for max_hits 1, beside mirt_intersect_along_device with
    the grid held.  Answers are compared before any time is taken: every max_hits against the sweep's."""
    import mirt
    h = hip()
    mirt.init(0)
    mirt.scene_upload(mirt.scene_soup(1, n, 0.05 if n >= 50000 else 0.2))
    top = 1 << 20
    down = np.array([0, 0, 1], np.float32)
    fresh = mirt.fresh_hits(top)
    d_starts, d_rays, d_rec = dev_alloc(h, 12 * top), dev_alloc(h, 24 * top), dev_alloc(h, fresh.nbytes, fresh)
    d_hits, d_cnt = dev_alloc(h, 8 * fresh.nbytes), dev_alloc(h, 4 * top)

    def tilted(i):
        d = down.copy()
        d[0] = np.float32(i) * np.finfo(np.float32).smallest_subnormal
        return d

    def run(fn, k):
        t0 = time.perf_counter()
        fn(k); mirt.sync()
        return (time.perf_counter() - t0) * 1e3

    def closest(q):
        assert h.hipMemcpy(d_rec, fresh.ctypes.data_as(C.c_void_p), 20 * q, 1) == 0
        t0 = time.perf_counter()
        mirt.intersect_along_device(down, d_starts, q, d_rec); mirt.sync()
        return (time.perf_counter() - t0) * 1e3

    def back(ptr, count, dtype):
        out = np.zeros(count, dtype)
        assert h.hipMemcpy(out.ctypes.data_as(C.c_void_p), ptr, out.nbytes, 2) == 0
        return out

    k, nudge = 1, 0
    while k <= top:
        starts = along_grid(k)
        rays = mirt.make_rays(starts, down)
        assert h.hipMemcpy(d_starts, starts.ctypes.data_as(C.c_void_p), starts.nbytes, 1) == 0
        assert h.hipMemcpy(d_rays, rays.ctypes.data_as(C.c_void_p), rays.nbytes, 1) == 0
        # the answers first
        counts = {}
        for m in ORDERED_HITS:
            mirt.set_ray_grid(False)
            run(lambda q: mirt.intersect_ordered_device(d_rays, q, None, m, d_hits, d_cnt), k)
            want = back(d_hits, k * m, mirt.HIT_DTYPE), back(d_cnt, k, np.int32)
            mirt.set_query_mode(mirt.QUERY_BINNED)
            run(lambda q: mirt.intersect_ordered_along_device(down, d_starts, q, None, m, d_hits, d_cnt), k)
            st = mirt.along_stats()
            assert st["mode_used"] == mirt.QUERY_BINNED, st
            got = back(d_hits, k * m, mirt.HIT_DTYPE), back(d_cnt, k, np.int32)
            assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]), "the ordered call along a direction disagrees with mirt_intersect_ordered_device"
            counts[m] = want[1]
        reps = 5 if k <= 65536 else 3
        ms = {}
        ms["along"] = float(np.median([closest(k) for _ in range(reps + 2)][2:]))
        assert mirt.along_stats()["cube_source"] == 2
        for m in ORDERED_HITS:
            yard = lambda q: mirt.intersect_ordered_device(d_rays, q, None, m, d_hits, d_cnt)
            mirt.set_ray_grid(False)
            ms[m, "sweep"] = float(np.median([run(yard, k) for _ in range(reps + 1)][1:]))
            mirt.set_ray_grid(True)
            ts = [run(yard, k) for _ in range(reps + 2)]
            gs = mirt.ray_grid_stats()
            ms[m, "grid"] = float(np.median(ts[2:])) if gs["mode_used"] == mirt.QUERY_BINNED and gs["source"] == 2 else float("nan")
            mirt.set_ray_grid(False)
            ts = []
            for _ in range(reps + 1):                    # (never the key of the call before)
                nudge += 1
                ts.append(run(lambda q: mirt.intersect_ordered_along_device(tilted(1 + nudge % 7), d_starts, q, None, m, d_hits, d_cnt), k))
                assert mirt.along_stats()["cube_source"] == 1
            ms[m, "built"] = float(np.median(ts[1:]))
            ts = [run(lambda q: mirt.intersect_ordered_along_device(down, d_starts, q, None, m, d_hits, d_cnt), k) for _ in range(reps + 2)]
            assert mirt.along_stats()["cube_source"] == 2
            ms[m, "kept"] = float(np.median(ts[2:]))
        mirt.set_query_mode(mirt.QUERY_AUTO)
        print("RESULT ordered_along n %6d rays %8d hit %.3f two %.3f eight %.3f  along %10.4f  " % (n, k, float((counts[1] > 0).mean()), float((counts[2] >= 2).mean()),
                                                                                          float((counts[8] == 8).mean()), ms["along"])
              + "  ".join("m%d %s" % (m, " ".join("%10.4f" % ms[m, c] for c in ("sweep", "grid", "built", "kept"))) for m in ORDERED_HITS) + " ms")
        sys.stdout.flush()
        k *= 4
    mirt.shutdown()


ORDERED_ALONG_ROW = re.compile(r"ordered_along n\s+(\d+) rays\s+(\d+) hit [0-9.]+ two [0-9.]+ eight [0-9.]+  along\s+([0-9.]+)  "
                               + "  ".join(r"m%d((?:\s+[0-9.na]+){4})" % m for m in ORDERED_HITS) + " ms")


def step_ordered_along(p):
    p("== ordered_along: mirt_intersect_ordered_along_device, max_hits 1, 2, 4, 8, after NULL, the along section's square grid of starts looking down the")
    p("   scene (dir = +z), beside what a caller does today in the same run on the same rays written out: mirt_intersect_ordered_device with the switch of")
    p("   mirt_set_ray_grid off (sweep) and on with the ray grid held (grid; nan where that grid is not built); host clock around call + mirt_sync, medians;")
    p("   answers compared first ==")
    p("along: mirt_intersect_along_device with the grid held (one hit).  Per max_hits four columns: sweep; grid; BINNED, the grid built by the call; BINNED, the grid held")
    p("hit / two / eight: the share of rays with a hit, with two or more, with eight or more")
    out = "".join(run_child(p, ["--child", "ordered_along", str(n)], {}, 420) for n in (100000, 2000))
    ordered_along_summary(out, p)


def ordered_along_summary(text, p):
    """What the rows say: the cells where the new call is behind a yardstick by more than the 2 % two runs differ by -- with its build
    and with the grid held, against the sweep and against the held ray grid --, max_hits 1 with the grid held against
    mirt_intersect_along_device, and per triangle count and max_hits the ray count from which the call with its build stays ahead
    of the sweep (where AUTO's rule would have to switch when the grid is not held)."""
    rows = []
    for m in ORDERED_ALONG_ROW.finditer(text):
        v = {"along": float(m.group(3))}
        for j, mh in enumerate(ORDERED_HITS):
            v.update({(mh, c): float(x) for c, x in zip(("sweep", "grid", "built", "kept"), m.group(4 + j).split())})
        rows.append((int(m.group(1)), int(m.group(2)), v))
    for mine in ("built", "kept"):
        for yard in ("sweep", "grid"):
            cells = [(n, k, mh, v[mh, mine], v[mh, yard]) for n, k, v in rows for mh in ORDERED_HITS if v[mh, yard] == v[mh, yard]]
            behind = [c for c in cells if c[3] > 1.02 * c[4]]
            ratios = sorted(c[3] / c[4] for c in cells)
            if not cells:
                continue
            p("grid %s against %s: time ratio min %.3f median %.3f max %.3f; behind by more than 2 %% in %d of %d cells"
              % ("built by the call" if mine == "built" else "held", "the sweep" if yard == "sweep" else "the held ray grid", ratios[0], ratios[len(ratios) // 2],
                 ratios[-1], len(behind), len(cells)))
            for n, k, mh, x, y in behind:
                p("  n %d rays %d max_hits %d: %.4f ms against %.4f ms" % (n, k, mh, x, y))
    one = [(n, k, v[1, "kept"], v["along"]) for n, k, v in rows]
    if one:
        rs = sorted(x / y for n, k, x, y in one)
        p("max_hits 1, grid held, against mirt_intersect_along_device: time ratio min %.3f median %.3f max %.3f" % (rs[0], rs[len(rs) // 2], rs[-1]))
        for n, k, x, y in one:
            if x > 1.02 * y:
                p("  n %d rays %d: %.4f ms against %.4f ms" % (n, k, x, y))
    for n in sorted({r[0] for r in rows}, reverse=True):
        for mh in ORDERED_HITS:
            cells = sorted((k, v[mh, "built"] <= v[mh, "sweep"]) for nn, k, v in rows if nn == n)
            lost = [k for k, ahead in cells if not ahead]
            first = min([k for k, _ in cells if not lost or k > max(lost)], default=None)
            p("n %d max_hits %d, grid built by the call: behind the sweep in %d of %d cells; ahead in every cell from %s rays on"
              % (n, mh, len(lost), len(cells), first if first is not None else "no count measured"))
    p("")


# ---- the number of hits along a ray: mirt_count_hits_along_device / mirt_count_hits_device ---------------------------------------------

COUNT_ALONG_COLS = ("cnt_sweep", "cnt_built", "cnt_kept", "ord8_sweep", "ord8_kept", "peel_kept", "occ_kept")
COUNT_RAYS_COLS = ("cnt", "ord8", "peel", "occ")


def count_peel(mirt, h, ordered, k, d_after, d_hits, d_cnt):
    """What a caller did for every hit of a ray before: ordered(after) at max_hits 8, the records and counts read back, each full ray's
    last record copied into `after` on the host and sent back, until no ray is full.  (counts summed per ray, rounds, ms)."""
    hits, cnt = np.zeros((k, 8), mirt.HIT_DTYPE), np.zeros(k, np.int32)
    total, after, rounds = np.zeros(k, np.int64), None, 0
    t0 = time.perf_counter()
    while True:
        if after is not None:
            assert h.hipMemcpy(d_after, after.ctypes.data_as(C.c_void_p), after.nbytes, 1) == 0
        ordered(None if after is None else d_after); mirt.sync()
        assert h.hipMemcpy(cnt.ctypes.data_as(C.c_void_p), d_cnt, cnt.nbytes, 2) == 0
        total += cnt
        rounds += 1
        full = cnt == 8
        if not full.any():
            break
        assert h.hipMemcpy(hits.ctypes.data_as(C.c_void_p), d_hits, hits.nbytes, 2) == 0
        after = mirt.fresh_hits(k)                                  # (a fresh record admits nothing: an exhausted ray stays exhausted)
        after[full] = hits[full, 7]
    return total, rounds, (time.perf_counter() - t0) * 1e3


def child_count(n, which):
    """which == "along": mirt_count_hits_along_device on the along section's grid of starts looking down the scene -- BRUTE, BINNED with
    the grid built by the call (a direction never used before: dir tilted by a few subnormals) and with the grid held --; otherwise
    mirt_count_hits_device on the grid section's ray set `which`.  Beside each, in the same run on the same rays: ONE ordered call at
    max_hits 8, the peels of count_peel, and one occlusion call without limits.  Answers are compared before any time is taken."""
    import mirt
    h = hip()
    mirt.init(0)
    tris = mirt.scene_soup(1, n, 0.05 if n >= 50000 else 0.2)
    mirt.scene_upload(tris)
    along = which == "along"
    down = np.array([0, 0, 1], np.float32)
    all_rays = None if along else grid_rays(mirt, h, tris, which, 1 << 20)
    top = 1 << 20 if along else len(all_rays)
    d_in = dev_alloc(h, (12 if along else 24) * top)
    d_after, d_hits, d_cnt, d_occ = dev_alloc(h, 20 * top), dev_alloc(h, 160 * top), dev_alloc(h, 4 * top), dev_alloc(h, top)

    def tilted(i):
        d = down.copy()
        d[0] = np.float32(i) * np.finfo(np.float32).smallest_subnormal
        return d

    def run(fn):
        t0 = time.perf_counter()
        fn(); mirt.sync()
        return (time.perf_counter() - t0) * 1e3

    def back(ptr, count, dtype):
        out = np.zeros(count, dtype)
        assert h.hipMemcpy(out.ctypes.data_as(C.c_void_p), ptr, out.nbytes, 2) == 0
        return out

    k, nudge = 1, 0
    while k <= top:
        src = along_grid(k) if along else np.ascontiguousarray(all_rays[:k])
        assert h.hipMemcpy(d_in, src.ctypes.data_as(C.c_void_p), src.nbytes, 1) == 0
        if along:
            count = lambda d=down: mirt.count_hits_along_device(d, d_in, k, None, None, d_cnt)
            ordered = lambda a=None: mirt.intersect_ordered_along_device(down, d_in, k, a, 8, d_hits, d_cnt)
            occluded = lambda: mirt.occluded_along_device(down, d_in, k, None, d_occ)
        else:
            count = lambda: mirt.count_hits_device(d_in, k, None, None, d_cnt)
            ordered = lambda a=None: mirt.intersect_ordered_device(d_in, k, a, 8, d_hits, d_cnt)
            occluded = lambda: mirt.occluded_device(d_in, k, None, d_occ)
        # the answers first: the count under every mode, the peels' sum, min(count, 8), count > 0
        mirt.set_query_mode(mirt.QUERY_BRUTE)
        run(count)
        want = back(d_cnt, k, np.int32)
        if along:
            mirt.set_query_mode(mirt.QUERY_BINNED)
            run(count)
            assert mirt.along_stats()["mode_used"] == mirt.QUERY_BINNED, mirt.along_stats()
            assert np.array_equal(back(d_cnt, k, np.int32), want), "the binned count disagrees with the sweep"
        total, rounds, _ = count_peel(mirt, h, ordered, k, d_after, d_hits, d_cnt)
        assert np.array_equal(total, want), "the peels enumerate other numbers than the count"
        run(ordered)
        assert np.array_equal(back(d_cnt, k, np.int32), np.minimum(want, 8))
        run(occluded)
        assert np.array_equal(back(d_occ, k, np.uint8) == 1, want > 0)
        reps = 5 if k <= 65536 else 3
        med = lambda fn, warm=2: float(np.median([run(fn) for _ in range(reps + warm)][warm:]))
        ms = {}
        if along:
            mirt.set_query_mode(mirt.QUERY_BRUTE)
            ms["cnt_sweep"], ms["ord8_sweep"] = med(count, 1), med(ordered, 1)
            mirt.set_query_mode(mirt.QUERY_BINNED)
            ts = []
            for _ in range(reps + 1):                    # (never the key of the call before)
                nudge += 1
                ts.append(run(lambda: count(tilted(1 + nudge % 7))))
                assert mirt.along_stats()["cube_source"] == 1
            ms["cnt_built"] = float(np.median(ts[1:]))
            ms["cnt_kept"] = med(count)
            assert mirt.along_stats()["cube_source"] == 2
            ms["ord8_kept"], ms["occ_kept"] = med(ordered), med(occluded)
            ms["peel_kept"] = float(np.median([count_peel(mirt, h, ordered, k, d_after, d_hits, d_cnt)[2] for _ in range(reps)]))
            cols = COUNT_ALONG_COLS
        else:
            ms["cnt"], ms["ord8"], ms["occ"] = med(count, 1), med(ordered, 1), med(occluded, 1)
            ms["peel"] = float(np.median([count_peel(mirt, h, ordered, k, d_after, d_hits, d_cnt)[2] for _ in range(reps)]))
            cols = COUNT_RAYS_COLS
        mirt.set_query_mode(mirt.QUERY_AUTO)
        print("RESULT count n %6d %-10s rays %8d hit %.3f above8 %.3f most %3d rounds %2d  " % (n, which, k, float((want > 0).mean()), float((want > 8).mean()), int(want.max()), rounds)
              + " ".join("%s %10.4f" % (c, ms[c]) for c in cols) + " ms")
        sys.stdout.flush()
        k = k * 4 if k * 4 <= top or k == top else top
    mirt.shutdown()


COUNT_ROW = re.compile(r"count n\s+(\d+) (\w+)\s+rays\s+(\d+) hit [0-9.]+ above8 [0-9.]+ most\s+\d+ rounds\s+\d+  ((?:\w+\s+[0-9.]+ ?)+) ms")


def step_count(p):
    p("== count: mirt_count_hits_along_device on the along section's square grid of starts looking down the scene (dir = +z) and mirt_count_hits_device on the grid")
    p("   section's ray sets, no `after`, no limits, beside what a caller did before for the same numbers in the same run on the same rays: peels of")
    p("   mirt_intersect_ordered_along_device / mirt_intersect_ordered_device at max_hits 8 through host memory until no ray is full (peel), ONE such call (ord8),")
    p("   and one mirt_occluded*_device call (occ: the floor of a walk that may stop early); host clock around call + mirt_sync, medians; answers compared first ==")
    p("along rows: cnt_sweep / ord8_sweep under MIRT_QUERY_BRUTE; cnt_built: BINNED, the grid built by the call; *_kept: BINNED, the grid held.  Ray rows: the sweep")
    p("(mirt_set_ray_grid off).  hit / above8: the share of rays with a hit, with more than eight; most: the most hits of a ray; rounds: the calls the peels need")
    out = "".join(run_child(p, ["--child", "count", str(n), which], {}, 420) for n in (100000, 2000) for which in ("along",) + GRID_SETS)
    count_summary(out, p)


def count_summary(text, p):
    """The expectation to confirm or refute: one count call is not behind one max_hits 8 ordered call in any cell (2 % is what two runs
    differ by).  Then the count against the peels it replaces and against the occlusion call."""
    rows = []
    for m in COUNT_ROW.finditer(text):
        f = m.group(4).split()
        rows.append((int(m.group(1)), m.group(2), int(m.group(3)), dict(zip(f[0::2], map(float, f[1::2])))))
    pairs = (("cnt_sweep", "ord8_sweep", "along, the sweep"), ("cnt_kept", "ord8_kept", "along, the grid held"), ("cnt", "ord8", "arbitrary rays, the sweep"))
    for mine, yard, what in pairs:
        cells = [(n, w, k, v[mine], v[yard]) for n, w, k, v in rows if mine in v]
        if not cells:
            continue
        behind = [c for c in cells if c[3] > 1.02 * c[4]]
        rs = sorted(c[3] / c[4] for c in cells)
        p("%s: one count call against one max_hits 8 call: time ratio min %.3f median %.3f max %.3f; behind by more than 2 %% in %d of %d cells"
          % (what, rs[0], rs[len(rs) // 2], rs[-1], len(behind), len(cells)))
        for n, w, k, x, y in behind:
            p("  n %d %s rays %d: %.4f ms against %.4f ms" % (n, w, k, x, y))
    for mine, yard, what in (("cnt_kept", "peel_kept", "along, the grid held, against the peels"), ("cnt", "peel", "arbitrary rays, against the peels"),
                             ("cnt_kept", "occ_kept", "along, the grid held, against the occlusion call"), ("cnt", "occ", "arbitrary rays, against the occlusion call"),
                             ("cnt_built", "cnt_sweep", "along, the grid built by the call against the sweep")):
        rs = sorted(v[mine] / v[yard] for n, w, k, v in rows if mine in v)
        if rs:
            p("%s: time ratio min %.3f median %.3f max %.3f" % (what, rs[0], rs[len(rs) // 2], rs[-1]))
    for n in sorted({r[0] for r in rows}, reverse=True):
        cells = sorted((k, v["cnt_built"] <= v["cnt_sweep"]) for nn, w, k, v in rows if nn == n and "cnt_built" in v)
        lost = [k for k, ahead in cells if not ahead]
        first = min([k for k, _ in cells if not lost or k > max(lost)], default=None)
        if cells:
            p("n %d, along, grid built by the call: behind the sweep in %d of %d cells; ahead in every cell from %s rays on (AUTO is along's rule, unchanged)"
              % (n, len(lost), len(cells), first if first is not None else "no count measured"))
    p("")


# ---- several directions in one call: mirt_intersect_alongs_device / mirt_occluded_alongs_device ------------------------------------------

ALONGS_K = (1, 4, 15, 16, 32, 64)
ALONGS_RAYS = (64, 256, 1024, 4096, 16384, 65536)             # rays per direction
ALONGS_BRUTE_CAP = 1.0e11                                     # rays x triangles from which the brute yardstick is timed once, not thrice


def alongs_directions(K):
    """K directions looking down the scene, up to 35 degrees off +z, seeded."""
    rng = np.random.default_rng(13)
    d = np.ones((K, 3), np.float32)
    d[:, 0:2] = rng.uniform(-0.7, 0.7, (K, 2))
    d[0] = (0.0, 0.0, 1.0)
    return np.ascontiguousarray(d)


def child_alongs(n, only_k):
    """One scene and one K: every ray count, closest hits and occlusion (no limits).  N points x K directions, ray i = point i // K
    along direction i % K, so the lanes of a wave mix the directions.  The yardsticks on the same rays in the same run, after all
    answers were found equal: (a) K mirt_*_along_device calls over the rays sorted by direction -- `fresh`: directions never seen,
    every call builds; `again`: the list repeated, where the one kept grid serves K = 1 and is evicted K times a round otherwise --,
    (b) mirt_intersect_device / mirt_occluded_device.  The new call with its groups built by the call (directions never seen) and
    with them held."""
    import mirt
    h = hip()
    mirt.init(0)
    mirt.scene_upload(mirt.scene_soup(1, n, 0.05 if n >= 50000 else 0.2))
    top = ALONGS_K[-1] * ALONGS_RAYS[-1]
    fresh = mirt.fresh_hits(top)
    d_starts, d_sorted, d_rays, d_of = dev_alloc(h, 12 * top), dev_alloc(h, 12 * top), dev_alloc(h, 24 * top), dev_alloc(h, 4 * top)
    d_hits, d_occ = dev_alloc(h, fresh.nbytes, fresh), dev_alloc(h, top)
    at = lambda ptr, off: C.c_void_p(ptr.value + int(off))
    variant = [0]

    def run(fn, total):
        assert h.hipMemcpy(d_hits, fresh.ctypes.data_as(C.c_void_p), 20 * total, 1) == 0
        t0 = time.perf_counter()
        fn(); mirt.sync()
        return (time.perf_counter() - t0) * 1e3

    def median_of(fn, total, reps, warm=1):
        return float(np.median([run(fn, total) for _ in range(reps + warm)][warm:]))

    for K in (only_k,):
        dirs = alongs_directions(K)
        for R in ALONGS_RAYS:
            total = K * R
            grid = along_grid(R)
            starts = np.ascontiguousarray(np.repeat(grid, K, axis=0))
            of = np.ascontiguousarray(np.tile(np.arange(K, dtype=np.int32), R))
            rays = mirt.make_rays(starts, dirs[of])
            by_dir = np.ascontiguousarray(np.tile(grid, (K, 1)))             # direction k's starts at [k R, (k + 1) R)
            for dst, src in ((d_starts, starts), (d_sorted, by_dir), (d_rays, rays), (d_of, of)):
                assert h.hipMemcpy(dst, src.ctypes.data_as(C.c_void_p), src.nbytes, 1) == 0

            def singles(kind, D):
                for k in range(K):
                    if kind == "intersect":
                        mirt.intersect_along_device(D[k], at(d_sorted, 12 * k * R), R, at(d_hits, 20 * k * R))
                    else:
                        mirt.occluded_along_device(D[k], at(d_sorted, 12 * k * R), R, None, at(d_occ, k * R))

            def unseen():
                """The list with other bits in every direction (a dyadic factor: the geometry stays), never the key of a call before."""
                variant[0] += 1
                return np.ascontiguousarray(dirs * np.float32(1.0 + variant[0] / 4096.0))

            calls = {
                "intersect": (lambda: mirt.intersect_device(d_rays, total, d_hits), lambda D: mirt.intersect_alongs_device(D, d_of, d_starts, total, d_hits)),
                "occluded": (lambda: mirt.occluded_device(d_rays, total, None, d_occ), lambda D: mirt.occluded_alongs_device(D, d_of, d_starts, total, None, d_occ)),
            }
            # the answers first: (b), the new call and (a) agree on every ray
            want, got = np.zeros(total, mirt.HIT_DTYPE), np.zeros(total, mirt.HIT_DTYPE)
            wocc, gocc = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
            ms = {}
            ms["intersect", "brute"] = run(calls["intersect"][0], total)
            assert h.hipMemcpy(want.ctypes.data_as(C.c_void_p), d_hits, want.nbytes, 2) == 0
            ms["occluded", "brute"] = run(calls["occluded"][0], total)
            assert h.hipMemcpy(wocc.ctypes.data_as(C.c_void_p), d_occ, total, 2) == 0
            mirt.set_query_mode(mirt.QUERY_BINNED)
            run(lambda: calls["intersect"][1](dirs), total)
            st = mirt.along_stats()
            assert st["mode_used"] == mirt.QUERY_BINNED, st
            assert h.hipMemcpy(got.ctypes.data_as(C.c_void_p), d_hits, got.nbytes, 2) == 0
            run(lambda: calls["occluded"][1](dirs), total)
            assert h.hipMemcpy(gocc.ctypes.data_as(C.c_void_p), d_occ, total, 2) == 0
            assert got.tobytes() == want.tobytes() and np.array_equal(gocc, wocc), "the call of several directions disagrees with mirt_intersect_device / mirt_occluded_device"
            run(lambda: singles("intersect", dirs), total)
            assert h.hipMemcpy(got.ctypes.data_as(C.c_void_p), d_hits, got.nbytes, 2) == 0
            run(lambda: singles("occluded", dirs), total)
            assert h.hipMemcpy(gocc.ctypes.data_as(C.c_void_p), d_occ, total, 2) == 0
            back = np.arange(total).reshape(R, K).T.ravel()                  # sorted position -> the ray it is
            assert got.tobytes() == want[back].tobytes() and np.array_equal(gocc, wocc[back]), "the single-direction calls disagree with mirt_intersect_device / mirt_occluded_device"
            reps = 5 if total <= 65536 else 3
            for name, (brute, alongs) in calls.items():
                mirt.set_query_mode(mirt.QUERY_AUTO)
                if float(total) * n <= ALONGS_BRUTE_CAP:
                    ms[name, "brute"] = median_of(brute, total, reps)
                mirt.set_query_mode(mirt.QUERY_BINNED)
                ms[name, "fresh"] = median_of(lambda: singles(name, unseen()), total, reps)
                ms[name, "again"] = median_of(lambda: singles(name, dirs), total, reps, warm=2)
                ms[name, "built"] = median_of(lambda: alongs(unseen()), total, reps)
                assert mirt.along_stats()["cube_source"] == 1
                ms[name, "held"] = median_of(lambda: alongs(dirs), total, reps, warm=2)
                assert mirt.along_stats()["cube_source"] == 2         # (at most five passes: every group is kept)
            mirt.set_query_mode(mirt.QUERY_AUTO)
            print("RESULT alongs n %6d K %2d rays %6d B %3d hit %.3f  " % (n, K, R, st["cube_bins"], float((want["index"] >= 0).mean()))
                  + "  ".join("%s %s" % (name, " ".join("%10.4f" % ms[name, m] for m in ("brute", "fresh", "again", "built", "held"))) for name in ("intersect", "occluded")) + " ms")
            sys.stdout.flush()
    mirt.shutdown()


ALONGS_ROW = re.compile(r"alongs n\s+(\d+) K\s+(\d+) rays\s+(\d+) B\s+\d+ hit [0-9.]+  intersect((?:\s+[0-9.]+){5})  occluded((?:\s+[0-9.]+){5}) ms")


def step_alongs(p):
    p("== alongs: mirt_intersect_alongs_device / mirt_occluded_alongs_device, N points (a square grid looking down the scene) x K directions up to 35 degrees")
    p("   off +z, ray i = point i / K along direction i % K; `rays` is N, the rays per direction (host clock around call + mirt_sync, medians) ==")
    p("five columns each: (b) mirt_intersect_device / mirt_occluded_device; (a) K mirt_*_along_device calls over the rays sorted by direction, BINNED,")
    p("directions never seen (`fresh`: every call builds) and the list repeated (`again`: K = 1 finds its grid held, K > 1 evicts it K times a round);")
    p("the new call, BINNED, its groups built by the call and held.  All answers were compared first.  (b) beyond %.0e rays x triangles: one timing, not a median" % ALONGS_BRUTE_CAP)
    out = "".join(run_child(p, ["--child", "alongs", str(n), str(K)], {}, 300) for n in (100000, 2000) for K in ALONGS_K)
    alongs_summary(out, p)


def alongs_summary(text, p):
    """What the rows say: the cells where the new call is behind either yardstick by more than the 2 % two runs differ by -- built
    by the call against (b) and (a) fresh, held against (b) and (a) again --, and per triangle count and kind the total ray count
    from which the call with its builds stays ahead of (b): where AUTO's rule has to switch when the groups are not held."""
    rows = []
    for m in ALONGS_ROW.finditer(text):
        rows.append((int(m.group(1)), int(m.group(2)), int(m.group(3)), {"intersect": [float(x) for x in m.group(4).split()], "occluded": [float(x) for x in m.group(5).split()]}))
    behind = {("built", "b"): [], ("built", "a"): [], ("held", "b"): [], ("held", "a"): []}
    for n, K, R, v in rows:
        for what, t in v.items():
            brute, fresh, again, built, held = t
            for key, mine, yard in ((("built", "b"), built, brute), (("built", "a"), built, fresh), (("held", "b"), held, brute), (("held", "a"), held, again)):
                if mine > 1.02 * yard:
                    behind[key].append("n %d K %d rays %d %s: %.4f against %.4f ms" % (n, K, R, what, mine, yard))
    names = {"b": "(b) the brute-force call", "a": "(a) K single-direction calls"}
    for (mode, yard), cells in behind.items():
        p("the new call, groups %s, behind %s by more than 2 %% in %d of %d cells%s" % (mode, names[yard], len(cells), 2 * len(rows), ": " + "; ".join(cells) if cells else ""))
    wave = 4096
    for n in sorted({r[0] for r in rows}, reverse=True):
        for what in ("intersect", "occluded"):
            cells = [(K * R, v[what][3] <= v[what][0], v[what][4] <= v[what][0]) for nn, K, R, v in rows if nn == n]
            small, large = [c for c in cells if c[0] <= wave], [c for c in cells if c[0] > wave]
            p("n %d %s against (b): built ahead in %d of %d cells of at most %d rays in all and in %d of %d beyond; held ahead in %d of %d and %d of %d"
              % (n, what, sum(c[1] for c in small), len(small), wave, sum(c[1] for c in large), len(large),
                 sum(c[2] for c in small), len(small), sum(c[2] for c in large), len(large)))
    p("AUTO's rule (auto_bins_fans: more than MIRT_QUERY_WAVE_RAYS = 4096 rays in all on a scene the fans bin, or every group held) is read off the two lines")
    p("per scene above: it stands where `built` loses at most 4096 rays and wins beyond, and `held` wins; DESIGN.md section 5.1 states what these rows gave.")
    p("")


# ---- shadow masks: mirt_shadow_mask_device and mirt_direct_light_masked_device beside mirt_direct_light_device ------------------------

MASK_SETS = ((1, 1), (2, 1), (2, 16), (4, 16), (16, 16))      # lights x samples: 1, 2, 32, 64 and 256 positions
MASK_RECORDS = tuple(1 << e for e in range(10, 22))
MASK_BRUTE_CAP = 2.0e11                                       # records x positions x triangles a BRUTE cell may cost (0.2 - 0.5 s a call)
HBM_PEAK = 8.0e12                                             # bytes per second (MI355X: 8 TB/s)


def mask_lights(nl, samples):
    """nl lights inside the scene's box -- the first the default light -- and their samples' jittered positions (None for hard shadows)."""
    import mirt
    rng = np.random.default_rng(11)
    L = np.zeros((nl, 7), np.float32)
    L[:, 0:3] = rng.uniform(-0.75, 0.75, (nl, 3))
    L[:, 3:6] = rng.choice(np.array([0.25, 0.5, 0.75, 1.0], np.float32), (nl, 3))
    L[:, 6] = rng.integers(3, 15, nl)
    L[0] = np.asarray(mirt.DEFAULT_LIGHT, np.float32).reshape(-1, 7)[0]
    jit = None
    if samples > 1:
        jit = (np.repeat(L[:, 0:3], samples, axis=0) + rng.uniform(-0.05, 0.05, (nl * samples, 3))).astype(np.float32)
    return L, jit


def mask_cell(mirt, d_hits, k, L, d_rgb, d_mask, d_rgb2, reps):
    """The three calls in turn, `reps` rounds after one unmeasured round: median ms of each."""
    calls = (lambda: mirt.direct_light_device(d_hits, k, L, d_rgb), lambda: mirt.shadow_mask_device(d_hits, k, L, d_mask),
             lambda: mirt.direct_light_masked_device(d_hits, k, L, d_mask, d_rgb2))
    ts = [[], [], []]
    for r in range(reps + 1):
        for i, fn in enumerate(calls):
            t0 = time.perf_counter()
            fn(); mirt.sync()
            if r:
                ts[i].append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(t)) for t in ts]


def child_mask(mode, n, spread):
    """One scene and one mode: every light set x every record count (spread: one cell, measured seven times over)."""
    import mirt
    h = hip()
    mirt.init(0)
    d_hits, count = closest_records(mirt, h, n, 0.05 if n >= 50000 else 0.2)
    top = MASK_RECORDS[-1]
    rec = np.zeros(count, mirt.HIT_DTYPE)
    assert h.hipMemcpy(rec.ctypes.data_as(C.c_void_p), d_hits, rec.nbytes, 2) == 0
    rec = rec[np.random.default_rng(5).permutation(count)]     # (a small call samples the whole frame)
    rec = np.ascontiguousarray(np.concatenate([rec, rec[:top - count]]))     # 1080p is 23 552 records short of 2^21
    h.hipFree(d_hits)
    d_hits = dev_alloc(h, rec.nbytes, rec)
    d_rgb, d_rgb2, d_mask = dev_alloc(h, top * 12), dev_alloc(h, top * 12), dev_alloc(h, top * 4 * 8)
    a, b = np.zeros((top, 3), np.float32), np.zeros((top, 3), np.float32)
    mirt.set_query_mode(mirt.QUERY_BRUTE if mode == "brute" else mirt.QUERY_BINNED)
    for nl, samples in (((2, 16),) if spread else MASK_SETS):
        L, jit = mask_lights(nl, samples)
        mirt.set_soft_shadows(samples, jit)
        npos = nl * samples
        for k in ((1 << 18,) * 7 if spread else MASK_RECORDS):
            if mode == "brute" and float(k) * npos * n > MASK_BRUTE_CAP:
                print("RESULT mask n %6d mode %-6s positions %3d records %8d  not measured: beyond %.0e row tests" % (n, mode, npos, k, MASK_BRUTE_CAP))
                continue
            dl, mk, rl = mask_cell(mirt, d_hits, k, L, d_rgb, d_mask, d_rgb2, 5 if k <= 65536 else 3)
            st, sm = mirt.query_stats(), mirt.shadow_mask_stats()
            assert st["mode_used"] == sm["mode_used"] and (mode == "brute" or (st["cube_source"] == 2 and sm["cube_source"] == 2)), (st, sm)
            # the answers: mask, then relight, is mirt_direct_light_device
            assert h.hipMemcpy(a.ctypes.data_as(C.c_void_p), d_rgb, k * 12, 2) == 0 and h.hipMemcpy(b.ctypes.data_as(C.c_void_p), d_rgb2, k * 12, 2) == 0
            assert np.array_equal(a[:k].view(np.uint32), b[:k].view(np.uint32)), "mask + relight differs from mirt_direct_light_device"
            moved = k * (20 + 4 * mirt.mask_words(npos) + 12 + 60)
            print("RESULT mask n %6d mode %-6s positions %3d records %8d  direct_light %10.4f  shadow_mask %10.4f  masked %8.4f ms  masked: %.0f MB, %4.1f %% of HBM peak"
                  % (n, mode, npos, k, dl, mk, rl, moved / 1e6, 100.0 * moved / (rl * 1e-3) / HBM_PEAK))
            sys.stdout.flush()
    mirt.set_soft_shadows(1)
    mirt.shutdown()


MASK_ROW = re.compile(r"mask n\s+(\d+) mode (\S+)\s+positions\s+(\d+) records\s+(\d+)  direct_light\s+([0-9.]+)  shadow_mask\s+([0-9.]+)  masked\s+([0-9.]+) ms")


def step_mask(p):
    p("== mask: mirt_shadow_mask_device and mirt_direct_light_masked_device beside mirt_direct_light_device -- the same records, lights and cubes, "
      "the three calls in turn (host clock around call + mirt_sync, medians) ==")
    p("records: the closest hits of the scene's 1080p primary rays in a fixed shuffled order; positions 1, 2: hard lights, 32, 64, 256: 2, 4, 16 lights x 16 samples; "
      "binned: BINNED with every cube held; masked: bytes the call must move (20 record + 4 per plane + 12 out + 60 triangle row, per record) over its time")
    out = run_child(p, ["--child", "mask", "binned", "100000", "spread"], {}, 300)
    rows = [tuple(float(x) for x in m.groups()[4:]) for m in MASK_ROW.finditer(out)]
    spread = max((max(c) - min(c)) / float(np.median(c)) for c in zip(*rows)) if rows else 0.0
    p("run-to-run spread of the cell above (seven measurements of n 100000, 32 positions, 2^18 records, binned): the medians of a call differ by up to %.1f %% of their median" % (100 * spread))
    p("")
    for n in (100000, 2000):
        for mode in ("brute", "binned"):
            out += run_child(p, ["--child", "mask", mode, str(n), "grid"], {}, 400)
    cells = {}
    for m in MASK_ROW.finditer(out):
        cells[(int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4)))] = tuple(float(x) for x in m.groups()[4:])
    behind = ["n %d %s, %d positions, %d records: %.4f against %.4f ms" % (k + (v[1], v[0])) for k, v in sorted(cells.items()) if v[1] > (1 + spread) * v[0]]
    p("")
    p("mirt_shadow_mask_device behind mirt_direct_light_device by more than the spread (%.1f %%) in %d of %d cells: %s" % (100 * spread, len(behind), len(cells), "; ".join(behind) or "nowhere"))
    worst = max(cells.items(), key=lambda kv: kv[1][1] / kv[1][0])
    ahead = [1 - v[1] / v[0] for v in cells.values()]
    p("its largest deficit: %.1f %% (n %d %s, %d positions, %d records: %.4f against %.4f ms); ahead in %d cells, by %.1f %% in the median and %.1f %% at most"
      % ((100 * (worst[1][1] / worst[1][0] - 1),) + worst[0] + (worst[1][1], worst[1][0], sum(a > 0 for a in ahead), 100 * float(np.median(ahead)), 100 * max(ahead))))
    ratios = [v[0] / v[2] for v in cells.values()]
    p("mirt_direct_light_device / mirt_direct_light_masked_device: %.1f .. %.1f, median %.1f" % (min(ratios), max(ratios), float(np.median(ratios))))
    # AUTO decides between the modes by mirt_direct_light's rule: does the faster mode of a cell differ between the two calls?
    differ = ["n %d, %d positions, %d records" % (n, q, k) for (n, mode, q, k), v in sorted(cells.items())
              if mode == "brute" and (n, "binned", q, k) in cells and (v[0] < cells[(n, "binned", q, k)][0]) != (v[1] < cells[(n, "binned", q, k)][1])]
    p("cells where the faster of BRUTE and BINNED-held is one mode for mirt_direct_light_device and the other for mirt_shadow_mask_device: %s" % ("; ".join(differ) or "none"))
    p("")


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


def step_throughput(p, expected):
    p("== throughput: the primary rays of soup100k at 1080p, lane per ray, beside the BRUTE frame of the same view ==")
    out = run_child(p, ["--child", "throughput"], {"MIRT_QUERY_WAVE_RAYS": "0"}, 300)
    m = re.search(r"measured_ratio query/brute\(primary only\) = ([0-9.]+)", out)
    if m and expected:
        p("expected_ratio (static issue cycles per test) = %.2f; measured / expected = %.2f" % (expected, float(m.group(1)) / expected))
    p("")


def step_sweep(p):
    p("== sweep: ms per mirt_intersect_device call (host clock around call + mirt_sync, median) ==")
    table = {}
    for n in (100000, 2000):
        for knob in ("0", HUGE):
            out = run_child(lambda s: None, ["--child", "sweep", str(n)], {"MIRT_QUERY_WAVE_RAYS": knob}, 420)
            for m in re.finditer(r"RESULT n\s+(\d+) knob (\S+)\s+rays\s+(\d+)\s+([0-9.]+) ms", out):
                table[(int(m.group(1)), m.group(2), int(m.group(3)))] = float(m.group(4))
    for n in (100000, 2000):
        p("n = %d triangles" % n)
        p("%10s %14s %14s   faster" % ("rays", "lane per ray", "wave per ray"))
        k, cross = 1, None
        while (n, "0", k) in table:
            a, b = table[(n, "0", k)], table[(n, HUGE, k)]
            p("%10d %11.4f ms %11.4f ms   %s" % (k, a, b, "wave" if b < a else "lane"))
            if b < a:
                cross = k
            k *= 2
        p("largest batch where a wave per ray is faster: %s rays" % cross)
        p("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_query_bench.txt"))
    ap.add_argument("--steps", default="issue,occupancy,throughput,sweep,directlight")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--child", nargs="+")
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "directlight":
            return child_directlight(a.child[1])
        if a.child[0] == "dlsweep":
            return child_dlsweep(a.child[1], int(a.child[2]))
        if a.child[0] == "fan":
            return child_fan(a.child[1])
        if a.child[0] == "fansweep":
            return child_fansweep(a.child[1], int(a.child[2]))
        if a.child[0] == "fans":
            return child_fans(int(a.child[1]))
        if a.child[0] == "occsweep":
            return child_occsweep(int(a.child[1]))
        if a.child[0] == "occfans":
            return child_occfans(int(a.child[1]))
        if a.child[0] == "along":
            return child_along(int(a.child[1]))
        if a.child[0] == "grid":
            return child_grid(int(a.child[1]), a.child[2])
        if a.child[0] == "ordered":
            return child_ordered(int(a.child[1]), a.child[2])
        if a.child[0] == "ordered_along":
            return child_ordered_along(int(a.child[1]))
        if a.child[0] == "count":
            return child_count(int(a.child[1]), a.child[2])
        if a.child[0] == "alongs":
            return child_alongs(int(a.child[1]), int(a.child[2]))
        if a.child[0] == "mask":
            return child_mask(a.child[1], int(a.child[2]), a.child[3] == "spread")
        return child_throughput() if a.child[0] == "throughput" else child_sweep(int(a.child[1]))
    lines = []

    def p(s):
        print(s)
        sys.stdout.flush()
        lines.append(s)
    steps = a.steps.split(",")
    expected = step_issue(p) if "issue" in steps else None
    if "occupancy" in steps:
        step_occupancy(p)
    try:
        if "throughput" in steps:
            step_throughput(p, expected)
        if "sweep" in steps:
            step_sweep(p)
        if "directlight" in steps:
            step_directlight(p)
        if "fan" in steps:
            step_fan(p)
        if "fans" in steps:
            step_fans(p)
        if "occluded" in steps:
            step_occluded(p)
        if "mask" in steps:
            step_mask(p)
        if "along" in steps:
            step_along(p)
        if "alongs" in steps:
            step_alongs(p)
        if "grid" in steps:
            step_grid(p)
        if "ordered" in steps:
            step_ordered(p)
        if "ordered_along" in steps:
            step_ordered_along(p)
        if "count" in steps:
            step_count(p)
    finally:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
