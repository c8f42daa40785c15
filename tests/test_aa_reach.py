"""tests/cpp/aa_reach_test.cpp on the CPU: the float chain of a pixel's sub-ray coordinates ends a few ulp beyond the half pixel at 4,
6, 7 and 8 samples (never at 2, 3 and 5); a supersampled camera frame pads its bins, and the tile kernel its rectangles, by exactly
half a pixel; the slivers that begin inside that gap are kept by the edge-function margin alone, which is 20 times and more what
they need.  The program measures the chain itself; the slivers it checks are written here: those of tests/supersampling.py (the
scenes test_gpu_supersampling.py renders) in two poses, and slivers at the chain's worst coordinates below 23 000 on frames as wide
or as high as those coordinates need."""
import os
import re
import subprocess

import numpy as np

import supersampling as ss
from ref_cases import aa_overshoot, sliver_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 23000                      # the largest frame side frame_fits_binning (capi/pass_plan.hpp) accepts


def worst_coordinates(samples):
    """(largest overshoot in pixels, largest in ulps of the coordinate, largest among the last columns of an 8-pixel bin)."""
    c = np.arange(LIMIT + 1)
    ov = aa_overshoot(c, samples)
    ulps = ov / np.spacing((c + 0.5).astype(np.float32)).astype(np.float64)
    last8 = np.where(c % 8 == 7, ov, 0.0)
    return int(np.argmax(ov)), int(np.argmax(ulps)), int(np.argmax(last8))


def records(oracle):
    out = []

    def add(kind, samples, W, H, focal, cam, rot, tris, cols, rows):
        for k, c in enumerate(list(cols) + list(rows)):
            axis = 0 if k < len(cols) else 1
            ov = max(float(aa_overshoot(c, samples)), float(aa_overshoot(c, samples, (H if axis else W) / 2.0)))
            f = [kind, samples, W, H, "%.9g" % focal] + ["%.9g" % v for v in cam] + ["%.9g" % v for v in rot] + [axis, c, "%.17g" % ov]
            out.append(" ".join(str(v) for v in f + ["%.9g" % v for v in tris[2 + k, 0:9]]))

    for samples in ss.SLIVER_SAMPLES:
        for yaw in (0.0, ss.SLIVER_YAW):
            c = ss.sliver_case(oracle, samples, yaw=yaw)
            add("D", samples, ss.SLIVER_W, ss.SLIVER_H, ss.SLIVER_FOCAL, ss.SLIVER_CAM, c["rot"], c["tris"], c["cols"], c["rows"])
        for c in sorted(set(worst_coordinates(samples))):
            size = min(LIMIT, (c + 8) // 8 * 8)                   # the coordinate's bin is the frame's last
            for yaw in (0.0, ss.SLIVER_YAW):
                rot = oracle.rot_from_yaw(yaw, 1.0) if yaw else ss.identity()
                t, cols, rows = sliver_scene(samples, size, 72, size / 2.0, ss.SLIVER_CAM, rot, [c], [])
                add("W", samples, size, 72, size / 2.0, ss.SLIVER_CAM, rot, t, cols, rows)
                t, cols, rows = sliver_scene(samples, 96, size, size / 2.0, ss.SLIVER_CAM, rot, [], [c])
                add("W", samples, 96, size, size / 2.0, ss.SLIVER_CAM, rot, t, cols, rows)
    return out


def test_half_pixel_pad_is_covered_by_the_edge_margin(oracle, tmp_path):
    exe, data = str(tmp_path / "aa_reach_test"), str(tmp_path / "slivers.txt")
    with open(data, "w") as f:
        f.write("\n".join(records(oracle)) + "\n")
    # the header is HIP source: the host side alone, with the library's floating-point contract
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-w",
                    os.path.join(ROOT, "tests", "cpp", "aa_reach_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    # the program's own walk of the chain finds its worst coordinates where the slivers above were put
    for samples in ss.SLIVER_SAMPLES:
        m = re.search(r"chain samples=%d .* at=(\d+) .* at_ulps=(\d+) .* at_last8=(\d+)" % samples, r.stdout)
        assert m and tuple(int(v) for v in m.groups()) == worst_coordinates(samples), (samples, m and m.groups(), worst_coordinates(samples))
