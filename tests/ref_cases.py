"""The frame configurations both pins share: tests/test_oracle_ref_render.py runs them through the reference's own text
(oracle/_ref, in the build container) against the CPU restatement, and tests/golden/make_golden.py records the reference's
outputs for them as hashes (tests/golden/ref_render.json), which the restatement AND the GPU path must reproduce wherever
the reference is absent.  Scenes are built from generators that live in this repository (Cornell box, mt19937 soups, the
supersampling slivers below), so only the expected outputs come from the reference.

Frames are the sizes the reference itself can render: 500x500, and 150x150 (its -DREALTIME build) for the ray tracer.
"""
import lzma
import os

import numpy as np

L0 = [0.0, -0.5, -0.7, 1.0, 1.0, 1.0, 14.0]                 # AddLight(vec3(0,-0.5f,-0.7f), vec3(1,1,1), 14), raytracer.cpp:116
L1 = [0.5, 0.3, -0.9, 1.0, 0.5, 0.2, 6.0]
L2 = [-0.6, -0.2, 0.1, 0.3, 0.9, 0.4, 9.0]
LS = [0.0, 0.0, 0.2, 1.0, 1.0, 1.0, 14.0]                   # the sliver scenes' light, just in front of their camera

# name: size, scene, camera position, yaw, focal length, lights, aa, soft-shadow samples
RT_CASES = {
    "cornell500_default": dict(size=500, scene=("cornell",), cam=(0, 0, -2), yaw=0.0, focal=250.0, lights=[L0], aa=1, soft=1),
    "cornell500_nolight": dict(size=500, scene=("cornell",), cam=(0, 0, -2), yaw=0.0, focal=250.0, lights=[], aa=1, soft=1),
    "cornell500_yaw_moved_3lights": dict(size=500, scene=("cornell",), cam=(0.2, -0.1, -2.5), yaw=0.3, focal=300.0, lights=[L0, L1, L2], aa=1, soft=1),
    "cornell_soup400_500_yaw": dict(size=500, scene=("cornell+soup", 7, 400, 0.12), cam=(0.1, 0.05, -2.2), yaw=-0.25, focal=250.0, lights=[L0, L1], aa=1, soft=1),
    "cornell150_realtime_default": dict(size=150, scene=("cornell",), cam=(0, 0, -4.3), yaw=0.0, focal=250.0, lights=[L0], aa=1, soft=1),
    "soup2000_150_inside": dict(size=150, scene=("soup", 3, 2000, 0.1), cam=(0.1, -0.2, -0.3), yaw=0.7, focal=75.0, lights=[L0, L2], aa=1, soft=1),
    "cornell150_soft16": dict(size=150, scene=("cornell",), cam=(0, 0, -2), yaw=0.0, focal=75.0, lights=[L0], aa=1, soft=16),
    "cornell150_aa3": dict(size=150, scene=("cornell",), cam=(0, 0, -2), yaw=0.1, focal=75.0, lights=[L0], aa=3, soft=1),
    "cornell_soup150_aa2_soft4_2lights": dict(size=150, scene=("cornell+soup", 5, 60, 0.2), cam=(0, 0.1, -2.1), yaw=-0.2, focal=80.0, lights=[L0, L1], aa=2, soft=4),
    # 4 to 8 samples.  A sparse soup around the camera: most sub-rays miss, x1 stalls, records are carried from sub-ray to sub-ray
    "soup500_150_inside_aa5": dict(size=150, scene=("soup", 13, 500, 0.15), cam=(0.1, -0.2, -0.3), yaw=0.7, focal=75.0, lights=[L0], aa=5, soft=1),
    # the Cornell box's exact ties under a soup, two lights, soft shadows
    "cornell_soup150_aa7_soft2_2lights": dict(size=150, scene=("cornell+soup", 6, 50, 0.2), cam=(0.05, 0.1, -2.1), yaw=0.25, focal=80.0, lights=[L0, L1], aa=7, soft=2),
    # slivers that begin beyond the half pixel around the last column / row of an 8-pixel bin, where the chain of sub-ray
    # coordinates ends beyond it too (sliver_scene below): none at 2, 3 and 5 samples
    "slivers150_aa4": dict(size=150, scene=("slivers", 4, 150, 75.0, (0, 0, 0), 0.0), cam=(0, 0, 0), yaw=0.0, focal=75.0, lights=[LS], aa=4, soft=1),
    "slivers150_aa6": dict(size=150, scene=("slivers", 6, 150, 75.0, (0, 0, 0), 0.0), cam=(0, 0, 0), yaw=0.0, focal=75.0, lights=[LS], aa=6, soft=1),
    "slivers150_aa7": dict(size=150, scene=("slivers", 7, 150, 75.0, (0, 0, 0), 0.0), cam=(0, 0, 0), yaw=0.0, focal=75.0, lights=[LS], aa=7, soft=1),
    "slivers150_aa8": dict(size=150, scene=("slivers", 8, 150, 75.0, (0, 0, 0), 0.0), cam=(0, 0, 0), yaw=0.0, focal=75.0, lights=[LS], aa=8, soft=1),
}

# Cases added after ref_render.json was first recorded.  make_golden.py draws their sampled pixels from a generator of their own, so
# that adding a case leaves every earlier entry of the file as it was recorded.
RT_CASES_ADDED = ("soup500_150_inside_aa5", "cornell_soup150_aa7_soft2_2lights", "slivers150_aa4", "slivers150_aa6", "slivers150_aa7", "slivers150_aa8")

# name: scene, camera position, yaw, focal length, cameraRot[1][1], lights, cull flags (bit0 back face, bit1 frustum), FOCAL_LENGTH
RASTER_CASES = {
    "cornell_default": dict(scene=("cornell",), cam=(0, 0, -3), yaw=0.0, focal=500.0, rot11=1.01, lights=[L0], flags=3, focal_plane=1.9),
    "cornell_yaw_offscreen": dict(scene=("cornell",), cam=(0.9, 0.1, -2.4), yaw=0.5, focal=500.0, rot11=1.01, lights=[L0], flags=3, focal_plane=1.9),
    "cornell_close_offscreen_2lights": dict(scene=("cornell",), cam=(-0.3, 0.2, -1.9), yaw=-0.35, focal=420.0, rot11=1.01, lights=[L0, L1], flags=1, focal_plane=1.3),
    "cornell_soup300_nocull": dict(scene=("cornell+soup", 9, 300, 0.2), cam=(0.1, 0, -3), yaw=0.1, focal=500.0, rot11=1.01, lights=[L0], flags=0, focal_plane=1.9),
    "soup4000_frustum_only": dict(scene=("soup", 4, 4000, 0.08), cam=(0.3, 0.1, -2.6), yaw=0.4, focal=500.0, rot11=1.0, lights=[L0, L2], flags=2, focal_plane=2.5),
}


# ---- supersampling: the sub-ray chain and the slivers it alone can see ------------------------------------------------------

def aa_chain_end(coords, samples):
    """The float32 coordinate of a pixel's last sub-ray: Draw() starts at c - 0.5f and adds 1.0f / (realSamples - 1) once per sub-ray
    before it (raytracer.cpp:566-596), each sum rounded -- a chain, not c - 0.5 + k / (n - 1)."""
    x1 = np.asarray(coords, np.float32) - np.float32(0.5)
    step = np.float32(1.0) / np.float32(samples - 1)
    for _ in range(samples - 1):
        x1 = (x1 + step).astype(np.float32)
    return x1


def aa_overshoot(coords, samples, half=None):
    """How far, in pixels, the last sub-ray of pixel coordinate c lies beyond c + 0.5 (float64; negative where it falls short).
    With `half` (W / 2 or H / 2): measured on the ray itself, whose direction takes float32(x1 - half) (raytracer.cpp:579) -- for
    coordinates below half the frame that subtraction rounds, and can drop the chain's last bits or add to them."""
    c = np.asarray(coords, np.float64)
    if half is None:
        return aa_chain_end(c, samples).astype(np.float64) - (c + 0.5)
    return (aa_chain_end(c, samples) - np.float32(half)).astype(np.float32).astype(np.float64) - (c + 0.5 - half)


def overshooting(limit, samples, every=8):
    """The last coordinates of a bin of `every` pixels below `limit` whose last sub-ray, in a frame `limit` pixels wide or high, lies
    beyond the half pixel."""
    c = np.arange(every - 1, limit, every)
    return [int(v) for v in c[aa_overshoot(c, samples, limit / 2.0) > 0]]


def _finish(v, colour):
    t = np.zeros((len(v), 15), np.float32)
    t[:, 0:9] = np.asarray(v, np.float64).reshape(len(v), 9)
    n = np.cross(t[:, 6:9].astype(np.float64) - t[:, 0:3], t[:, 3:6].astype(np.float64) - t[:, 0:3])
    t[:, 9:12] = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    t[:, 12:15] = colour
    return t


_NUDGE = np.array([(i, j, k) for i in range(-8, 9) for j in range(-8, 9) for k in range(-8, 9)], np.int64)


def project(points, W, H, focal, cam, rot9):
    """Pixel coordinates (u, v) of world points seen from the view, in float64 on the values given."""
    R = np.asarray(rot9, np.float64).reshape(3, 3).T           # columns of the column-major matrix
    h = (np.asarray(points, np.float64).reshape(-1, 3) - np.asarray(cam, np.float64)) @ R      # R^-1 = R^T for a rotation
    return np.stack([W / 2.0 + focal * h[:, 0] / h[:, 2], H / 2.0 + focal * h[:, 1] / h[:, 2]], axis=1)


def _vertex_at(u, v, depth, axis, W, H, focal, cam, rot9):
    """The float32 world point at pixel (u, v) and the given depth; among the float32 points up to eight ulps around it in every
    coordinate, the one whose projected coordinate `axis` is nearest to the wanted one (a projected coordinate moves by some
    (c - W / 2) * 2^-24 pixel per ulp of one world coordinate, which is more than the overshoot of a column near the frame's edge;
    the ulps of two or three coordinates together are finer)."""
    R = np.asarray(rot9, np.float64).reshape(3, 3).T
    p = (np.asarray(cam, np.float64) + R @ (np.array([u - W / 2.0, v - H / 2.0, focal]) * (depth / focal))).astype(np.float32)
    if axis is None:
        return p
    ulp = np.spacing(np.abs(p)).astype(np.float64)
    cand = (p.astype(np.float64) + _NUDGE * ulp).astype(np.float32)
    got = project(cand, W, H, focal, cam, rot9)[:, axis]
    return cand[np.argmin(np.abs(got - (u, v)[axis]))]


def sliver_scene(samples, W, H, focal, cam, rot9, columns=None, rows=None):
    """The scene only a sub-ray beyond the half pixel can tell from its backdrop, for the view given.

    Two backdrop triangles at depth 2 cover the view (x1 advances only after a hit).  For every column x in `columns` (default: every
    last column of an 8-pixel bin whose last sub-ray overshoots at `samples`) a right triangle at depth 1: its vertical left edge at
    u = x + 0.5 + overshoot(x) / 2, rows 4 to H - 4, its third vertex at u = x + 0.95 -- beyond the half pixel around x, within reach
    of the chain's end.  For every row y in `rows` the same turned by a quarter, at depth 1.25, columns 4 to W - 4.  A coordinate that
    does not overshoot (5 samples: none does) gets its edge 2^-16 pixel beyond the half pixel: no sub-ray reaches it.
    Returns (triangles, columns, rows): backdrop 0 and 1, column slivers from 2, row slivers after them."""
    cols = overshooting(W, samples) if columns is None else list(columns)
    rws = overshooting(H, samples) if rows is None else list(rows)
    at = lambda u, v, d, axis=None: _vertex_at(u, v, d, axis, W, H, focal, cam, rot9)
    edge_gap = lambda c, size: float(aa_overshoot(c, samples, size / 2.0)) / 2.0 if aa_overshoot(c, samples, size / 2.0) > 0 else 2.0 ** -16
    v = [[at(-3, -3, 2.0), at(W + 3, -3, 2.0), at(-3, H + 3, 2.0)], [at(W + 3, H + 3, 2.0), at(-3, H + 3, 2.0), at(W + 3, -3, 2.0)]]
    for x in cols:
        edge = x + 0.5 + edge_gap(x, W)
        v.append([at(edge, 4.0, 1.0, 0), at(x + 0.95, 4.0, 1.0), at(edge, H - 4.0, 1.0, 0)])
    for y in rws:
        edge = y + 0.5 + edge_gap(y, H)
        v.append([at(4.0, edge, 1.25, 1), at(4.0, y + 0.95, 1.25), at(W - 4.0, edge, 1.25, 1)])
    t = _finish(v, 0.5)
    t[0:2, 12:15] = (0.75, 0.15, 0.15)
    t[2 + len(cols):, 12:15] = (0.15, 0.75, 0.15)
    return t, cols, rws


def sliver_gaps(tris, cols, rows, W, H, focal, cam, rot9):
    """Per sliver, (lowest, highest) distance in pixels of its edge's two vertices beyond c + 0.5: float64 on the float32 vertices."""
    out = []
    for k, c in enumerate(list(cols) + list(rows)):
        axis = 0 if k < len(cols) else 1
        e = project(tris[2 + k, [0, 1, 2, 6, 7, 8]].reshape(2, 3), W, H, focal, cam, rot9)[:, axis] - (c + 0.5)
        out.append((float(e.min()), float(e.max())))
    return out


def build_scene(oracle, spec):
    if spec[0] == "cornell":
        return oracle.cornell()
    if spec[0] == "slivers":                                        # ("slivers", samples, size, focal, camera position, yaw)
        return sliver_scene(spec[1], spec[2], spec[2], spec[3], spec[4], oracle.rot_from_yaw(spec[5], 1.0))[0]
    soup = oracle.soup(spec[1], spec[2], spec[3])
    return soup if spec[0] == "soup" else np.concatenate([oracle.cornell(), soup])


def lights_array(lights):
    return np.array(lights, np.float32).reshape(-1, 7)


def reference_asset(directory):
    """Writes the reference's own mesh (rasteriser/Source/enemy1.stl, stored as data in tests/golden/enemy1.stl.xz) to
    <directory>/Source/enemy1.stl, the relative path the reference's loader opens, and returns that path."""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enemy1.stl.xz")
    os.makedirs(os.path.join(str(directory), "Source"), exist_ok=True)
    path = os.path.join(str(directory), "Source", "enemy1.stl")
    with lzma.open(src, "rb") as f, open(path, "wb") as g:
        g.write(f.read())
    return path
