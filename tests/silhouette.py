"""Rays aimed at silhouettes and bin borders, and the scenes they are aimed at: generators for test_silhouette_probes_host.py and
test_gpu_silhouette_probes.py.  A plain module like ref_cases.py; numpy float64 throughout, rounded to float32 last.

A probe is a direction float32(P - O) from an origin O to a point P in the plane of its target triangle, within delta of the
triangle's silhouette.  Probes come as twins: the inside twin at +delta towards the triangle's interior, the outside twin at -delta
(consecutive entries: inside at the even index, outside at the odd one), delta relative to the distance to the opposite vertex
(edge and border probes) or to the centroid (vertex probes).  Kinds:
  edge    P on each edge at three interior parameters, moved towards or away from the opposite vertex;
  vertex  each vertex moved towards or away from the centroid -- the extremes of a triangle's (u, v) box;
  border  P on an edge where, as seen from O, the edge crosses a bin border line u = -1 + 2i/64 or v = -1 + 2j/64 of the cube face
          that holds the direction (the face seams |u| = 1, |v| = 1 among them; borders of the 64, 128 and 256 grids alike), 2^-12
          of the edge to either side of the crossing: the bins a triangle enters by a corner only.
bin_of() says which face and bin of a cube around the origin a direction belongs to: the face choice and u = a / m, v = b / m of
the kernels' bin lookup in this module's own words, float32 step by step."""
import numpy as np

DELTAS = (2.0 ** -20, 2.0 ** -14, 2.0 ** -8)
EDGE_PARAMS = (0.25, 0.5, 0.75)
ALONG = 2.0 ** -12
KIND_NAMES = ("edge", "vertex", "border")
EDGE, VERTEX, BORDER = 0, 1, 2

INSIDE = np.array([0.125, -0.0625, 0.1875], np.float32)            # the inside origin of test_gpu_fan_query.py
OUTSIDE = np.array([2.5, 0.75, -1.5], np.float32)
FAR = np.array([300.0, 200.0, -100.0])                             # the "@ far" scenes' offset (placement.py: 300_200_-100): one ulp is about 2^-15 there

PROBE_DTYPE = np.dtype([("dir", np.float32, 3), ("point", np.float64, 3), ("target", np.int32), ("kind", np.int8), ("delta", np.int8),
                        ("inside", np.bool_), ("face", np.int8), ("i", np.int16), ("j", np.int16)])


# ---- the bin of a direction ----------------------------------------------------------------------------------------------------

def bin_of(dirs, bins=64):
    """(face, i, j) of each direction on a cube of bins x bins bins per face.  The ray's negated direction picks the face: the axis
    of its largest magnitude (x before y before z on ties), face 2 * axis, plus one where that component is negative; the two
    other components in cyclic order, divided by the magnitude, are u and v in [-1, 1]; bin i = floor((u + 1) * bins / 2), clamped."""
    nd = -np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    a = np.abs(nd)
    k = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    r = np.arange(len(nd))
    m = a[r, k]
    half = np.float32(0.5 * bins)
    with np.errstate(all="ignore"):
        u, v = nd[r, (k + 1) % 3] / m, nd[r, (k + 2) % 3] / m
        i, j = np.floor((u + np.float32(1)) * half), np.floor((v + np.float32(1)) * half)
    i = np.clip(np.nan_to_num(i, nan=0.0), 0, bins - 1).astype(np.int64)
    j = np.clip(np.nan_to_num(j, nan=0.0), 0, bins - 1).astype(np.int64)
    return 2 * k + (nd[r, k] < 0), i, j


def outside_the_fan_window(dirs):
    """Directions that take no bin of an origin fan: a component that is not finite, or the largest magnitude outside
    [2^-32, 2^19) -- such a ray sweeps the origin's whole table instead (query/rt_query.hpp: fan_dir_of)."""
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    m = np.abs(d).max(axis=1)
    return ~(np.isfinite(d).all(axis=1) & (m >= np.float32(2.0 ** -32)) & (m < np.float32(2.0 ** 19)))


_scenes = {}


def scene_of(oracle, name):
    """The probed scenes by name: (triangles, indices of the target triangles or None for all, crossings per edge, scale)."""
    if name not in _scenes:
        if name == "shell":
            v = scene_shell(), None, 4, 1.0
        elif name == "shell_dense":
            v = scene_shell_dense(), range(150), 4, 1.0
        elif name == "needles":
            v = scene_needles(), None, 4, 1.0
        elif name == "walls":
            v = scene_walls(), None, 24, 1.0
        elif name == "grazing":
            v = scene_grazing(), None, 4, 1.0
        elif name == "tips":
            v = scene_tips(), None, 2, 1.0
        elif name == "soup150":
            v = oracle.soup(41, 2000, 0.2)[:150].copy(), None, 4, 1.0
        elif name == "soup2000":
            v = oracle.soup(41, 2000, 0.2), range(150), 4, 1.0
        elif name == "shell @ far":
            v = finish(shell_vertices(5, np.random.default_rng(3), origin=INSIDE + FAR)), None, 4, 1.0
        elif name == "needles @ far":
            v = finish(shell_vertices(5, np.random.default_rng(4), needles=True, origin=INSIDE + FAR)), None, 4, 1.0
        elif name == "soup2000 @ far":                              # placement.place's arithmetic: one rounding a coordinate
            t = oracle.soup(41, 2000, 0.2)
            t[:, 0:9] = (t[:, 0:9].astype(np.float64).reshape(-1, 3) + FAR).reshape(-1, 9)
            v = t, range(150), 4, 1.0
        elif name == "shell x 3e-4":
            v = scene_shell(3e-4), None, 4, 3e-4
        elif name == "shell x 3e5":
            v = scene_shell(3e5), None, 4, 3e5
        else:
            raise KeyError(name)
        v[0].setflags(write=False)
        _scenes[name] = v
    return _scenes[name]


# ---- probes ------------------------------------------------------------------------------------------------------------------------

_LINES = (np.repeat(np.arange(3), 4), np.tile([1.0, 1.0, -1.0, -1.0], 3), (np.repeat(np.arange(3), 4) + np.tile([1, 2, 1, 2], 3)) % 3)


def border_crossings(A, B, O, max_crossings):
    """Parameters s in (0, 1) at which the edge A + s (B - A), seen from O, crosses a line u = c or v = c, c = -1 + 2i/64, of the cube
    face that holds its direction there.  At most max_crossings of them: the face seams first, the rest spread evenly over the edge
    from the crossing nearest A to the one nearest B."""
    N0, F = -(A - O), -(B - A)                                 # the negated direction along the edge: N0 + s F
    # twelve families of lines: the face's axis k, its sign, and u (the component after k) or v (the one before k) held at c
    k, sg, other = _LINES
    c = (-1.0 + 2.0 * np.arange(65) / 64.0)[None, :]
    with np.errstate(all="ignore"):
        cs = c * sg[:, None]
        s = (cs * N0[k][:, None] - N0[other][:, None]) / (F[other][:, None] - cs * F[k][:, None])
        N = N0 + s[:, :, None] * F
        m = sg[:, None] * np.take_along_axis(N, k[:, None, None], axis=2)[:, :, 0]
        ok = np.isfinite(s) & (s > 4 * ALONG) & (s < 1 - 4 * ALONG) & (m > 0) & (np.abs(N) <= (m * (1 + 1e-9))[:, :, None]).all(axis=2)
    s, seam = s[ok], np.broadcast_to(np.abs(c) == 1.0, ok.shape)[ok]
    if len(s) == 0:
        return s
    s, first = np.unique(np.round(s, 9), return_index=True)   # a seam is a line of both faces
    seam = seam[first]
    seams, rest = s[seam][:max_crossings], s[~seam]
    room = max_crossings - len(seams)
    if room > 0 and len(rest) > room:
        rest = rest[np.unique(np.round(np.linspace(0, len(rest) - 1, room)).astype(int))]
    return np.sort(np.concatenate([seams, rest[:max(room, 0)]]))


def probes(tris, origin, targets=None, max_crossings=4):
    """The probes of triangles `targets` (indices; all when None) of `tris` from `origin`: PROBE_DTYPE, twins adjacent."""
    tris = np.asarray(tris).reshape(-1, 15)
    O = np.asarray(origin, np.float64)
    pts, tgt, kind, dl, ins = [], [], [], [], []

    def twins(P, inw, t, kd):
        for q, d in enumerate(DELTAS):
            for sg in (1, -1):
                pts.append(P + sg * d * inw); tgt.append(t); kind.append(kd); dl.append(q); ins.append(sg > 0)

    for t in (range(len(tris)) if targets is None else targets):
        v = tris[t, :9].reshape(3, 3).astype(np.float64)
        cen = v.mean(0)
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for s in EDGE_PARAMS:
                P = v[a] + s * (v[b] - v[a])
                twins(P, v[c] - P, t, EDGE)
            twins(v[a], cen - v[a], t, VERTEX)
            for s in border_crossings(v[a], v[b], O, max_crossings):
                for side in (ALONG, -ALONG):
                    P = v[a] + (s + side) * (v[b] - v[a])
                    twins(P, v[c] - P, t, BORDER)
    out = np.zeros(len(pts), PROBE_DTYPE)
    out["point"] = np.array(pts).reshape(-1, 3)
    out["dir"] = (out["point"] - O).astype(np.float32)
    out["target"], out["kind"], out["delta"], out["inside"] = tgt, kind, dl, ins
    out["face"], out["i"], out["j"] = bin_of(out["dir"], 64)
    return out


def describe(p, tris, origin, bins=64):
    """Everything needed to find the cause of one probe's failure by reading code."""
    f, i, j = bin_of(p["dir"][None, :], bins)
    return ("%s probe, delta 2^%d, %s twin, target triangle %d, face %d bin (%d, %d) of 64 / face %d bin (%d, %d) of %d\n"
            "    dir %r\n    triangle %r\n    origin %r" % (
                KIND_NAMES[p["kind"]], int(np.log2(DELTAS[p["delta"]])), "inside" if p["inside"] else "outside", p["target"],
                p["face"], p["i"], p["j"], f[0], i[0], j[0], bins, p["dir"].tolist(),
                np.asarray(tris).reshape(-1, 15)[p["target"], :9].tolist(), np.asarray(origin).tolist()))


def oracle_index(oracle, tris, origin, dirs):
    """The oracle's closest-hit index of every ray {origin, dirs[k]} on a fresh record."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 15)
    origin = np.asarray(origin, np.float32)
    out = np.empty(len(dirs), np.int64)
    for k in range(len(dirs)):
        out[k] = oracle.closest_intersection(tris, origin, dirs[k])[3]
    return out


def shares(p, index):
    """Share of probes whose closest hit is their target: all, inside twins, outside twins, and (inside, outside) at the
    smallest delta."""
    hit = index == p["target"]
    ins, small = p["inside"], p["delta"] == 0
    return {"all": float(hit.mean()), "inside": float(hit[ins].mean()), "outside": float(hit[~ins].mean()),
            "inside at 2^-20": float(hit[ins & small].mean()), "outside at 2^-20": float(hit[~ins & small].mean())}


def border_pairs_split(p):
    """Share of border-probe twin pairs whose two directions fall into different bins of the 64 grid."""
    b = np.flatnonzero(p["kind"] == BORDER)
    a, o = b[0::2], b[1::2]
    assert np.all(p["inside"][a]) and not np.any(p["inside"][o]) and np.all(o == a + 1)
    return float(((p["face"][a] != p["face"][o]) | (p["i"][a] != p["i"][o]) | (p["j"][a] != p["j"][o])).mean())


# ---- scenes ------------------------------------------------------------------------------------------------------------------------

def finish(v, scale=1.0):
    """Rows of 15 floats from vertices (count x 3 x 3, float64): scaled, rounded, unit normals, grey."""
    t = np.zeros((len(v), 15), np.float32)
    t[:, 0:9] = (np.asarray(v, np.float64) * scale).reshape(len(v), 9)
    n = np.cross(t[:, 6:9].astype(np.float64) - t[:, 0:3], t[:, 3:6].astype(np.float64) - t[:, 0:3])
    t[:, 9:12] = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    t[:, 12:15] = 0.5
    return t


def on_face(k, sgn, uv):
    """Points (count x 3) at u, v on the face of axis k and sign sgn of the unit cube."""
    uv = np.asarray(uv, np.float64)
    P = np.zeros((len(uv), 3))
    P[:, k], P[:, (k + 1) % 3], P[:, (k + 2) % 3] = sgn, uv[:, 0], uv[:, 1]
    return P


def shell_vertices(n_side, rng, r_lo=0.3, r_hi=3.0, fill=0.8, needles=False, origin=INSIDE):
    """One triangle inside each angular cell of an n_side x n_side grid on each of the six faces of the cube around `origin`, every
    vertex at its own distance in [r_lo, r_hi], so that no triangle hides another from the origin.  needles: aspect 1:1000 and
    sharper, the third vertex a thousandth of the cell off the line through the two others, one distance per triangle."""
    O = np.asarray(origin, np.float64)
    out = []
    for k in range(3):
        for sgn in (1.0, -1.0):
            for i in range(n_side):
                for j in range(n_side):
                    h = fill / n_side
                    uv = np.array([-1 + (2 * i + 1.0) / n_side, -1 + (2 * j + 1.0) / n_side]) + rng.uniform(-h, h, (3, 2))
                    if needles:
                        uv[2] = uv[0] + (uv[1] - uv[0]) * rng.uniform(0.2, 0.8) + rng.uniform(-1, 1, 2) * h * 1e-3
                        r = np.full(3, rng.uniform(r_lo, r_hi))
                    else:
                        r = rng.uniform(r_lo, r_hi, 3)
                    out.append(O + on_face(k, sgn, uv) * r[:, None])
    return np.array(out)


def scene_shell(scale=1.0):
    """150 triangles: the probed set.  `scale` multiplies the scene (and so its origins)."""
    return finish(shell_vertices(5, np.random.default_rng(3)), scale)


def scene_shell_dense():
    """The shell and, behind it, a denser one: 150 + 2166 triangles, past the 2000 at which the cube takes 128 bins a side."""
    return np.concatenate([scene_shell(), finish(shell_vertices(19, np.random.default_rng(5), 3.2, 6.0))])


def scene_needles():
    return finish(shell_vertices(5, np.random.default_rng(4), needles=True))


def scene_walls(origin=INSIDE):
    """Per cube face around `origin`: a needle along the face's diagonal whose box is more than 32 bins of 64 wide and high and
    almost empty, a triangle as wide and high, one more than 64 bins wide that crosses the face's seams on every side, and one with
    a vertex behind the face's plane."""
    O = np.asarray(origin, np.float64)
    out = []
    for k in range(3):
        for sgn in (1.0, -1.0):
            f = 2 * k + (sgn < 0)
            sh = 0.013 * f
            a, b = np.array([-0.7 + sh, -0.6]), np.array([0.6, 0.5 + sh])
            c = a + 0.47 * (b - a) + 3e-4 * np.array([a[1] - b[1], b[0] - a[0]])
            out.append(O + on_face(k, sgn, [a, b, c]) * (0.4 + 0.02 * f))
            out.append(O + on_face(k, sgn, [(-0.62 + sh, -0.55), (0.49 + sh, -0.41 - sh), (-0.3, 0.6 + sh)]) * (0.6 + 0.05 * f))
            out.append(O + on_face(k, sgn, [(-1.7 + sh, -1.3), (1.9, -0.8 + sh), (0.1 - sh, 2.1)]) * (1.4 + 0.05 * f))
            w = on_face(k, sgn, [(-0.4 + sh, -0.7), (0.8, -0.2 - sh), (0.3 + sh, 1.5)])
            w[2, k] = -0.25 * sgn
            out.append(O + w * (2.2 + 0.05 * f))
    return finish(out)


TIP_EPS = (2.0 ** -16, 2.0 ** -18, 2.0 ** -20, 2.0 ** -22)


def scene_tips(origin=INSIDE):
    """The tile-corner slivers of the camera frame on the cube around `origin`: at every sixteenth bin corner of the 64 grid -- a
    corner of the 128 and 256 grids too -- four triangles, one per quadrant.  The first vertex, the tip, lies eps (in u and in v)
    inside one bin, the body in the diagonally opposite one, 0.75 and 0.19 of a bin from the corner: the tip's bin is entered by
    a corner that is 2^-16 .. 2^-22 wide, the last about the rounding of the vertex itself.  384 triangles; eps round-robin."""
    rng = np.random.default_rng(7)
    O = np.asarray(origin, np.float64)
    out, w = [], 2.0 / 64.0 / 8.0
    for k in range(3):
        for sgn in (1.0, -1.0):
            for i in range(8, 64, 16):
                for j in range(8, 64, 16):
                    cu, cv = -1 + 2.0 * i / 64, -1 + 2.0 * j / 64
                    for side, (sx, sy) in enumerate(((1, 1), (-1, -1), (1, -1), (-1, 1))):
                        eps = TIP_EPS[(side + i // 16 + j // 16 + 2 * k) % 4]
                        uv = [(cu - sx * eps, cv - sy * eps), (cu + sx * 6.0 * w, cv + sy * 1.5 * w), (cu + sx * 1.5 * w, cv + sy * 6.0 * w)]
                        out.append(O + on_face(k, sgn, uv) * rng.uniform(0.3, 3.0, 3)[:, None])
    return finish(out)


def tips_in_their_own_bin(p, tris, origin):
    """Share of the inside twins at the smallest delta of the tips' vertex probes (scene_tips: vertex 0) whose direction falls into
    another bin of the 64 grid than the direction to the triangle's centroid."""
    v = np.asarray(tris, np.float64).reshape(-1, 15)[:, :9].reshape(-1, 3, 3)
    sel = np.flatnonzero((p["kind"] == VERTEX) & p["inside"] & (p["delta"] == 0))
    sel = sel[np.linalg.norm(p["point"][sel] - v[p["target"][sel], 0], axis=1) < 1e-5 * np.linalg.norm(v[p["target"][sel], 1] - v[p["target"][sel], 0], axis=1)]
    f, i, j = bin_of((v[p["target"][sel]].mean(axis=1) - np.asarray(origin, np.float64)).astype(np.float32), 64)
    return float(((f != p["face"][sel]) | (i != p["i"][sel]) | (j != p["j"][sel])).mean()), len(sel)


def scene_grazing(origin=INSIDE):
    """64 triangles whose plane passes 1e-3 .. 1e-6 from `origin`, 0.5 .. 2 away from it inside that plane: seen almost edge-on."""
    rng = np.random.default_rng(6)
    O = np.asarray(origin, np.float64)
    out = []
    for q in range(64):
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        e1 = np.cross(n, rng.normal(size=3)); e1 /= np.linalg.norm(e1)
        e2 = np.cross(n, e1)
        h = (1e-3, 1e-4, 1e-5, 1e-6)[q % 4] * (1 if (q // 4) % 2 else -1)
        centre = rng.uniform(0.5, 2.0) * e1
        ab = rng.uniform(-0.3, 0.3, (3, 2))
        out.append(O + h * n + centre + ab[:, :1] * e1 + ab[:, 1:] * e2)
    return finish(out)


def offset_of(name):
    """Where the scene `name` of scene_of lies: FAR for the "@ far" scenes, the world origin for the others."""
    return FAR if name.endswith("@ far") else np.zeros(3)


def origins_of(tris, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """Inside the scene, outside its box, and exactly on a vertex of triangle 0; `offset`: where the scene lies (offset_of)."""
    off = np.asarray(offset, np.float64)
    return {"inside": (INSIDE.astype(np.float64) * scale + off).astype(np.float32), "outside": (OUTSIDE.astype(np.float64) * scale + off).astype(np.float32),
            "vertex": np.array(tris[0, 0:3], np.float32)}


def with_receivers(tris, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """The scene plus six small far triangles whose normals are the six axis directions: what a DirectLight record names as its
    surface, so that some normal faces the light wherever the record lies.  Returns (scene, index of the first receiver).
    `offset`: where the scene lies (offset_of) -- the receivers surround it there."""
    v = []
    for k in range(3):
        for sgn in (1.0, -1.0):
            n = np.zeros(3); n[k] = sgn
            a, b = np.zeros(3), np.zeros(3)
            a[(k + 1) % 3], b[(k + 2) % 3] = 1e-3, 1e-3
            base = 40.0 * n
            v.append([base, base + (b if sgn > 0 else a), base + (a if sgn > 0 else b)])
    rec = finish(np.asarray(v, np.float64) * scale + np.asarray(offset, np.float64))
    want = np.repeat(np.eye(3), 2, axis=0) * np.tile([1.0, -1.0], 3)[:, None]
    assert np.allclose(rec[:, 9:12], want), rec[:, 9:12]
    return np.concatenate([np.asarray(tris, np.float32).reshape(-1, 15), rec]), len(tris)


SHADOW_STEPS = (1.25, 2.0, 4.0)


def shadow_records(p, light, first_receiver, hit_dtype):
    """One DirectLight record per probe: position L + k (P - L) behind the probe's point P as seen from the light L, k dealt
    round-robin over the twin pairs; index the receiver whose normal faces the light most directly."""
    L = np.asarray(light, np.float64)
    k = np.array(SHADOW_STEPS)[(np.arange(len(p)) // 2) % len(SHADOW_STEPS)]
    rec = np.zeros(len(p), hit_dtype)
    pos = L + k[:, None] * (p["point"] - L)
    rec["position"] = pos
    to_light = L - pos
    ax = np.abs(to_light).argmax(axis=1)
    rec["index"] = first_receiver + 2 * ax + (to_light[np.arange(len(p)), ax] < 0)
    rec["distance"] = 1.0
    return rec


def resolved(p, rec, light, name):
    """The probes and records without those whose float32 position IS the light: a delta below what a position resolves.  At the
    world origin there is none; at FAR (an ulp of a position is 2^-15 of the scene) there are the two 2^-20 twins of the light's own
    vertex, seen from that vertex.  Such a record is DirectLight's 0 / 0 -- no shadow ray, by design a sweep -- and no probe."""
    at_light = (rec["position"] == np.asarray(light, np.float32)).all(axis=1)
    if name.endswith("@ far"):
        assert at_light.sum() <= 2 and (p["kind"][at_light] == VERTEX).all() and (p["delta"][at_light] == 0).all(), (name, int(at_light.sum()))
    else:
        assert not at_light.any(), (name, int(at_light.sum()))
    return p[~at_light], rec[~at_light]


# ---- camera tile-corner slivers ------------------------------------------------------------------------------------------------------

W, H = 203, 117
FOCAL = H / 2.0
CAM = np.array([0.0, 0.0, -2.0])
SLIVER_DELTAS = (2.0 ** -6, 2.0 ** -10, 2.0 ** -14, 2.0 ** -17)


def scene_slivers(rot9):
    """Four triangles for every third 8 x 8-pixel tile horizontally and every second vertically, one per corner pixel of the tile:
    the tip lies delta pixels past the pixel's centre, the body in the diagonal neighbour tile.  Placed along the rays of the view
    with rotation rot9 (column-major 3 x 3, as the reference's cameraRot).  Returns (triangles, corner pixels (x, y), delta index)."""
    rng = np.random.default_rng(5)
    R = np.asarray(rot9, np.float64).reshape(3, 3).T          # columns of the column-major matrix

    def world(px, py, depth):
        return CAM + R @ (np.array([px - W / 2.0, py - H / 2.0, FOCAL]) * (depth / FOCAL))

    v, tgt, dl = [], [], []
    for tj in range(1, H // 8 - 1, 2):
        for ti in range(1, W // 8 - 1, 3):
            for side, (sx, sy) in enumerate(((1, 1), (-1, -1), (1, -1), (-1, 1))):
                q = (side + ti + tj) % 4
                delta = SLIVER_DELTAS[q]
                x, y = 8 * ti + (7 if sx > 0 else 0), 8 * tj + (7 if sy > 0 else 0)
                depth = rng.uniform(1.0, 5.0)
                v.append([world(x - sx * delta, y - sy * delta, depth), world(x + sx * 6.0, y + sy * 1.5, depth),
                          world(x + sx * 1.5, y + sy * 6.0, depth)])
                tgt.append((x, y)); dl.append(q)
    return finish(v), np.array(tgt), np.array(dl)


def sliver_ownership(index_plane, tgt, dl):
    """Share of slivers that own their corner pixel in an index plane: overall and per delta."""
    got = index_plane[tgt[:, 1], tgt[:, 0]] == np.arange(len(tgt))
    return float(got.mean()), [float(got[dl == q].mean()) for q in range(len(SLIVER_DELTAS))]
