"""What the tests of the arbitrary-ray grid (test_ray_grid_host.py, test_gpu_ray_grid.py) share: the wall scene, the grid's geometry
as grid/ray_grid.hpp's grid_make_desc computes it, the ray sets and the unfit rays planted in them, the incoming records, and the
reference's accept test in numpy float32 (used only to pick phantom candidates on the host; the oracle decides what is expected).
Test plumbing only."""
import numpy as np

import mirt

F32 = np.float32
INF, NAN = F32("inf"), F32("nan")
START_EXTENTS = 2.0                                  # ray_grid.hpp: GRID_START_EXTENTS
# the wall's plane y = 0.3125 z + 0.15625 x + delta: its slopes sit on a corner of the plane index's (alpha, beta) bins (5 / 128 wide)
WALL_NORMAL = np.array([-0.15625, 1.0, -0.3125])
_cache = {}


def _tri_rows(verts):
    """(n, 3, 3) float vertices -> (n, 15) rows: the vertices, the normal and a grey colour."""
    v = np.asarray(verts, np.float64)
    out = np.zeros((len(v), 15), F32)
    out[:, 0:9] = v.reshape(-1, 9).astype(F32)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    out[:, 9:12] = nrm.astype(F32)
    out[:, 12:15] = 0.75
    return out


def wall_frame():
    n = WALL_NORMAL / np.linalg.norm(WALL_NORMAL)
    t1 = np.array([1.0, 0.2, 0.3])
    t1 -= t1.dot(n) * n
    t1 /= np.linalg.norm(t1)
    return n, t1, np.cross(n, t1)


def wall_scene():
    """About 130 triangles: an oblique quad of side 1.2 tessellated 8 x 8, a second parallel wall 0.5 behind it, four soup triangles."""
    if "wall" not in _cache:
        n, t1, t2 = wall_frame()
        o = np.array([-0.2, 0.1, 0.1]) - 0.6 * (t1 + t2)
        c = 1.2 / 8
        tris = []
        for i in range(8):
            for j in range(8):
                q = [o + c * (a * t1 + b * t2) for a, b in ((i, j), (i + 1, j), (i, j + 1), (i + 1, j + 1))]
                tris += [[q[0], q[1], q[2]], [q[3], q[2], q[1]]]
        o2 = o - 0.5 * n
        q = [o2 + 1.2 * (a * t1 + b * t2) for a, b in ((0, 0), (1, 0), (0, 1), (1, 1))]
        tris += [[q[0], q[1], q[2]], [q[3], q[2], q[1]]]
        v = np.concatenate([_tri_rows(np.array(tris)), mirt.scene_soup(13, 4, 0.3)])
        v.setflags(write=False)
        _cache["wall"] = v
    return _cache["wall"]


def scene(name):
    if name == "cornell":
        return mirt.scene_cornell()
    if name == "soup2000":
        return mirt.scene_soup(41, 2000, 0.2)
    if name == "wall":
        return wall_scene()
    raise KeyError(name)


def grid_of(tris):
    """(G, lo[3], w, R, smax) of the scene's grid, in float64 as grid_make_desc computes them."""
    v = np.asarray(tris, F32).reshape(-1, 15)[:, :9].reshape(-1, 3)
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    n, G = len(tris), 4
    while G < 128 and G ** 3 < 2 * n:
        G *= 2
    R = float(max(np.abs(lo).max(), np.abs(hi).max()))
    smax = START_EXTENTS * R
    slack = (smax + R) * (1.0 + 1e-6) * 2.0 ** -20
    w = (max(float((hi - lo).max()), R * 2.0 ** -10) + 2.0 * slack) / (G - 1)
    return G, 0.5 * (lo + hi) - 0.5 * G * w, w, R, smax


def ref_accept(tris, start, direction):
    """raytracer.cpp:216-239 for one ray against every triangle, in numpy float32 (no fused operations): the accept mask."""
    t = np.asarray(tris, F32).reshape(-1, 15)
    v0, e1, e2 = t[:, 0:3], t[:, 3:6] - t[:, 0:3], t[:, 6:9] - t[:, 0:3]

    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)

    def dot(a, b):
        return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

    b = np.asarray(start, F32)[None, :] - v0
    nd = np.broadcast_to(-np.asarray(direction, F32), b.shape)
    x = cross(e1, e2)
    with np.errstate(all="ignore"):
        den = dot(x, nd)
        tt, u, v = dot(x, b) / den, dot(cross(b, e2), nd) / den, dot(cross(e1, b), nd) / den
        return (u + v <= 1) & (u >= 0) & (v >= 0) & (tt >= 0)


def _in_plane_rays(rng, tris, count):
    """The phantom generator on the triangles' own planes: starts in a triangle's plane (or 2^-24 .. 2^-10 off it) up to the scene's
    diameter away, directions within the plane (or 2^-24 .. 2^-6 rad out of it) towards, past and away from the triangle."""
    t = np.asarray(tris, np.float64).reshape(-1, 15)
    out = np.zeros((count, 6), F32)
    for k in range(count):
        r = t[rng.integers(len(t))]
        v0, e1, e2 = r[0:3], r[3:6] - r[0:3], r[6:9] - r[0:3]
        n = np.cross(e1, e2)
        n /= max(np.linalg.norm(n), 1e-30)
        a = e1 / max(np.linalg.norm(e1), 1e-30)
        b = np.cross(n, a)
        phi, dist = rng.uniform(0, 2 * np.pi), rng.uniform(0.05, 1.5)
        psi = [phi + np.pi + rng.uniform(-0.2, 0.2), phi + rng.uniform(-0.3, 0.3), rng.uniform(0, 2 * np.pi)][k % 3]
        eps = 0.0 if k % 5 == 0 else 2.0 ** rng.integers(-24, -5) * rng.choice([-1, 1])
        off = 0.0 if k % 7 < 3 else 2.0 ** rng.integers(-24, -9) * rng.choice([-1, 1])
        c = v0 + (e1 + e2) / 3
        out[k, 0:3] = c + dist * (np.cos(phi) * a + np.sin(phi) * b) + off * n
        out[k, 3:6] = np.cos(psi) * a + np.sin(psi) * b + eps * n
    return out


def phantom_rays(tris, count, seed=5, tries=40000):
    """Up to `count` in-plane rays that the reference's float test accepts on a triangle whose centroid the exact half-line misses by more
    than two cells of the scene's grid -- picked with ref_accept on the host."""
    rng = np.random.default_rng(seed)
    t = np.asarray(tris, np.float64).reshape(-1, 15)
    cen = (t[:, 0:3] + t[:, 3:6] + t[:, 6:9]) / 3
    rad = np.maximum(np.linalg.norm(t[:, 3:6] - t[:, 0:3], axis=1), np.linalg.norm(t[:, 6:9] - t[:, 0:3], axis=1))
    _, _, w, _, _ = grid_of(tris)
    found = []
    cand = _in_plane_rays(rng, tris, tries)
    for ray in cand:
        acc = np.flatnonzero(ref_accept(tris, ray[0:3], ray[3:6]))
        if not len(acc):
            continue
        s, d = ray[0:3].astype(np.float64), ray[3:6].astype(np.float64)
        sc = cen[acc] - s
        tt = np.maximum(0.0, sc.dot(d) / d.dot(d))
        gap = np.linalg.norm(sc - tt[:, None] * d, axis=1)
        if (gap > rad[acc] + 2 * w).any():
            found.append(ray)
            if len(found) == count:
                break
    return np.array(found, F32).reshape(-1, 6)


def lattice_phantom_rays(tris, count, seed=5, tries=4000):
    """phantom_rays for a scene placed away from the origin, where a point of a triangle's plane drawn in float64 is rounded off that
    plane by an ulp of its large coordinates and the float test decides it exactly.  Here start and direction are whole-number
    combinations of the triangle's own float32 edges, S = v0 + i e1 + j e2 and d = k e1 + l e2 in float32: a few edges off the
    triangle, and -- where the vertices share a binade, as those of a small scene at an offset do -- exactly in its plane, so that
    the reference's quotients are rounding noise over rounding noise.  Picked with ref_accept on the host like phantom_rays."""
    rng = np.random.default_rng(seed)
    t32 = np.asarray(tris, F32).reshape(-1, 15)
    t = t32.astype(np.float64)
    cen = (t[:, 0:3] + t[:, 3:6] + t[:, 6:9]) / 3
    rad = np.maximum(np.linalg.norm(t[:, 3:6] - t[:, 0:3], axis=1), np.linalg.norm(t[:, 6:9] - t[:, 0:3], axis=1))
    _, _, w, _, _ = grid_of(tris)
    found = []
    for _ in range(tries):
        r = t32[rng.integers(len(t32))]
        v0, e1, e2 = r[0:3], r[3:6] - r[0:3], r[6:9] - r[0:3]
        i, j = rng.integers(-6, 7, 2)
        k, l = rng.integers(-3, 4, 2)
        if (k == 0 and l == 0) or max(abs(i), abs(j)) < 3:
            continue
        ray = np.concatenate([(v0 + F32(i) * e1) + F32(j) * e2, F32(k) * e1 + F32(l) * e2]).astype(F32)
        acc = np.flatnonzero(ref_accept(tris, ray[0:3], ray[3:6]))
        if not len(acc):
            continue
        s, d = ray[0:3].astype(np.float64), ray[3:6].astype(np.float64)
        sc = cen[acc] - s
        tt = np.maximum(0.0, sc.dot(d) / d.dot(d))
        gap = np.linalg.norm(sc - tt[:, None] * d, axis=1)
        if (gap > rad[acc] + 2 * w).any():
            found.append(ray)
            if len(found) == count:
                break
    return np.array(found, F32).reshape(-1, 6)


def ray_set(name, n=4097, seed=3):
    """(rays (n, 6) float32, planted): uniform segments, axis-parallel rays, rays in cell faces and through cell corners, rays between
    points of one triangle's plane and of two triangles, phantom rays, starts outside the box pointing in, past and away -- and the
    unfit rays planted among them: `planted` is their number."""
    key = ("rays", name, n, seed)
    if key in _cache:
        return _cache[key]
    tris = scene(name)
    rng = np.random.default_rng(seed)
    t = np.asarray(tris, np.float64).reshape(-1, 15)
    v = t[:, :9].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    G, glo, w, R, smax = grid_of(tris)
    rays = np.zeros((n, 6), np.float64)

    def point_on(tri):
        a, b = rng.uniform(0, 1, 2)
        if a + b > 1:
            a, b = 1 - a, 1 - b
        return tri[0:3] + a * (tri[3:6] - tri[0:3]) + b * (tri[6:9] - tri[0:3])

    ph = phantom_rays(tris, max(8, n // 16), seed=seed + 1, tries=3000 if len(tris) > 500 else (2000 if len(tris) < 100 else 12000))
    for i in range(n):
        kind = i % 8
        S, E = rng.uniform(lo, hi), rng.uniform(lo, hi)
        if kind == 1:                                               # axis-parallel, one or two zero components
            d = np.zeros(3)
            d[rng.integers(3)] = rng.choice([-1, 1])
            if i % 16 == 1:
                d[rng.integers(3)] = rng.choice([-1, 1])
            E = S + d
        elif kind == 2:                                             # in a cell face / through a cell corner
            c = rng.integers(3)
            S[c] = E[c] = glo[c] + rng.integers(1, G) * w
            if i % 16 == 2:
                S = glo + rng.integers(1, G, 3) * w
                E = glo + rng.integers(1, G, 3) * w + (rng.integers(0, 2, 3) * w if i % 32 == 2 else 0)
                if np.abs(E - S).max() < 0.5 * w:                   # the same corner twice: along a cell edge instead
                    E = S + np.array([w, 0.0, 0.0])
        elif kind == 3:                                             # two points of one triangle's plane (a wall's: many coplanar triangles)
            a = t[rng.integers(len(t))]
            S, E = point_on(a), point_on(a)
            E = S + (E - S) * rng.uniform(0.5, 3.0)
        elif kind == 4:                                             # points of two triangles
            S, E = point_on(t[rng.integers(len(t))]), point_on(t[rng.integers(len(t))])
        elif kind == 5 and len(ph):                                 # phantoms
            S, E = ph[i % len(ph), 0:3].astype(np.float64), None
            rays[i, 3:6] = ph[i % len(ph), 3:6]
        elif kind == 6:                                             # outside the box: pointing in, past, away
            c = 0.5 * (lo + hi)
            S = c + (S - c) / max(np.abs(S - c).max(), 1e-9) * (hi - lo).max() * rng.uniform(0.6, 0.9)
            E = [E, S + np.cross(S - c, rng.uniform(-1, 1, 3)), S + (S - c)][(i // 8) % 3]
        rays[i, 0:3] = S
        if E is not None:
            rays[i, 3:6] = (E - S) * [1.0, 2.0 ** -20, 2.0 ** 12][(i // 8) % 3 if kind == 0 else 0]
    rays = rays.astype(F32)
    # a zero-length segment would be an unfit ray that nobody planted
    zero = ~rays[:, 3:6].any(axis=1)
    rays[zero, 3] = 1.0
    planted = 0
    if n >= 63:
        odd = [((3, NAN),), ((4, INF),), ((3, 0.0), (4, 0.0), (5, 0.0)), ((3, 1e7),), ((3, 2.0 ** -40), (4, 0.0), (5, 2.0 ** -41)), ((4, 2.0 ** 19),),
               ((0, 1.5 * smax),), ((1, -1.01 * smax), (0, 0.0)), ((2, NAN),), ((0, 1e9),), ((5, -INF),)]
        for k, i in enumerate(range(7, n, max(11, n // 40))):
            for col, val in odd[k % len(odd)]:
                rays[i, col] = val
            planted += 1
    rays.setflags(write=False)
    _cache[key] = (rays, planted)
    return _cache[key]


def as_rays(r6):
    return mirt.make_rays(r6[:, 0:3], r6[:, 3:6])


INCOMING = ("fresh", "earlier", "inf", "negative", "nan", "tie_lower", "tie_higher")


def incoming_records(kind, fresh_result):
    """The in/out records of `kind` for rays whose fresh-record result is `fresh_result`."""
    h = mirt.fresh_hits(len(fresh_result))
    if kind == "earlier":
        h = np.roll(fresh_result, 1).copy()                         # the record the previous ray left
    elif kind == "inf":
        h["distance"] = INF
    elif kind == "negative":
        h["distance"] = -1.0
        h["index"] = 5
    elif kind == "nan":
        h["distance"] = NAN
        h["position"] = 7.0
    elif kind in ("tie_lower", "tie_higher"):
        hit = fresh_result["index"] >= 0
        h["distance"][hit] = fresh_result["distance"][hit]
        h["index"][hit] = fresh_result["index"][hit] + (-1 if kind == "tie_lower" else 1)
        h["position"][hit] = 0.5
    return h
