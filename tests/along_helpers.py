"""What the tests of the ray queries along one direction (test_along_host.py, test_gpu_along.py) share: the directions, starts
outside the structure's reach, the grid of a direction in this module's own words, and starts aimed at silhouettes and cell
borders -- tests/silhouette.py's probes (its deltas, edge parameters and twins) turned from directions into starts.  Test
plumbing only."""
import numpy as np

from query_helpers import NAN, seam_directions
from silhouette import ALONG, DELTAS, EDGE_PARAMS

INF = np.float32("inf")
OBLIQUE = np.array([0.37, -0.52, 0.81], np.float32)         # the direction of the rows-offered bound (GPU) and of its CPU forecast
SHELLS = 8                                                   # along/along.hpp: ALONG_SHELLS
START_EXTENTS = 8.0                                          # ... ALONG_START_EXTENTS
PAD_MAX = 0.25                                               # ... ALONG_PAD_MAX


def directions():
    """The 26 axis, face-diagonal and corner directions (seam_directions()'s base set), the oblique one, and one each of
    magnitude 2^-30 and 2^18."""
    base = seam_directions()[::7]
    assert len(base) == 26 and all(set(np.abs(d).tolist()) <= {0.0, 1.0} for d in base)
    tiny = (OBLIQUE / np.abs(OBLIQUE).max() * np.float32(2.0 ** -30)).astype(np.float32)
    huge = (np.array([-0.3, 1.0, 0.45], np.float32) * np.float32(2.0 ** 18)).astype(np.float32)
    return [d for d in base] + [OBLIQUE, tiny, huge]


def plant_odd_starts(starts, extent):
    """query_helpers.odd_rays' kinds for a call whose direction is shared (every 41st start from the 6th on): a start at 1e9, a
    NaN component, an infinite one, and one just beyond the structure's reach (16 x the scene's extent).  Returns (starts, planted)."""
    starts = np.array(starts, np.float32)
    planted = np.zeros(len(starts), bool)
    for k, i in enumerate(range(5, len(starts), 41)):
        starts[i][k % 3] = (np.float32(1e9), NAN, INF if k % 2 else -INF, np.float32(2 * START_EXTENTS * extent))[k % 4]
        planted[i] = True
    return starts, planted


def bins_for(n):
    B = 8
    while B < 256 and B * B * 2 < n:
        B *= 2
    return B


def grid_of(direction, lo, hi, n):
    """The grid across `direction` over the box [lo, hi] for a scene of n triangles (along/along.hpp: along_make_desc): dominant
    axis k of the direction and the two across, c = dir[k1 | k2] / dir[k], and the cell of (p, q) = (S[k1] - c1 S[k], S[k2] - c2 S[k])
    as ((p - p0) * ip, (q - q0) * iq): B - 2 cells over the box's projection and one of margin on every side.  None where the
    header makes no descriptor for a finite box and a direction inside the window: `pad` beyond PAD_MAX."""
    d = np.asarray(direction, np.float32)
    k = int(np.argmax(np.abs(d) >= np.abs(d).max()))
    k1, k2 = (k + 1) % 3, (k + 2) % 3
    c1, c2 = np.float32(d[k1] / d[k]), np.float32(d[k2] / d[k])
    B = bins_for(n)
    corners = np.array([[(hi if s >> c & 1 else lo)[c] for c in range(3)] for s in range(8)], np.float64)
    p, q = corners[:, k1] - float(c1) * corners[:, k], corners[:, k2] - float(c2) * corners[:, k]
    R = max(np.abs(np.asarray(lo, np.float64)).max(), np.abs(np.asarray(hi, np.float64)).max())
    wp, wq = max(p.max() - p.min(), R * 2.0 ** -10) / (B - 2), max(q.max() - q.min(), R * 2.0 ** -10) / (B - 2)
    g = dict(k=k, k1=k1, k2=k2, c1=c1, c2=c2, B=B, p0=np.float32(p.min() - wp), q0=np.float32(q.min() - wq),
             ip=np.float32(1.0 / wp), iq=np.float32(1.0 / wq))
    # how far a computed cell coordinate may lie from the exact one, in cells: beyond PAD_MAX the cells are finer than a float
    # resolves at the scene's distance from the origin, and no grid is made (None) -- "no descriptor"
    smax = float(np.float32(START_EXTENTS * max(R, 1e-30)))
    g["pad"] = max(2.0 ** -20 * (float(g["ip"]) * (smax + abs(float(g["p0"]))) + B), 2.0 ** -20 * (float(g["iq"]) * (smax + abs(float(g["q0"]))) + B))
    return g if g["pad"] <= PAD_MAX else None


def cell_of(grid, starts):
    """The cell coordinates (i, j) of every start, float32 step by step as the kernels compute them; -1 outside the grid."""
    S = np.ascontiguousarray(starts, np.float32).reshape(-1, 3)
    g = grid
    with np.errstate(all="ignore"):
        p = S[:, g["k1"]] - g["c1"] * S[:, g["k"]]
        q = S[:, g["k2"]] - g["c2"] * S[:, g["k"]]
        gi, gj = (p - g["p0"]) * g["ip"], (q - g["q0"]) * g["iq"]
    ok = (gi >= 0) & (gi < g["B"]) & (gj >= 0) & (gj < g["B"])
    return np.where(ok, np.nan_to_num(gi).astype(np.int64), -1), np.where(ok, np.nan_to_num(gj).astype(np.int64), -1)


def silhouette_starts(tris, direction, targets, grid, depths=(0.75, 2.5, 0.001)):
    """Starts whose ray along `direction` passes within DELTAS (2^-20, 2^-14, 2^-8, relative) of the projected edges and vertices
    of the target triangles, and of the points where an edge crosses a border line of the grid; twins to either side, as in
    silhouette.probes.  Each point P of the triangle's plane becomes the start P - depth * dir / |dir|, the depths dealt in turn."""
    tris = np.asarray(tris).reshape(-1, 15)
    d = np.asarray(direction, np.float64)
    dh = d / np.linalg.norm(d)
    pts = []

    def twins(P, inw):
        for delta in DELTAS:
            for sg in (1, -1):
                pts.append(P + sg * delta * inw)

    def crossings(A, Bv):
        """Parameters s in (0, 1) where the projection of A + s (Bv - A) crosses a border line of the grid (a few per edge)."""
        out = []
        for ax, c, o, inv in ((grid["k1"], grid["c1"], grid["p0"], grid["ip"]), (grid["k2"], grid["c2"], grid["q0"], grid["iq"])):
            fa = (A[ax] - float(c) * A[grid["k"]] - float(o)) * float(inv)
            fb = (Bv[ax] - float(c) * Bv[grid["k"]] - float(o)) * float(inv)
            for line in range(int(np.ceil(min(fa, fb))), int(np.floor(max(fa, fb))) + 1)[:3]:
                if fa != fb and 4 * ALONG < (line - fa) / (fb - fa) < 1 - 4 * ALONG:
                    out.append((line - fa) / (fb - fa))
        return out

    for t in targets:
        v = tris[t, :9].reshape(3, 3).astype(np.float64)
        cen = v.mean(0)
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for s in EDGE_PARAMS:
                P = v[a] + s * (v[b] - v[a])
                twins(P, v[c] - P)
            twins(v[a], cen - v[a])
            for s in crossings(v[a], v[b]):
                for side in (ALONG, -ALONG, 0.0):
                    P = v[a] + (s + side) * (v[b] - v[a])
                    twins(P, v[c] - P)
    pts = np.array(pts).reshape(-1, 3)
    depth = np.array(depths)[np.arange(len(pts)) % len(depths)]
    return np.ascontiguousarray((pts - depth[:, None] * dh).astype(np.float32))
