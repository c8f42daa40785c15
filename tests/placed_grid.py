"""The placed inputs of the arbitrary-ray grid and of the ordered hits, and the oracle's answers on them: what
test_gpu_placement_grid.py compares the library with and test_placement_host.py looks at without a GPU.  A sibling of
test_gpu_placement.Placed over placement.GRID_PLACEMENTS; everything is made from the placed float32 inputs by the CPU oracle alone,
once per placement, and left unchanged.  Test plumbing only.

FIGURES holds what the oracle shows per placement (measured on the CPU, never on a GPU); every floor of floors_missed is half of it."""
import numpy as np

import mirt
import ordered_helpers as O
import placement as pl
import query_helpers as rq
import ray_grid_helpers as H
from test_gpu_alongs import deal
from test_gpu_placement import QUERY_SCENE, SHARE, Placed

TIE_SCENE = pl.TIE_SCENE
SCENES = (QUERY_SCENE, TIE_SCENE)
NBASE, NPLANE, NPHANTOM = 1025, 240, 96          # ray_set's rays, in-plane rays and (at most) phantom rays: under 1500 with room to spare
NSMALL = 65                                      # the rays that have a per-triangle table: `after` records and the in-place peel
NALONG, NALONG_TABLE = 257, 65
KINDS = ("fresh", "earlier", "tie_lower", "tie_higher", "nan")
HITS = (1, 3, 8)
UNFIT_EVERY = 31                                 # an unfit ray planted at 5, 36, 67, ...: two among the first 65


def unfit(r6, tris):
    """grid_ray_fit's words in numpy: a ray takes the grid when its direction is finite with its largest |component| in
    [2^-32, 2^19) and no |component| of its start exceeds smax = 2 R, R the largest |coordinate| of the scene.  The others sweep."""
    r6 = np.asarray(r6, np.float32)
    with np.errstate(invalid="ignore"):
        m = np.abs(r6[:, 3:6]).max(axis=1)
        fit = np.isfinite(r6).all(axis=1) & (m >= np.float32(2.0 ** -32)) & (m < np.float32(2.0 ** 19))
        fit &= np.abs(r6[:, 0:3]).max(axis=1).astype(np.float64) <= H.START_EXTENTS * pl.extent_of(tris)
    return ~fit


def phantom_hits(tris, r6, hits):
    """Of the oracle's records hits[n, slots] of the rays r6, those that name a triangle the exact half-line misses by more than the
    triangle's size and two cells of the scene's grid (test_gpu_ray_grid.py: test_the_ray_sets_hold_phantoms): accepted by rounding
    alone, and offered by the plane index or the every-ray list alone."""
    t = np.asarray(tris, np.float64).reshape(-1, 15)
    ix = np.clip(hits["index"], 0, len(t) - 1)
    cen = (t[:, 0:3] + t[:, 3:6] + t[:, 6:9])[ix] / 3
    rad = np.maximum(np.linalg.norm(t[:, 3:6] - t[:, 0:3], axis=1), np.linalg.norm(t[:, 6:9] - t[:, 0:3], axis=1))[ix]
    s, d = r6[:, None, 0:3].astype(np.float64), r6[:, None, 3:6].astype(np.float64)
    with np.errstate(all="ignore"):
        tt = np.maximum(0.0, ((cen - s) * d).sum(axis=2) / (d * d).sum(axis=2))
        gap = np.linalg.norm(cen - s - tt[:, :, None] * d, axis=2)
        return (hits["index"] >= 0) & (gap > rad + 2 * H.grid_of(tris)[2])


def tie_counts(hits, counts):
    """(rays with two equal distances next to each other in their first 8 hits, rays with such a pair as the K-th and (K + 1)-th hit
    for K = 1, 2 or 4: the cut falls between the two)."""
    d, ok = hits["distance"], np.arange(hits.shape[1])[None, :] < counts[:, None]
    pair = (d[:, 1:] == d[:, :-1]) & ok[:, 1:]
    return int(pair.any(axis=1).sum()), int(pair[:, [0, 1, 3]].any(axis=1).sum())


class PlacedGrid(Placed):
    def __init__(self, oracle, pname, rows=None):
        self.o, self.pname = oracle, pname
        self.T, self.s = pl.GRID_PLACEMENTS[pname]
        self.rows = rows or {}
        self.memo, self.shares, self.figures = {}, {}, {}

    # -- arbitrary rays: the ray grid, and the ordered hits by sweep and through it --
    def grid_rays(self, scene):
        """dict(r6, rays, unfit): ray_grid_helpers.ray_set of the unit soup with its starts placed and its directions scaled, in-plane
        and phantom rays made on the PLACED triangles (a placed in-plane ray is in no plane), all in a fixed shuffle, then the unfit
        rays planted: starts beyond 2 R of the placed box, zero, non-finite and out-of-window directions."""
        def make():
            tris = self.tris(scene)
            u = H.ray_set("soup2000", NBASE, seed=3)[0]
            base = np.concatenate([self.place(u[:, 0:3]), pl.place_dirs(u[:, 3:6], self.s)], axis=1)
            rng = np.random.default_rng(19)
            plane = H._in_plane_rays(rng, tris, NPLANE)
            # (away from the origin phantom_rays finds next to nothing -- its float64 plane points are rounded off the plane --, the
            # lattice generator some 40 to 80 in every placement)
            ph = np.concatenate([H.phantom_rays(tris, NPHANTOM, seed=6, tries=1500), H.lattice_phantom_rays(tris, NPHANTOM, seed=6, tries=3000)])
            r6 = np.concatenate([base, plane, ph]).astype(np.float32)
            r6 = r6[np.random.default_rng(29).permutation(len(r6))]
            R = np.float32(pl.extent_of(tris))
            two = np.float32(2.0)
            odd = [((0, np.nextafter(two * R, np.float32("inf"))),), ((1, -np.float32(2.5) * R),), ((3, 0.0), (4, 0.0), (5, 0.0)), ((4, rq.NAN),), ((5, rq.INF),),
                   ((3, 2.0 ** 19), (4, 1.0), (5, -3.0)), ((3, 2.0 ** -33), (4, 0.0), (5, -2.0 ** -34)), ((2, rq.NAN),), ((0, -rq.INF),)]
            for k, i in enumerate(range(5, len(r6), UNFIT_EVERY)):
                for col, val in odd[k % len(odd)]:
                    r6[i, col] = val
            assert len(r6) <= 1500
            return dict(r6=r6, rays=H.as_rays(r6), unfit=unfit(r6, tris), nphantom_rays=len(ph))
        return self.once(("grid rays", scene), make)

    def grid_records(self, scene, kind):
        """(incoming records of `kind`, the oracle's records after the call) for grid_rays(scene)."""
        def make():
            rays = self.grid_rays(scene)["rays"]
            fresh = None if kind == "fresh" else self.grid_records(scene, "fresh")[1]
            incoming = mirt.fresh_hits(len(rays)) if kind == "fresh" else H.incoming_records(kind, fresh)
            with np.errstate(all="ignore"):
                out = rq.oracle_intersect(self.o, self.tris(scene), rays, incoming)
            if kind == "fresh":
                self.share("grid rays on " + scene, out)
            return incoming, out
        return self.once(("grid records", scene, kind), make)

    def grid_limits(self, scene):
        """(limits, the occlusion bytes with them, the bytes with NULL): at, one float above and one float below the closest distance."""
        def make():
            hits = self.grid_records(scene, "fresh")[1]
            d = np.where(hits["index"] >= 0, hits["distance"], np.float32(self.s)).astype(np.float32)
            kind = np.arange(len(hits)) % 3
            limits = np.select([kind == 0, kind == 1], [d, np.nextafter(d, rq.INF)], np.nextafter(d, np.float32(0))).astype(np.float32)
            want = rq.expected(hits, limits)
            hit = hits["index"] >= 0
            assert want[hit & (kind == 1)].all() and not want[kind != 1].any() and (hit & (kind == 1)).sum() > 20
            return limits, want, rq.expected(hits, None)
        return self.once(("grid limits", scene), make)

    def grid_ordered(self, scene):
        """(hits[n, 8], counts[n]): the oracle's enumeration of every grid ray's first eight hits (ordered_helpers.peel)."""
        def make():
            want = O.peel(self.o, self.tris(scene), self.grid_rays(scene)["rays"], 8)
            c = want[1]
            self.figures["phantom acceptances on " + scene] = int(phantom_hits(self.tris(scene), self.grid_rays(scene)["r6"], want[0]).sum())
            self.shares["grid rays on %s, ordered: a hit" % scene] = float((c >= 1).mean())
            self.figures["grid rays on %s: share with two hits" % scene] = float((c >= 2).mean())
            self.figures["grid rays on %s: share full at max_hits 4" % scene] = float((c >= 4).mean())
            if scene == TIE_SCENE:
                self.figures["grid rays on %s: rays with a tie" % scene], self.figures["grid rays on %s: rays with a tie at a cut" % scene] = tie_counts(*want)
            return want
        return self.once(("grid ordered", scene), make)

    def grid_table(self, scene):
        """ordered_helpers.table for the first NSMALL grid rays: what an arbitrary `after` record is answered from."""
        def make():
            rec = O.table(self.o, self.tris(scene), self.grid_rays(scene)["rays"][:NSMALL])
            O_same(O.from_table(rec, None, 8), (self.grid_ordered(scene)[0][:NSMALL], self.grid_ordered(scene)[1][:NSMALL]), "table vs peel")
            return (rec,)
        return self.once(("grid table", scene), make)[0]

    # -- parallel rays: the ordered hits through the along grids --
    def ordered_along(self, scene, dname):
        """One direction of placement.ALONG_DIRS: Placed.starts' starts, the oracle's enumeration to eight hits and the table of
        the first NALONG_TABLE rays."""
        def make():
            starts, planted = self.starts(scene, NALONG)
            d = pl.place_dirs(pl.ALONG_DIRS[dname], self.s)
            return self._along_answers("along %s on %s" % (dname, scene), scene, starts, planted, mirt.make_rays(starts, d), dict(d=d))
        return self.once(("ordered along", scene, dname), make)

    def ordered_alongs(self, scene=QUERY_SCENE):
        """The five directions of placement.ALONG_DIRS dealt as test_gpu_alongs.deal deals them."""
        def make():
            starts, planted = self.starts(scene, NALONG)
            dirs = np.ascontiguousarray([pl.place_dirs(d, self.s) for d in pl.ALONG_DIRS.values()], np.float32)
            of = deal(NALONG, len(dirs))
            return self._along_answers("along five directions on %s" % scene, scene, starts, planted, mirt.make_rays(starts, dirs[of]), dict(dirs=dirs, of=of))
        return self.once(("ordered alongs", scene), make)

    def _along_answers(self, what, scene, starts, planted, rays, out):
        tris = self.tris(scene)
        want = O.peel(self.o, tris, rays, 8)
        rec = O.table(self.o, tris, rays[:NALONG_TABLE])
        O_same(O.from_table(rec, None, 8), (want[0][:NALONG_TABLE], want[1][:NALONG_TABLE]), what + ": table vs peel")
        c = want[1]
        self.shares[what + ", ordered: a hit"] = float((c >= 1).mean())
        self.figures[what + ": share with two hits"] = float((c >= 2).mean())
        self.figures[what + ": share full at max_hits 4"] = float((c >= 4).mean())
        if scene == TIE_SCENE:
            self.figures[what + ": rays with a tie"], self.figures[what + ": rays with a tie at a cut"] = tie_counts(*want)
        out.update(starts=starts, planted=planted, want=want, rec=rec)
        return out

    def after_cases(self, rec):
        """[(after records, {max_hits: (hits, counts)})] for the three rotations of ordered_helpers.after_records: every ray meets
        three of the eleven kinds."""
        slot0 = O.from_table(rec, None, 1)[0][:, 0]
        return [(after, {m: O.from_table(rec, after, m) for m in HITS}) for after in (O.after_records(slot0, shift)[0] for shift in (0, 4, 8))]

    def everything(self):
        """Every input and answer of test_gpu_placement_grid.py (what test_placement_host.py looks at without a GPU):
        (hit shares, figures)."""
        for scene in SCENES:
            for kind in KINDS:
                self.grid_records(scene, kind)
            self.grid_limits(scene); self.grid_ordered(scene); self.grid_table(scene)
        if self.pname in pl.PLACEMENTS:
            for scene in SCENES:
                for dname in pl.SINGLE_DIRS:
                    self.ordered_along(scene, dname)
                self.ordered_alongs(scene)
        return self.shares, self.figures


def O_same(got, want, what):
    assert np.array_equal(got[1], want[1]) and np.ascontiguousarray(got[0]).tobytes() == np.ascontiguousarray(want[0]).tobytes(), what


def prefix(want, n, max_hits):
    hits, counts = want
    return np.ascontiguousarray(hits[:n, :max_hits]), np.minimum(counts[:n], max_hits).astype(np.int32)


# what the oracle shows, per placement (the floors are half of these; phantom acceptances count where the ray grid bins)
FIGURES = {
    'unit': {
        'phantom acceptances on soup2000': 167,
        'grid rays on soup2000: share with two hits': 0.544,
        'grid rays on soup2000: share full at max_hits 4': 0.309,
        'phantom acceptances on soup2000+dup': 192,
        'grid rays on soup2000+dup: share with two hits': 0.542,
        'grid rays on soup2000+dup: share full at max_hits 4': 0.318,
        'grid rays on soup2000+dup: rays with a tie': 101,
        'grid rays on soup2000+dup: rays with a tie at a cut': 68,
        'along oblique on soup2000: share with two hits': 0.249,
        'along oblique on soup2000: share full at max_hits 4': 0.097,
        'along -y on soup2000: share with two hits': 0.226,
        'along -y on soup2000: share full at max_hits 4': 0.082,
        'along five directions on soup2000: share with two hits': 0.237,
        'along five directions on soup2000: share full at max_hits 4': 0.101,
        'along oblique on soup2000+dup: share with two hits': 0.253,
        'along oblique on soup2000+dup: share full at max_hits 4': 0.109,
        'along oblique on soup2000+dup: rays with a tie': 11,
        'along oblique on soup2000+dup: rays with a tie at a cut': 6,
        'along -y on soup2000+dup: share with two hits': 0.226,
        'along -y on soup2000+dup: share full at max_hits 4': 0.089,
        'along -y on soup2000+dup: rays with a tie': 9,
        'along -y on soup2000+dup: rays with a tie at a cut': 4,
        'along five directions on soup2000+dup: share with two hits': 0.237,
        'along five directions on soup2000+dup: share full at max_hits 4': 0.113,
        'along five directions on soup2000+dup: rays with a tie': 11,
        'along five directions on soup2000+dup: rays with a tie at a cut': 7,
    },
    '3_0_0': {
        'phantom acceptances on soup2000': 41,
        'grid rays on soup2000: share with two hits': 0.549,
        'grid rays on soup2000: share full at max_hits 4': 0.305,
        'phantom acceptances on soup2000+dup': 59,
        'grid rays on soup2000+dup: share with two hits': 0.541,
        'grid rays on soup2000+dup: share full at max_hits 4': 0.305,
        'grid rays on soup2000+dup: rays with a tie': 97,
        'grid rays on soup2000+dup: rays with a tie at a cut': 66,
        'along oblique on soup2000: share with two hits': 0.249,
        'along oblique on soup2000: share full at max_hits 4': 0.097,
        'along -y on soup2000: share with two hits': 0.226,
        'along -y on soup2000: share full at max_hits 4': 0.082,
        'along five directions on soup2000: share with two hits': 0.237,
        'along five directions on soup2000: share full at max_hits 4': 0.101,
        'along oblique on soup2000+dup: share with two hits': 0.253,
        'along oblique on soup2000+dup: share full at max_hits 4': 0.109,
        'along oblique on soup2000+dup: rays with a tie': 11,
        'along oblique on soup2000+dup: rays with a tie at a cut': 6,
        'along -y on soup2000+dup: share with two hits': 0.226,
        'along -y on soup2000+dup: share full at max_hits 4': 0.089,
        'along -y on soup2000+dup: rays with a tie': 9,
        'along -y on soup2000+dup: rays with a tie at a cut': 4,
        'along five directions on soup2000+dup: share with two hits': 0.237,
        'along five directions on soup2000+dup: share full at max_hits 4': 0.113,
        'along five directions on soup2000+dup: rays with a tie': 11,
        'along five directions on soup2000+dup: rays with a tie at a cut': 7,
    },
    '10_-7_5': {
        'phantom acceptances on soup2000': 57,
        'grid rays on soup2000: share with two hits': 0.539,
        'grid rays on soup2000: share full at max_hits 4': 0.304,
        'phantom acceptances on soup2000+dup': 65,
        'grid rays on soup2000+dup: share with two hits': 0.535,
        'grid rays on soup2000+dup: share full at max_hits 4': 0.314,
        'grid rays on soup2000+dup: rays with a tie': 99,
        'grid rays on soup2000+dup: rays with a tie at a cut': 64,
        'along oblique on soup2000: share with two hits': 0.249,
        'along oblique on soup2000: share full at max_hits 4': 0.097,
        'along -y on soup2000: share with two hits': 0.226,
        'along -y on soup2000: share full at max_hits 4': 0.082,
        'along five directions on soup2000: share with two hits': 0.237,
        'along five directions on soup2000: share full at max_hits 4': 0.101,
        'along oblique on soup2000+dup: share with two hits': 0.253,
        'along oblique on soup2000+dup: share full at max_hits 4': 0.109,
        'along oblique on soup2000+dup: rays with a tie': 11,
        'along oblique on soup2000+dup: rays with a tie at a cut': 6,
        'along -y on soup2000+dup: share with two hits': 0.226,
        'along -y on soup2000+dup: share full at max_hits 4': 0.089,
        'along -y on soup2000+dup: rays with a tie': 9,
        'along -y on soup2000+dup: rays with a tie at a cut': 4,
        'along five directions on soup2000+dup: share with two hits': 0.237,
        'along five directions on soup2000+dup: share full at max_hits 4': 0.113,
        'along five directions on soup2000+dup: rays with a tie': 11,
        'along five directions on soup2000+dup: rays with a tie at a cut': 7,
    },
    '300_200_-100': {
        'phantom acceptances on soup2000': 58,
        'grid rays on soup2000: share with two hits': 0.540,
        'grid rays on soup2000: share full at max_hits 4': 0.304,
        'phantom acceptances on soup2000+dup': 73,
        'grid rays on soup2000+dup: share with two hits': 0.543,
        'grid rays on soup2000+dup: share full at max_hits 4': 0.315,
        'grid rays on soup2000+dup: rays with a tie': 103,
        'grid rays on soup2000+dup: rays with a tie at a cut': 68,
        'along oblique on soup2000: share with two hits': 0.249,
        'along oblique on soup2000: share full at max_hits 4': 0.097,
        'along -y on soup2000: share with two hits': 0.226,
        'along -y on soup2000: share full at max_hits 4': 0.082,
        'along five directions on soup2000: share with two hits': 0.237,
        'along five directions on soup2000: share full at max_hits 4': 0.101,
        'along oblique on soup2000+dup: share with two hits': 0.253,
        'along oblique on soup2000+dup: share full at max_hits 4': 0.109,
        'along oblique on soup2000+dup: rays with a tie': 11,
        'along oblique on soup2000+dup: rays with a tie at a cut': 6,
        'along -y on soup2000+dup: share with two hits': 0.226,
        'along -y on soup2000+dup: share full at max_hits 4': 0.089,
        'along -y on soup2000+dup: rays with a tie': 9,
        'along -y on soup2000+dup: rays with a tie at a cut': 4,
        'along five directions on soup2000+dup: share with two hits': 0.237,
        'along five directions on soup2000+dup: share full at max_hits 4': 0.113,
        'along five directions on soup2000+dup: rays with a tie': 11,
        'along five directions on soup2000+dup: rays with a tie at a cut': 7,
    },
    '1000_1000_1000': {
        'phantom acceptances on soup2000': 58,
        'grid rays on soup2000: share with two hits': 0.544,
        'grid rays on soup2000: share full at max_hits 4': 0.305,
        'phantom acceptances on soup2000+dup': 54,
        'grid rays on soup2000+dup: share with two hits': 0.543,
        'grid rays on soup2000+dup: share full at max_hits 4': 0.312,
        'grid rays on soup2000+dup: rays with a tie': 102,
        'grid rays on soup2000+dup: rays with a tie at a cut': 68,
        'along oblique on soup2000: share with two hits': 0.249,
        'along oblique on soup2000: share full at max_hits 4': 0.093,
        'along -y on soup2000: share with two hits': 0.226,
        'along -y on soup2000: share full at max_hits 4': 0.082,
        'along five directions on soup2000: share with two hits': 0.237,
        'along five directions on soup2000: share full at max_hits 4': 0.101,
        'along oblique on soup2000+dup: share with two hits': 0.253,
        'along oblique on soup2000+dup: share full at max_hits 4': 0.105,
        'along oblique on soup2000+dup: rays with a tie': 11,
        'along oblique on soup2000+dup: rays with a tie at a cut': 6,
        'along -y on soup2000+dup: share with two hits': 0.226,
        'along -y on soup2000+dup: share full at max_hits 4': 0.089,
        'along -y on soup2000+dup: rays with a tie': 9,
        'along -y on soup2000+dup: rays with a tie at a cut': 4,
        'along five directions on soup2000+dup: share with two hits': 0.237,
        'along five directions on soup2000+dup: share full at max_hits 4': 0.113,
        'along five directions on soup2000+dup: rays with a tie': 11,
        'along five directions on soup2000+dup: rays with a tie at a cut': 7,
    },
    'origin_x1024': {
        'phantom acceptances on soup2000': 167,
        'grid rays on soup2000: share with two hits': 0.568,
        'grid rays on soup2000: share full at max_hits 4': 0.319,
        'phantom acceptances on soup2000+dup': 192,
        'grid rays on soup2000+dup: share with two hits': 0.574,
        'grid rays on soup2000+dup: share full at max_hits 4': 0.331,
        'grid rays on soup2000+dup: rays with a tie': 114,
        'grid rays on soup2000+dup: rays with a tie at a cut': 83,
        'along oblique on soup2000: share with two hits': 0.249,
        'along oblique on soup2000: share full at max_hits 4': 0.097,
        'along -y on soup2000: share with two hits': 0.226,
        'along -y on soup2000: share full at max_hits 4': 0.082,
        'along five directions on soup2000: share with two hits': 0.237,
        'along five directions on soup2000: share full at max_hits 4': 0.101,
        'along oblique on soup2000+dup: share with two hits': 0.253,
        'along oblique on soup2000+dup: share full at max_hits 4': 0.109,
        'along oblique on soup2000+dup: rays with a tie': 11,
        'along oblique on soup2000+dup: rays with a tie at a cut': 6,
        'along -y on soup2000+dup: share with two hits': 0.226,
        'along -y on soup2000+dup: share full at max_hits 4': 0.089,
        'along -y on soup2000+dup: rays with a tie': 9,
        'along -y on soup2000+dup: rays with a tie at a cut': 4,
        'along five directions on soup2000+dup: share with two hits': 0.237,
        'along five directions on soup2000+dup: share full at max_hits 4': 0.113,
        'along five directions on soup2000+dup: rays with a tie': 11,
        'along five directions on soup2000+dup: rays with a tie at a cut': 7,
    },
    'origin_div1024': {
        'phantom acceptances on soup2000': 168,
        'grid rays on soup2000: share with two hits': 0.475,
        'grid rays on soup2000: share full at max_hits 4': 0.286,
        'phantom acceptances on soup2000+dup': 193,
        'grid rays on soup2000+dup: share with two hits': 0.479,
        'grid rays on soup2000+dup: share full at max_hits 4': 0.296,
        'grid rays on soup2000+dup: rays with a tie': 92,
        'grid rays on soup2000+dup: rays with a tie at a cut': 64,
        'along oblique on soup2000: share with two hits': 0.249,
        'along oblique on soup2000: share full at max_hits 4': 0.097,
        'along -y on soup2000: share with two hits': 0.226,
        'along -y on soup2000: share full at max_hits 4': 0.082,
        'along five directions on soup2000: share with two hits': 0.237,
        'along five directions on soup2000: share full at max_hits 4': 0.101,
        'along oblique on soup2000+dup: share with two hits': 0.253,
        'along oblique on soup2000+dup: share full at max_hits 4': 0.109,
        'along oblique on soup2000+dup: rays with a tie': 11,
        'along oblique on soup2000+dup: rays with a tie at a cut': 6,
        'along -y on soup2000+dup: share with two hits': 0.226,
        'along -y on soup2000+dup: share full at max_hits 4': 0.089,
        'along -y on soup2000+dup: rays with a tie': 9,
        'along -y on soup2000+dup: rays with a tie at a cut': 4,
        'along five directions on soup2000+dup: share with two hits': 0.237,
        'along five directions on soup2000+dup: share full at max_hits 4': 0.113,
        'along five directions on soup2000+dup: rays with a tie': 11,
        'along five directions on soup2000+dup: rays with a tie at a cut': 7,
    },
    '40_-25_60_div1024': {
        'phantom acceptances on soup2000': 0,
        'grid rays on soup2000: share with two hits': 0.480,
        'grid rays on soup2000: share full at max_hits 4': 0.289,
        'phantom acceptances on soup2000+dup': 1,
        'grid rays on soup2000+dup: share with two hits': 0.485,
        'grid rays on soup2000+dup: share full at max_hits 4': 0.297,
        'grid rays on soup2000+dup: rays with a tie': 79,
        'grid rays on soup2000+dup: rays with a tie at a cut': 53,
        'along oblique on soup2000: share with two hits': 0.245,
        'along oblique on soup2000: share full at max_hits 4': 0.097,
        'along -y on soup2000: share with two hits': 0.218,
        'along -y on soup2000: share full at max_hits 4': 0.082,
        'along five directions on soup2000: share with two hits': 0.241,
        'along five directions on soup2000: share full at max_hits 4': 0.105,
        'along oblique on soup2000+dup: share with two hits': 0.249,
        'along oblique on soup2000+dup: share full at max_hits 4': 0.109,
        'along oblique on soup2000+dup: rays with a tie': 11,
        'along oblique on soup2000+dup: rays with a tie at a cut': 6,
        'along -y on soup2000+dup: share with two hits': 0.218,
        'along -y on soup2000+dup: share full at max_hits 4': 0.089,
        'along -y on soup2000+dup: rays with a tie': 9,
        'along -y on soup2000+dup: rays with a tie at a cut': 4,
        'along five directions on soup2000+dup: share with two hits': 0.241,
        'along five directions on soup2000+dup: share full at max_hits 4': 0.113,
        'along five directions on soup2000+dup: rays with a tie': 12,
        'along five directions on soup2000+dup: rays with a tie at a cut': 9,
    },
    '10_-7_5_div1024': {
        'phantom acceptances on soup2000': 2,
        'grid rays on soup2000: share with two hits': 0.482,
        'grid rays on soup2000: share full at max_hits 4': 0.289,
        'phantom acceptances on soup2000+dup': 10,
        'grid rays on soup2000+dup: share with two hits': 0.486,
        'grid rays on soup2000+dup: share full at max_hits 4': 0.297,
        'grid rays on soup2000+dup: rays with a tie': 85,
        'grid rays on soup2000+dup: rays with a tie at a cut': 61,
        'along oblique on soup2000: share with two hits': 0.249,
        'along oblique on soup2000: share full at max_hits 4': 0.097,
        'along -y on soup2000: share with two hits': 0.226,
        'along -y on soup2000: share full at max_hits 4': 0.082,
        'along five directions on soup2000: share with two hits': 0.237,
        'along five directions on soup2000: share full at max_hits 4': 0.101,
        'along oblique on soup2000+dup: share with two hits': 0.253,
        'along oblique on soup2000+dup: share full at max_hits 4': 0.109,
        'along oblique on soup2000+dup: rays with a tie': 11,
        'along oblique on soup2000+dup: rays with a tie at a cut': 6,
        'along -y on soup2000+dup: share with two hits': 0.226,
        'along -y on soup2000+dup: share full at max_hits 4': 0.089,
        'along -y on soup2000+dup: rays with a tie': 9,
        'along -y on soup2000+dup: rays with a tie at a cut': 4,
        'along five directions on soup2000+dup: share with two hits': 0.237,
        'along five directions on soup2000+dup: share full at max_hits 4': 0.113,
        'along five directions on soup2000+dup: rays with a tie': 11,
        'along five directions on soup2000+dup: rays with a tie at a cut': 7,
    },
    '0_0_4096': {
        'phantom acceptances on soup2000': 34,
        'grid rays on soup2000: share with two hits': 0.543,
        'grid rays on soup2000: share full at max_hits 4': 0.311,
        'phantom acceptances on soup2000+dup': 63,
        'grid rays on soup2000+dup: share with two hits': 0.541,
        'grid rays on soup2000+dup: share full at max_hits 4': 0.314,
        'grid rays on soup2000+dup: rays with a tie': 96,
        'grid rays on soup2000+dup: rays with a tie at a cut': 67,
        'along oblique on soup2000: share with two hits': 0.249,
        'along oblique on soup2000: share full at max_hits 4': 0.097,
        'along -y on soup2000: share with two hits': 0.222,
        'along -y on soup2000: share full at max_hits 4': 0.082,
        'along five directions on soup2000: share with two hits': 0.237,
        'along five directions on soup2000: share full at max_hits 4': 0.101,
        'along oblique on soup2000+dup: share with two hits': 0.253,
        'along oblique on soup2000+dup: share full at max_hits 4': 0.109,
        'along oblique on soup2000+dup: rays with a tie': 11,
        'along oblique on soup2000+dup: rays with a tie at a cut': 6,
        'along -y on soup2000+dup: share with two hits': 0.222,
        'along -y on soup2000+dup: share full at max_hits 4': 0.089,
        'along -y on soup2000+dup: rays with a tie': 9,
        'along -y on soup2000+dup: rays with a tie at a cut': 4,
        'along five directions on soup2000+dup: share with two hits': 0.237,
        'along five directions on soup2000+dup: share full at max_hits 4': 0.113,
        'along five directions on soup2000+dup: rays with a tie': 11,
        'along five directions on soup2000+dup: rays with a tie at a cut': 7,
    },
    '20_-14_10': {
        'phantom acceptances on soup2000': 73,
        'grid rays on soup2000: share with two hits': 0.541,
        'grid rays on soup2000: share full at max_hits 4': 0.301,
        'phantom acceptances on soup2000+dup': 93,
        'grid rays on soup2000+dup: share with two hits': 0.555,
        'grid rays on soup2000+dup: share full at max_hits 4': 0.318,
        'grid rays on soup2000+dup: rays with a tie': 99,
        'grid rays on soup2000+dup: rays with a tie at a cut': 70,
    },
}


def floors_missed(pname, shares, figures):
    """What a placement's inputs fail to show: a hit share outside SHARE, or a figure below half of FIGURES[pname]'s."""
    bad = {k: v for k, v in shares.items() if not SHARE[0] <= v <= SHARE[1]}
    for k, seen in FIGURES[pname].items():
        if k.startswith("phantom") and pl.RAY_GRID_CLASS[k.split(" on ")[1]][pname] != "binned":
            continue                                                # (phantoms are asked for where the grid walks)
        if not figures.get(k, 0) >= seen / 2 > 0:
            bad[k] = (figures.get(k), "floor", seen / 2)
    missing = set(figures) - set(FIGURES[pname])
    if missing:
        bad["not in FIGURES"] = sorted(missing)
    return bad
