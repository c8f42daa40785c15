"""Every binned path on scenes placed away from the world origin (tests/placement.py): frames, shading from records, single and
many-origin fans, rays along one and several directions, and the brute-force calls as controls -- each under BRUTE, BINNED and AUTO,
host and device forms, on soup2000, on Cornell + soup2000 and (the grids, B = 256) on soup33000.

Everything is compared bit for bit with the CPU oracle ON THE PLACED float32 INPUTS; there is no tolerance, and no placed result is
compared with a unit one.  The margins of the binning structures are stated in the operands' magnitudes (rt_binned.hpp, along.hpp,
DESIGN 3.2 / 5.1); an offset moves those apart from the scene's size, which no pure scaling does.

Beside equality: where the path's rule says binned -- placement.ALONG_CLASS for the grids, always for the cubes on these finite
scenes -- the statistics say so, the structure built by the first call (cube_source 1) and kept for the repeat (2); where the grid is
refused or gives up, BINNED runs the brute-force kernels, twice, building nothing; and no call touches another family's statistics.
The oracle's answers are computed once per placement and family and shared by the modes and forms compared with them; its hit share
of every batch lies in [0.05, 0.95] (checked without a GPU by test_placement_host.py as well).

test_in_place reaches the far placement from the unit upload by mirt_scene_transform and by mirt_scene_set_objects + mirt_scene_pose,
with structures of the unit scene held: every family again, on the downloaded rows, the first call rebuilding."""
import numpy as np
import pytest

import mirt
import placement as pl
import query_helpers as rq
from along_helpers import SHELLS, plant_odd_starts
from devbuf import DeviceArray, to_device
from test_gpu_along import GUARD, checked, closest as along_closest, occluded as along_occluded
from test_gpu_alongs import closest as alongs_closest, deal, occluded as alongs_occluded

pytestmark = pytest.mark.gpu

BRUTE, BINNED, AUTO = mirt.QUERY_BRUTE, mirt.QUERY_BINNED, mirt.QUERY_AUTO
W, H, FOCAL = 96, 64, 32.0
CAM = np.array([0.2, -0.1, -3.0])                                   # outside Cornell's box: the frame has misses
THIRD = np.array([[-0.375, 0.5, 0.25, 0.5, 1, 0.75, 9]], np.float32)
NRAYS = 1500                                                       # at most 2048 a batch
NBIG = 400                                                         # soup33000: at most 512
FRAME_SCENE, QUERY_SCENE, BIG_SCENE = "cornell+soup2000", "soup2000", "soup33000"
SHARE = (0.05, 0.95)
_cases = {}


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.set_query_mode(AUTO)
    mirt.set_profiling(False)
    mirt.set_soft_shadows(1)
    mirt.set_frames_in_flight(1)
    mirt.shutdown()


# ---- what a placement's calls are compared with: the oracle alone ---------------------------------------------------------------------

class Placed:
    """The placed inputs of every family and the oracle's answers on them, each computed once (no GPU).  `rows`: triangles that
    stand in for placement.placed_scene (test_in_place: the rows the library moved)."""

    def __init__(self, oracle, pname, rows=None):
        self.o, self.pname = oracle, pname
        self.T, self.s = pl.PLACEMENTS[pname]
        self.rows = rows or {}
        self.memo, self.shares = {}, {}

    def tris(self, name):
        return self.rows[name] if name in self.rows else pl.placed_scene(name, self.pname)

    def once(self, key, make):
        if key not in self.memo:
            v = make()
            for x in (v.values() if isinstance(v, dict) else v):
                if isinstance(x, np.ndarray):
                    x.setflags(write=False)
            self.memo[key] = v
        return self.memo[key]

    def place(self, x):
        return pl.place(x, self.T, self.s)

    def share(self, what, hits):
        self.shares[what] = float((hits["index"] >= 0).mean())

    # -- frames --
    def frames(self):
        def make():
            o, tris = self.o, self.tris(FRAME_SCENE)
            cam, rot = self.place(CAM), o.rot_from_yaw(0.1, 1.0)
            L = pl.place_lights(rq.LIGHTS, self.T, self.s)
            jit = self.place(rq.jitter(o, rq.LIGHTS[:1], 4, seed=5))
            configs = [("1 light", L[:1], 1, None), ("2 lights", L, 1, None), ("1 light x 4 samples", L[:1], 4, jit)]
            refs = [o.raytrace(tris, cam, rot, FOCAL, W, H, l, threads=4, samples=sm, jitter=j) for _, l, sm, j in configs]
            # The reference's "frustum" cull mixes the camera's WORLD z into its depth range (rasteriser.cpp:386, :400): away from
            # z = 0 it culls every triangle.  Both flag sets are compared; the frame is drawn with back-face culling alone.
            culled = {flags: o.cull(tris, cam, rot, FOCAL, W, H, flags) for flags in (3, 1)}
            rast = o.rasterise(tris, culled[1], cam, rot, FOCAL, W, H, L)
            self.shares["frame pixels"] = float((refs[0]["index"] >= 0).mean())
            self.shares["rasterised pixels"] = float((rast["index"] >= 0).mean())
            return dict(cam=cam, rot=rot, L=L, configs=configs, refs=refs, culled=culled, rast=rast)
        return self.once("frames", make)

    # -- the general batch: rays for the brute-force controls (soup2000), records for the shading calls (Cornell + soup2000) --
    def rays(self, scene, n=NRAYS, seed=7):
        def make():
            a, b = (1.7, 2.6) if scene == FRAME_SCENE else (1.5, 1.5)     # (Cornell's box is closed: starts and targets outside it too)
            u = rq.make_batch(n, a, b, seed=seed)
            rays = mirt.make_rays(self.place(u["start"]), pl.place_dirs(u["dir"], self.s))
            hits = rq.oracle_intersect(self.o, self.tris(scene), rays)
            self.share("rays on " + scene, hits)
            return dict(rays=rays, hits=hits)
        return self.once(("rays", scene, n, seed), make)

    def shading(self):
        def make():
            o, tris = self.o, self.tris(FRAME_SCENE)
            recs = self.rays(FRAME_SCENE)["hits"]
            L3 = pl.place_lights(np.concatenate([rq.LIGHTS, THIRD]), self.T, self.s)
            jit = self.place(rq.jitter(o, np.concatenate([rq.LIGHTS, THIRD]), 11, seed=3))
            want2 = rq.oracle_direct_light(o, tris, recs, L3[:2])
            want33 = rq.oracle_direct_light(o, tris, recs, L3, samples=11, jitter=jit)
            # DirectLight's shadow decisions (raytracer.cpp:306-315) for the first hit records, with the oracle's own operations
            sel = np.flatnonzero(recs["index"] >= 0)[:160]
            bits = np.zeros((len(sel), 2), bool)
            rdir = np.zeros(3, np.float32)
            for i, pos in enumerate(np.ascontiguousarray(recs["position"][sel], np.float32)):
                for j, p in enumerate(np.ascontiguousarray(L3[:2, :3])):
                    r = np.float32(o.lib.mirt_oracle_distance(pos, p))
                    o.lib.mirt_oracle_normalize((p - pos).astype(np.float32), rdir)
                    hit, _, dist, _ = o.closest_intersection(tris, p, (-rdir).astype(np.float32))
                    bits[i, j] = hit and dist < r * np.float32(0.99)
            self.shares["shadow bits set"] = float(bits.mean())
            self.shares["shadow bits, columns of one value"] = float((~(bits.any(axis=0) & ~bits.all(axis=0))).sum())
            return dict(recs=recs, L3=L3, jit=jit, want2=want2, want33=want33, sel=sel, bits=bits)
        return self.once("shading", make)

    # -- fans --
    def fan(self):
        def make():
            rng = np.random.default_rng(13)
            target = rng.uniform(-1.4, 1.4, (NRAYS, 3))
            origin = self.place(rq.INSIDE)
            dirs = pl.place_dirs((target - rq.INSIDE.astype(np.float64)).astype(np.float32), self.s)
            hits = rq.oracle_intersect(self.o, self.tris(QUERY_SCENE), mirt.make_rays(origin, dirs))
            self.share("single fan", hits)
            return dict(origin=origin, dirs=dirs, hits=hits)
        return self.once("fan", make)

    def fans(self):
        def make():
            rng = np.random.default_rng(17)
            tris = self.tris(QUERY_SCENE)
            v = rng.normal(size=3)
            ou = np.array([rq.INSIDE, pl.unit_scene(QUERY_SCENE)[0, 0:3], rq.OUTSIDE, rng.uniform(-0.4, 0.4, 3), v / np.linalg.norm(v) * 2.5], np.float64)
            origins = self.place(ou)
            origins[1] = tris[0, 0:3]                                # exactly on a vertex of triangle 0, as the scene holds it
            of = rng.integers(0, 5, NRAYS).astype(np.int32)
            target = rng.uniform(-1.4, 1.4, (NRAYS, 3))
            dirs = pl.place_dirs((target - ou[of]).astype(np.float32), self.s)
            hits = rq.oracle_intersect(self.o, tris, mirt.make_rays(origins[of], dirs))
            self.share("many-origin fans", hits)
            # limits at, one float above and one float below the closest distance (a miss: one unit of the scene)
            d = np.where(hits["index"] >= 0, hits["distance"], np.float32(self.s)).astype(np.float32)
            kind = np.arange(NRAYS) % 3
            limits = np.select([kind == 0, kind == 1], [d, np.nextafter(d, rq.INF)], np.nextafter(d, np.float32(0))).astype(np.float32)
            return dict(origins=origins, of=of, dirs=dirs, hits=hits, limits=limits, kind=kind, want=rq.expected(hits, limits))
        return self.once("fans", make)

    # -- along one direction, and along five --
    def starts(self, scene, n):
        u = rq.make_batch(n, 1.5, 1.0, seed=23)["start"]
        return plant_odd_starts(self.place(u), pl.extent_of(self.tris(scene)))

    def along(self, scene, dname, n=NRAYS):
        def make():
            starts, planted = self.starts(scene, n)
            d = pl.place_dirs(pl.ALONG_DIRS[dname], self.s)
            hits = rq.oracle_intersect(self.o, self.tris(scene), mirt.make_rays(starts, d))
            self.share("along %s on %s" % (dname, scene), hits)
            limits, kind = rq.limits_for(hits)
            return dict(d=d, starts=starts, planted=planted, hits=hits, limits=limits, want=rq.expected(hits, limits), want_null=rq.expected(hits, None))
        return self.once(("along", scene, dname, n), make)

    def alongs(self):
        def make():
            starts, planted = self.starts(QUERY_SCENE, NRAYS)
            dirs = np.ascontiguousarray([pl.place_dirs(d, self.s) for d in pl.ALONG_DIRS.values()], np.float32)
            of = deal(NRAYS, len(dirs))
            hits = rq.oracle_intersect(self.o, self.tris(QUERY_SCENE), mirt.make_rays(starts, dirs[of]))
            self.share("along five directions", hits)
            limits, kind = rq.limits_for(hits)
            return dict(dirs=dirs, of=of, starts=starts, hits=hits, limits=limits, want=rq.expected(hits, limits), want_null=rq.expected(hits, None))
        return self.once("alongs", make)

    def everything(self):
        """Every family's inputs and answers (what test_placement_host.py looks at without a GPU)."""
        self.frames(); self.shading(); self.rays(QUERY_SCENE); self.fan(); self.fans(); self.alongs()
        for scene in (QUERY_SCENE, FRAME_SCENE):
            for dname in pl.SINGLE_DIRS:
                self.along(scene, dname)
        self.along(BIG_SCENE, "oblique", NBIG)
        return self.shares


def vacuous(shares):
    """The entries of Placed.shares outside what a batch has to show: hit shares in [0.05, 0.95], shadow bits that differ."""
    bad = {k: v for k, v in shares.items() if not k.startswith("shadow bits") and not SHARE[0] <= v <= SHARE[1]}
    if shares.get("shadow bits, columns of one value", 0):
        bad["shadow bits, columns of one value"] = shares["shadow bits, columns of one value"]
    return bad


def case_of(oracle, pname):
    if pname not in _cases:
        _cases[pname] = Placed(oracle, pname)
    return _cases[pname]


# ---- plumbing: modes, statistics, device forms -------------------------------------------------------------------------------------------

KINDS = {"frame": mirt.stats, "light": mirt.query_stats, "mask": mirt.shadow_mask_stats, "fan": mirt.fan_stats,
         "occlusion": mirt.occlusion_stats, "along": mirt.along_stats}


class only:
    """The calls inside touch the statistics of kind `mine` (or none) and no other family's."""

    def __init__(self, mine, what):
        self.mine, self.what = mine, what

    def __enter__(self):
        self.before = {k: f() for k, f in KINDS.items() if k != self.mine}
        return self

    def __exit__(self, etype, exc, tb):
        if etype is None:
            after = {k: f() for k, f in KINDS.items() if k != self.mine}
            for k in after:
                assert after[k] == self.before[k], "%s: touched the %s statistics: %r -> %r" % (self.what, k, self.before[k], after[k])


class mode:
    def __init__(self, m):
        self.m = m

    def __enter__(self):
        mirt.set_query_mode(self.m)

    def __exit__(self, *exc):
        mirt.set_query_mode(AUTO)


def upload(name, tris, warm=None):
    """How a placed scene arrives by default: uploaded as it is (a new scene version: nothing is held)."""
    mirt.scene_upload(tris)


def brute_stats(st, what):
    assert st["mode_used"] == BRUTE and st["cube_source"] == 0 and st["cube_bins"] == 0, (what, st)


def built_then_kept(st, first, what, bins=None):
    """A binned call: the structure built by the first call after the scene arrived, kept from then on."""
    assert st["mode_used"] == BINNED and st["cube_source"] == (1 if first else 2), (what, "first" if first else "repeat", st)
    assert st["cube_bins"] >= 8 and st["shells"] >= 1 and (bins is None or st["cube_bins"] == bins), (what, st)


def auto_stats(st, what):
    assert st["mode_used"] in (BRUTE, BINNED) and (st["cube_source"] != 0) == (st["mode_used"] == BINNED), (what, st)
    return "binned" if st["mode_used"] == BINNED else "brute"


def note(case, family, text):
    print("PATH %-18s %-26s %s" % (case.pname, family, text))


def records_device(call, n, *arrays):
    """A closest-hit device form: the arrays on the device, fresh records with four of guard behind them."""
    bufs = [to_device(a) for a in arrays]
    d_hits = to_device(np.concatenate([mirt.fresh_hits(n), mirt.fresh_hits(4)]))
    try:
        call(*[b.ptr for b in bufs], d_hits.ptr)
        mirt.sync()
        back = np.frombuffer(d_hits.read().tobytes(), mirt.HIT_DTYPE)
        assert back[n:].tobytes() == mirt.fresh_hits(4).tobytes(), "wrote beyond %d records" % n
        return back[:n].copy()
    finally:
        for b in bufs + [d_hits]:
            b.free()


def bytes_device(call, n, what, *arrays):
    """An occlusion device form: the arrays on the device (None stays None), 0xAA bytes with a guard behind them."""
    bufs = [None if a is None else to_device(a) for a in arrays]
    with DeviceArray((n + GUARD,), np.uint8, 0xAA) as d_out:
        try:
            call(*[None if b is None else b.ptr for b in bufs], d_out.ptr)
            return checked(d_out.read(), n, what)
        finally:
            for b in bufs:
                if b is not None:
                    b.free()


def same_bytes(got, want, what):
    assert np.array_equal(got, want), "%s: %d bytes differ (first at ray %d)" % (what, int((got != want).sum()), int(np.flatnonzero(got != want)[0]))


def bit_matrix(mask, npos):
    j = np.arange(npos)
    return ((mask[j >> 5, :] >> (j & 31).astype(np.uint32)[:, None]) & 1).T.astype(bool)


# ---- the families ------------------------------------------------------------------------------------------------------------------------

def run_frames(case, arrive=upload):
    f = case.frames()
    tris, view = case.tris(FRAME_SCENE), mirt.make_view(f["cam"], f["rot"], FOCAL, W, H)

    def frame(l, sm, j, m):
        mirt.set_soft_shadows(sm, j)
        try:
            with only("frame", "a ray-traced frame"):
                return mirt.raytrace(view, l, mode=m, want_intersection=True)
        finally:
            mirt.set_soft_shadows(1)

    arrive(FRAME_SCENE, tris, lambda: [frame(f["L"][:1], 1, None, mirt.RT_BINNED) for _ in range(2)])
    paths = []
    for k, ((cname, l, sm, j), ref) in enumerate(zip(f["configs"], f["refs"])):
        for mname, m in (("binned", mirt.RT_BINNED), ("brute", mirt.RT_BRUTE)):
            got = frame(l, sm, j, m)
            what = "%s: frame, %s, %s" % (case.pname, cname, mname)
            assert np.array_equal(got["index"], ref["index"]), "%s: index differs in %d pixels" % (what, int((got["index"] != ref["index"]).sum()))
            rq.same_bits(got["dist"], ref["dist"], what + ": distance")
            rq.same_bits(got["pos"], ref["pos"], what + ": position")
            rq.same_bits(got["rgb"], ref["rgb"], what + ": rgb")
            assert np.array_equal(got["xrgb"], ref["xrgb"]), what + ": xrgb"
            st = got["stats"]
            assert st["primary_rays"] == W * H and st["shadow_rays"] == ref["nshadow"], (what, st)
            if m == mirt.RT_BRUTE:
                assert st["mode_used"] == mirt.RT_BRUTE, (what, st)
            else:
                assert st["mode_used"] == mirt.RT_BINNED, (what, st)           # finite operands inside the filter's range: the frame bins
                if k == 0:
                    assert st["bins_reused"] == 0, (what, st)                  # the first binned frame after the scene arrived
            paths.append("%s %s" % (cname, {mirt.RT_BRUTE: "brute", mirt.RT_BINNED: "binned"}.get(st["mode_used"], st["mode_used"])))
    # the rasteriser on the same view
    for flags in (3, 1):
        culled = mirt.cull(tris, view, flags)
        assert np.array_equal(culled, f["culled"][flags]), "%s: cull (flags %d) differs for %d triangles" % (case.pname, flags, int((culled != f["culled"][flags]).sum()))
    mirt.scene_set_culled(culled)
    with only("frame", "a rasterised frame"):
        got = mirt.rasterise(view, f["L"])
    ref = f["rast"]
    what = "%s: rasterised frame" % case.pname
    assert np.array_equal(got["index"], ref["index"]), "%s: owner differs in %d pixels" % (what, int((got["index"] != ref["index"]).sum()))
    rq.same_bits(got["depth"], ref["depth"], what + ": depth")
    rq.same_bits(got["rgb"], ref["rgb"], what + ": rgb")
    assert np.array_equal(got["xrgb"], ref["xrgb"]), what + ": xrgb"
    note(case, "frames", "; ".join(paths) + "; rasterised")


def run_shading(case, arrive=upload):
    sh = case.shading()
    tris, recs, n = case.tris(FRAME_SCENE), sh["recs"], len(sh["recs"])

    def light_host(L):
        with only("light", "mirt_direct_light"):
            return mirt.direct_light(recs, L), mirt.query_stats()

    def light_device(L):
        d_hits = to_device(recs)
        try:
            with DeviceArray((n, 3), np.float32, 0x5A) as d_rgb, only("light", "mirt_direct_light_device"):
                mirt.direct_light_device(d_hits.ptr, n, L, d_rgb.ptr)
                return d_rgb.read(), mirt.query_stats()
        finally:
            d_hits.free()

    def mask_host(L):
        with only("mask", "mirt_shadow_mask"):
            return mirt.shadow_mask(recs, L), mirt.shadow_mask_stats()

    def mask_device(L, npos):
        words = mirt.mask_words(npos)
        d_hits = to_device(recs)
        try:
            with DeviceArray((words * n + 8,), np.uint32, 0x5A) as d_mask, only("mask", "mirt_shadow_mask_device"):
                mirt.shadow_mask_device(d_hits.ptr, n, L, d_mask.ptr)
                got = d_mask.read()
            assert (got[words * n:] == 0x5A5A5A5A).all(), "wrote beyond the mask's planes"
            return got[:words * n].reshape(words, n), mirt.shadow_mask_stats()
        finally:
            d_hits.free()

    def relight_device(L, mask):
        d_hits, d_mask = to_device(recs), to_device(mask)
        try:
            with DeviceArray((n, 3), np.float32, 0x5A) as d_rgb, only(None, "mirt_direct_light_masked_device"):
                mirt.direct_light_masked_device(d_hits.ptr, n, L, d_mask.ptr, d_rgb.ptr)
                return d_rgb.read()
        finally:
            d_hits.free(); d_mask.free()

    paths = []
    for lname, L, samples, jit, npos, want in (("2 lights", sh["L3"][:2], 1, None, 2, sh["want2"]), ("3 x 11 positions", sh["L3"], 11, sh["jit"], 33, sh["want33"])):
        mirt.set_soft_shadows(samples, jit)
        try:
            with mode(BINNED):
                arrive(FRAME_SCENE, tris, lambda: light_host(L))
            what = "%s: %s" % (case.pname, lname)
            with mode(BRUTE):
                got, st = light_host(L)
                brute_stats(st, what)
                rq.same_bits(got, want, what + ", direct_light, brute, host form")
                mask, st = mask_host(L)
                brute_stats(st, what)
                masks = {"brute": mask}
            with mode(BINNED):
                got, st = light_host(L)
                built_then_kept(st, True, what + ", direct_light")
                rq.same_bits(got, want, what + ", direct_light, binned, host form")
                got, st = light_device(L)
                built_then_kept(st, False, what + ", direct_light_device")
                rq.same_bits(got, want, what + ", direct_light, binned, device form")
                mask, st = mask_host(L)
                built_then_kept(st, False, what + ", shadow_mask (DirectLight's cubes serve it)")
                dmask, st = mask_device(L, npos)
                built_then_kept(st, False, what + ", shadow_mask_device")
                assert np.array_equal(dmask, mask), what + ": device mask"
                masks["binned"] = mask
            with mode(AUTO):
                got, st = light_device(L)
                took = auto_stats(st, what)
                rq.same_bits(got, want, what + ", direct_light, auto")
                masks["auto"], st = mask_host(L)
                auto_stats(st, what)
            for mname, mask in masks.items():
                assert mask.shape == (mirt.mask_words(npos), n) and np.array_equal(mask, masks["brute"]), "%s: the %s mask differs from the brute one" % (what, mname)
            with only(None, "mirt_direct_light_masked"):
                rq.same_bits(mirt.direct_light_masked(recs, L, mask), want, what + ", mask then relight, host form")
            rq.same_bits(relight_device(L, mask), want, what + ", mask then relight, device form")
            if npos == 2:
                got = bit_matrix(mask, 2)[sh["sel"]]
                assert np.array_equal(got, sh["bits"]), "%s: %d shadow decisions differ from the oracle's" % (what, int((got != sh["bits"]).sum()))
            paths.append("%s: binned built, kept; auto %s" % (lname, took))
        finally:
            mirt.set_soft_shadows(1)
    note(case, "shading from records", "; ".join(paths))


def run_fan(case, arrive=upload):
    f = case.fan()
    tris, origin, dirs, want = case.tris(QUERY_SCENE), f["origin"], f["dirs"], f["hits"]

    def host():
        with only("fan", "mirt_intersect_from"):
            return mirt.intersect_from(origin, dirs), mirt.fan_stats()

    def dev():
        with only("fan", "mirt_intersect_from_device"):
            got = records_device(lambda d, h: mirt.intersect_from_device(origin, d, len(dirs), h), len(dirs), dirs)
            return got, mirt.fan_stats()

    with mode(BINNED):
        arrive(QUERY_SCENE, tris, host)
    what = "%s: single fan" % case.pname
    with mode(BRUTE):
        got, st = dev()
        brute_stats(st, what)
        rq.same_hits(got, want, what + ", brute, device form")
    with mode(BINNED):
        got, st = host()
        built_then_kept(st, True, what)
        rq.same_hits(got, want, what + ", binned, host form")
        got, st = dev()
        built_then_kept(st, False, what)
        rq.same_hits(got, want, what + ", binned, device form")
    with mode(AUTO):
        got, st = host()
        took = auto_stats(st, what)
        rq.same_hits(got, want, what + ", auto")
    note(case, "single fan", "binned built, kept (%d bins a side); auto %s" % (st["cube_bins"] if st["cube_bins"] else 0, took))


def run_fans(case, arrive=upload):
    f = case.fans()
    tris, origins, of, dirs, n = case.tris(QUERY_SCENE), f["origins"], f["of"], f["dirs"], len(f["of"])

    def closest(form):
        with only("fan", "mirt_intersect_fans"):
            if form == "host":
                return mirt.intersect_fans(origins, of, dirs), mirt.fan_stats()
            got = records_device(lambda o, d, h: mirt.intersect_fans_device(origins, o, d, n, h), n, of, dirs)
            return got, mirt.fan_stats()

    def occluded(form, what):
        with only("occlusion", "mirt_occluded_fans"):
            if form == "host":
                buf = np.full(n + GUARD, 0xAA, np.uint8)
                mirt.occluded_fans(origins, of, dirs, f["limits"], buf[:n])
                return checked(buf, n, what), mirt.occlusion_stats()
            got = bytes_device(lambda o, d, l, out: mirt.occluded_fans_device(origins, o, d, n, l, out), n, what, of, dirs, f["limits"])
            return got, mirt.occlusion_stats()

    with mode(BINNED):
        arrive(QUERY_SCENE, tris, lambda: closest("host"))
    what = "%s: fans from 5 origins" % case.pname
    with mode(BRUTE):
        got, st = closest("host")
        brute_stats(st, what)
        rq.same_hits(got, f["hits"], what + ", brute, host form")
        got, st = occluded("device", what)
        brute_stats(st, what)
        same_bytes(got, f["want"], what + ", occluded, brute, device form")
    with mode(BINNED):
        got, st = closest("device")
        built_then_kept(st, True, what)
        rq.same_hits(got, f["hits"], what + ", binned, device form")
        got, st = closest("host")
        built_then_kept(st, False, what)
        rq.same_hits(got, f["hits"], what + ", binned, host form")
        for form in ("host", "device"):
            got, st = occluded(form, what)
            built_then_kept(st, False, what + ", occluded (the fans' cubes serve it)")
            same_bytes(got, f["want"], what + ", occluded, binned, %s form" % form)
    with mode(AUTO):
        got, st = closest("device")
        took = auto_stats(st, what)
        rq.same_hits(got, f["hits"], what + ", auto")
        got, st = occluded("host", what)
        auto_stats(st, what)
        same_bytes(got, f["want"], what + ", occluded, auto")
    # the three kinds of limit decide as the oracle's distances say: at and below the closest distance nothing is nearer
    hit = f["hits"]["index"] >= 0
    assert f["want"][hit & (f["kind"] == 1)].all() and not f["want"][f["kind"] != 1].any() and (hit & (f["kind"] == 1)).sum() > 20
    note(case, "many-origin fans", "closest and occluded: binned built, kept; auto %s" % took)


def run_along(case, scene, dname, arrive=upload, n=NRAYS, bins=32, forms=("host", "device")):
    a = case.along(scene, dname, n)
    tris, d, starts = case.tris(scene), a["d"], a["starts"]
    cls = pl.along_class(scene, case.pname, dname)
    what = "%s: along %s on %s (%s)" % (case.pname, dname, scene, cls)

    def closest(form, m):
        with only("along", "mirt_intersect_along"):
            return along_closest(form, d, starts, m)

    def occluded(form, m, limits):
        with only("along", "mirt_occluded_along"):
            return along_occluded(form, d, starts, limits, m, what)

    arrive(scene, tris, lambda: closest("host", BINNED))
    got, st = closest(forms[-1], BRUTE)
    brute_stats(st, what)
    rq.same_hits(got, a["hits"], what + ", brute")
    got, st = occluded(forms[0], BRUTE, a["limits"])
    brute_stats(st, what)
    same_bytes(got, a["want"], what + ", occluded, brute")
    for k, form in enumerate(forms + forms[:1]):
        got, st = closest(form, BINNED)
        if cls == "binned":
            built_then_kept(st, k == 0, what, bins)
            assert st["shells"] == SHELLS, (what, st)
        else:
            brute_stats(st, what + ", BINNED call %d" % k)          # refused, or gave up: nothing is built, this time or the next
        rq.same_hits(got, a["hits"], what + ", BINNED call %d, %s form" % (k, form))
    for form in forms:
        for limits, want in ((a["limits"], a["want"]), (None, a["want_null"])):
            got, st = occluded(form, BINNED, limits)
            if cls == "binned":
                built_then_kept(st, False, what + ", occluded (one structure serves both kinds)", bins)
            else:
                brute_stats(st, what + ", occluded")
            same_bytes(got, want, what + ", occluded, BINNED, %s form%s" % (form, "" if limits is not None else ", no limits"))
    got, st = closest(forms[-1], AUTO)
    took = auto_stats(st, what)
    assert cls == "binned" or took == "brute", (what, st)
    rq.same_hits(got, a["hits"], what + ", auto")
    got, st = occluded(forms[0], AUTO, a["limits"])
    same_bytes(got, a["want"], what + ", occluded, auto")
    note(case, "along %s, %s" % (dname, scene), "%s: BINNED %s; auto %s" % (cls, "built, kept (B = %d)" % bins if cls == "binned" else "ran brute twice, built nothing", took))


def run_alongs(case, arrive=upload):
    a = case.alongs()
    tris, dirs, of, starts = case.tris(QUERY_SCENE), a["dirs"], a["of"], a["starts"]
    cls = pl.alongs_class(QUERY_SCENE, case.pname)
    what = "%s: along five directions (%s)" % (case.pname, cls)

    def closest(form, m):
        with only("along", "mirt_intersect_alongs"):
            return alongs_closest(form, dirs, of, starts, m)

    def occluded(form, m, limits):
        with only("along", "mirt_occluded_alongs"):
            return alongs_occluded(form, dirs, of, starts, limits, m, what)

    arrive(QUERY_SCENE, tris, lambda: closest("host", BINNED))
    got, st = closest("host", BRUTE)
    brute_stats(st, what)
    rq.same_hits(got, a["hits"], what + ", brute")
    got, st = occluded("device", BRUTE, a["limits"])
    brute_stats(st, what)
    same_bytes(got, a["want"], what + ", occluded, brute")
    for k, form in enumerate(("device", "host", "device")):
        got, st = closest(form, BINNED)
        if cls == "binned":
            built_then_kept(st, k == 0, what, 32)
        else:
            brute_stats(st, what + ", BINNED call %d" % k)
        rq.same_hits(got, a["hits"], what + ", BINNED call %d, %s form" % (k, form))
    for form, limits, want in (("host", a["limits"], a["want"]), ("device", None, a["want_null"])):
        got, st = occluded(form, BINNED, limits)
        if cls == "binned":
            built_then_kept(st, False, what + ", occluded", 32)
        else:
            brute_stats(st, what + ", occluded")
        same_bytes(got, want, what + ", occluded, BINNED, %s form" % form)
    got, st = closest("host", AUTO)
    took = auto_stats(st, what)
    assert cls == "binned" or took == "brute", (what, st)
    rq.same_hits(got, a["hits"], what + ", auto")
    got, st = occluded("host", AUTO, a["limits"])
    same_bytes(got, a["want"], what + ", occluded, auto")
    note(case, "along five directions", "%s: BINNED %s; auto %s" % (cls, "built, kept" if cls == "binned" else "ran brute, built nothing", took))


def run_brute_controls(case, arrive=upload):
    r = case.rays(QUERY_SCENE)
    tris, rays, hits, n = case.tris(QUERY_SCENE), r["rays"], r["hits"], len(r["rays"])
    limits, kind = rq.limits_for(hits)
    want = rq.expected(hits, limits)
    arrive(QUERY_SCENE, tris, None)
    what = "%s: mirt_intersect / mirt_occluded" % case.pname
    for mname, m in (("brute", BRUTE), ("binned", BINNED), ("auto", AUTO)):           # (the mode is not theirs to look at)
        with mode(m):
            with only(None, "mirt_intersect"):
                rq.same_hits(mirt.intersect(rays), hits, what + ", host form, mode " + mname)
                got = records_device(lambda d, h: mirt.intersect_device(d, n, h), n, rays)
                rq.same_hits(got, hits, what + ", device form, mode " + mname)
            with only("occlusion", "mirt_occluded"):
                buf = np.full(n + GUARD, 0xAA, np.uint8)
                mirt.occluded(rays, limits, buf[:n])
                same_bytes(checked(buf, n, what), want, what + ", host form, mode " + mname)
                got = bytes_device(lambda d, l, out: mirt.occluded_device(d, n, l, out), n, what, rays, limits)
                same_bytes(got, want, what + ", device form, mode " + mname)
                brute_stats(mirt.occlusion_stats(), what)
    note(case, "brute controls", "brute")


# ---- the tests: one family and one placement each ---------------------------------------------------------------------------------------

PNAMES = list(pl.PLACEMENTS)


@pytest.mark.parametrize("pname", PNAMES)
def test_batches_are_not_vacuous(oracle, pname):
    """In every placement the oracle's hit share of each batch lies in [0.05, 0.95], and shadow bits differ between records."""
    shares = case_of(oracle, pname).everything()
    print(pname, {k: round(v, 3) for k, v in shares.items()})
    assert not vacuous(shares), vacuous(shares)


@pytest.mark.parametrize("pname", PNAMES)
def test_frames(oracle, pname):
    run_frames(case_of(oracle, pname))


@pytest.mark.parametrize("pname", PNAMES)
def test_shading_from_records(oracle, pname):
    run_shading(case_of(oracle, pname))


@pytest.mark.parametrize("pname", PNAMES)
def test_single_fan(oracle, pname):
    run_fan(case_of(oracle, pname))


@pytest.mark.parametrize("pname", PNAMES)
def test_many_origin_fans(oracle, pname):
    run_fans(case_of(oracle, pname))


@pytest.mark.parametrize("pname", PNAMES)
def test_along_one_direction(oracle, pname):
    for scene in (QUERY_SCENE, FRAME_SCENE):
        for dname in pl.SINGLE_DIRS:
            run_along(case_of(oracle, pname), scene, dname)


@pytest.mark.parametrize("pname", PNAMES)
def test_along_one_direction_on_a_grid_of_256_cells_a_side(oracle, pname):
    run_along(case_of(oracle, pname), BIG_SCENE, "oblique", n=NBIG, bins=256, forms=("device",))


@pytest.mark.parametrize("pname", PNAMES)
def test_along_five_directions(oracle, pname):
    run_alongs(case_of(oracle, pname))


@pytest.mark.parametrize("pname", PNAMES)
def test_brute_controls(oracle, pname):
    run_brute_controls(case_of(oracle, pname))


def test_every_class_of_grid_is_met():
    """The three outcomes of a grid all occur among the calls above."""
    met = {pl.along_class(s, p, d) for s in (QUERY_SCENE, FRAME_SCENE) for p in PNAMES for d in pl.SINGLE_DIRS}
    met |= {pl.alongs_class(QUERY_SCENE, p) for p in PNAMES} | {pl.along_class(BIG_SCENE, p, "oblique") for p in PNAMES}
    assert met == {"binned", "gave_up", "no_grid"}, met


# ---- getting there in place ----------------------------------------------------------------------------------------------------------------

EYE = np.eye(3, dtype=np.float32).ravel()


@pytest.mark.parametrize("how", ["scene_transform", "set_objects + pose"])
def test_in_place(oracle, how):
    """The far placement reached from the unit upload, with the unit scene's structures held (each family's first binned call is made
    on the unit scene before the move): the box mirt_scene_info reports is numpy's of the downloaded rows, every family equals the
    oracle on those rows, and the first call after the move rebuilds (cube_source 1, bins_reused 0: the families' own assertions)."""
    T, s = pl.PLACEMENTS[pl.FAR]
    assert s == 1.0

    def arrive(name, tris, warm):
        unit = pl.unit_scene(name)
        mirt.scene_upload(unit)
        if warm is not None:
            warm()                                                  # (the unit scene's structure, and results nobody looks at)
        if how == "scene_transform":
            mirt.scene_transform(0, len(unit), EYE, T)
        else:
            mirt.scene_set_objects([(0, 0, len(unit))])
            mirt.scene_pose([np.concatenate([EYE, np.asarray(T, np.float32)])])

    rows = {}
    for name in (QUERY_SCENE, FRAME_SCENE, BIG_SCENE):
        arrive(name, None, None)
        got = mirt.scene_download()
        info = mirt.scene_info()
        v = got[:, :9].reshape(-1, 3)
        assert info["n"] == len(got) and info["finite"] == 1, info
        assert np.array_equal(info["bbox_lo"], v.min(axis=0)) and np.array_equal(info["bbox_hi"], v.max(axis=0)), (name, info, v.min(axis=0), v.max(axis=0))
        # one rounding a coordinate: the vertices are placement.place's, so ALONG_CLASS speaks of these rows too
        assert np.array_equal(got[:, :9], pl.placed_scene(name, pl.FAR)[:, :9]), name
        assert np.array_equal(got, mirt.transform(pl.unit_scene(name), EYE, T)), name
        got.setflags(write=False)
        rows[name] = got
    case = Placed(oracle, pl.FAR, rows)
    case.pname = pl.FAR
    run_frames(case, arrive)
    run_shading(case, arrive)
    run_fan(case, arrive)
    run_fans(case, arrive)
    for scene in (QUERY_SCENE, FRAME_SCENE):
        for dname in pl.SINGLE_DIRS:
            run_along(case, scene, dname, arrive)
    run_along(case, BIG_SCENE, "oblique", arrive, n=NBIG, bins=256, forms=("device",))
    run_alongs(case, arrive)
    run_brute_controls(case, arrive)
    assert not vacuous(case.shares), vacuous(case.shares)
