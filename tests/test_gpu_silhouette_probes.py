"""The binning chain probed black-box with rays placed by hand (silhouette.py): a (bin, triangle) pair that frame_may_see, add_bbox,
box_to_bins, the tests in units of four bins, bin_walk_large or bin_jointly_empty (csrc/rt_binned.hpp, csrc/rt_binned.hip) drop
shows only on a ray that lies in that bin and is accepted by that triangle -- a ray within a few ulps of the triangle's silhouette,
in a bin the triangle barely enters.  Random rays and pixel grids do not find those; these do.

  fans     mirt.intersect_from under QUERY_BINNED -- through the cube around the origin that light_cache_ensure builds, the builder of
           the frames' light cubes -- against the same call under QUERY_BRUTE and mirt.intersect on {O, dir}: bit for bit on every
           probe, and against the oracle's ClosestIntersection on a fixed shuffled 1024 of them.  Once more with incoming records
           at the probe's own hit distance: the record loses the tie, the hit replaces it, the list does not end before it.
  shadows  mirt.direct_light with the probe origins as lights and records behind the probe points: the same cube, lists ended at
           0.99 r.  QUERY_BINNED against QUERY_BRUTE on every record, 1024 of them against the oracle's DirectLight.
  slivers  camera bins serve pixel centres only, so there the triangle is the adversary: tips that reach a tile's corner pixel by
           2^-6 .. 2^-17 of a pixel from the diagonal neighbour tile.  RT_BINNED against RT_BRUTE on all four planes.

Scenes, origins and what each is for: silhouette.py and test_silhouette_probes_host.py, which also holds the measured shares.  The
grid of the cube (64 bins a side below 2000 triangles, 128 from there on, 256 by MIRT_CUBE_BINS) and the binning kernels' workgroup
(MIRT_BIN_WG) are read once per process: shell, needles, walls and tips run again in a child process per combination.  A failing probe
is printed with its kind, delta, twin, bin, triangle and origin: its cause is to be found by reading the code."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_RAYS = 1024
SCENES = ("shell", "shell_dense", "needles", "walls", "grazing", "tips", "soup150", "soup2000", "shell x 3e-4", "shell x 3e5", "shell @ far", "needles @ far")
LIGHT = np.array([[0.0, -0.5, -0.7, 1.0, 1.0, 1.0, 14.0]], np.float32)
BAND = (13, 101)


# ---- comparisons that name the probe ------------------------------------------------------------------------------------------

def same_hits(got, want, p, tris, origin, bins, what):
    """same_hits of test_gpu_fan_query.py: index, distance and position bit for bit on every probe; the first failures in full."""
    bad = np.flatnonzero((got["index"] != want["index"]) | (got["distance"].view(np.uint32) != want["distance"].view(np.uint32)) |
                         (got["position"].view(np.uint32) != want["position"].view(np.uint32)).any(axis=1))
    if len(bad):
        import silhouette as sil
        lines = ["%s: %d of %d probes differ" % (what, len(bad), len(p))]
        for q in bad[:6]:
            lines.append("probe %d: got %r, want %r\n  %s" % (q, got[q].tolist(), want[q].tolist(), sil.describe(p[q], tris, origin, bins)))
        pytest.fail("\n".join(lines), pytrace=False)
    assert got.tobytes() == want.tobytes(), what


def same_light(got, want, p, rec, tris, origin, bins, what):
    bad = np.flatnonzero((np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).any(axis=1))
    if len(bad):
        import silhouette as sil
        lines = ["%s: %d of %d records differ" % (what, len(bad), len(p))]
        for q in bad[:6]:
            lines.append("record %d at %r naming %d: got %r, want %r\n  %s" % (
                q, rec["position"][q].tolist(), rec["index"][q], got[q].tolist(), want[q].tolist(), sil.describe(p[q], tris, origin, bins)))
        pytest.fail("\n".join(lines), pytrace=False)


def expected_bins(n):
    env = os.environ.get("MIRT_CUBE_BINS", "")
    return int(env) if env in ("64", "128", "256") else (64 if n < 2000 else 128)


# ---- fans ------------------------------------------------------------------------------------------------------------------------

def fan(mirt, origin, dirs, mode, hits=None):
    mirt.set_query_mode(mode)
    try:
        out = mirt.intersect_from(origin, dirs, hits)
        return out, mirt.fan_stats()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


def check_fans(mirt, oracle, name, with_oracle=True):
    """Every origin of one scene; returns per origin the shares of probes whose closest hit, by brute force, is their target."""
    import silhouette as sil
    from query_helpers import oracle_intersect
    tris, targets, crossings, scale = sil.scene_of(oracle, name)
    bins = expected_bins(len(tris))
    mirt.scene_upload(tris)
    out = {}
    for oname, O in sil.origins_of(tris, scale, sil.offset_of(name)).items():
        what = "%s from %s" % (name, oname)
        p = sil.probes(tris, O, targets, crossings)
        assert 3000 < len(p) < 60000, (what, len(p))
        dirs = np.ascontiguousarray(p["dir"])
        rays = mirt.make_rays(O, dirs)
        want = mirt.intersect(rays)
        brute, sb = fan(mirt, O, dirs, mirt.QUERY_BRUTE)
        binned, st = fan(mirt, O, dirs, mirt.QUERY_BINNED)
        assert sb["mode_used"] == mirt.QUERY_BRUTE and sb["cube_bins"] == 0, (what, sb)
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_bins"] == bins, (what, st)
        same_hits(brute, want, p, tris, O, bins, what + ": brute fan vs mirt.intersect")
        same_hits(binned, want, p, tris, O, bins, what + ": binned fan vs mirt.intersect")
        # the counting kernel is another instantiation: the same answers, and no ray that the bins cover sweeps the table instead.
        # Directions whose largest component lies outside [2^-32, 2^19) take no bin by design (fan_dir_of): only the shell scaled
        # by 3e5, and by 3e-4 seen from its own vertex, have any, and exactly those are counted
        swept = int(sil.outside_the_fan_window(dirs).sum())
        assert swept == 0 or name in ("shell x 3e5", "shell x 3e-4"), (what, swept)
        mirt.set_profiling(True)
        try:
            counted, cst = fan(mirt, O, dirs, mirt.QUERY_BINNED)
        finally:
            mirt.set_profiling(False)
        assert cst["mode_used"] == mirt.QUERY_BINNED and cst["cube_bins"] == bins and cst["shadow_rays"] == len(p), (what, cst)
        assert cst["fallback_records"] == swept, (what, cst, swept)
        assert 0 < cst["tests"] <= cst["candidates"], (what, cst)
        same_hits(counted, want, p, tris, O, bins, what + ": binned fan with counters vs mirt.intersect")
        if with_oracle:
            some = np.sort(np.random.default_rng(2).permutation(len(p))[:ORACLE_RAYS])
            same_hits(binned[some], oracle_intersect(oracle, tris, rays[some]), p[some], tris, O, bins, what + ": binned fan vs oracle")
        # carried records at the probe's own hit distance: the record loses the tie and the hit still replaces it
        hit = brute["index"] >= 0
        rec = mirt.fresh_hits(len(p))
        rec["distance"][hit] = brute["distance"][hit]
        rec["index"][hit] = 7
        rec["position"][hit] = (9, 9, 9)
        for mode in (mirt.QUERY_BINNED, mirt.QUERY_BRUTE):
            got, st = fan(mirt, O, dirs, mode, rec)
            assert st["mode_used"] == mode
            same_hits(got, brute, p, tris, O, bins, what + ": carried records, mode %d" % mode)
        same_hits(mirt.intersect(rays, rec), brute, p, tris, O, bins, what + ": carried records, mirt.intersect")
        on = brute["index"] == p["target"]
        small = p["delta"] == 0
        out[oname] = {"all": float(on.mean()), "inside": float(on[p["inside"]].mean()), "outside": float(on[~p["inside"]].mean()),
                      "rejected inside twins at 2^-20": int((~on & p["inside"] & small).sum()),
                      "accepted outside twins at 2^-20": int((on & ~p["inside"] & small).sum()),
                      "border pairs split": sil.border_pairs_split(p), "rows per ray": cst["candidates"] / len(p)}
    print(name, "grid", bins, out)
    return out


def check_conditions(name, got):
    """The conditions test_silhouette_probes_host.py checks with the oracle, again from the brute-force result."""
    s = got["inside"]
    # (the "@ far" scenes: a direction is float32(P - O), so the deltas a float resolves in it are the unit scene's, 2^-20 included --
    # it is positions, not directions, that lose them at the far offset; test_silhouette_probes_host.py has the oracle's word)
    if name in ("shell", "needles", "soup150", "tips", "shell @ far", "needles @ far"):
        assert s["all"] >= 1.0 / 3.0, (name, s)
    if name in ("shell", "needles", "soup150", "grazing", "walls", "tips", "shell @ far", "needles @ far"):
        assert s["rejected inside twins at 2^-20"] >= 1 and s["accepted outside twins at 2^-20"] >= 1, (name, s)
    assert s["border pairs split"] >= 0.1, (name, s)


@pytest.fixture(scope="module")
def mirt_on():
    import mirt
    mirt.init(0)
    yield mirt
    mirt.set_query_mode(mirt.QUERY_AUTO)
    mirt.set_profiling(False)
    mirt.set_soft_shadows(1)
    mirt.shutdown()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_fan_probes(mirt_on, oracle, name):
    check_conditions(name, check_fans(mirt_on, oracle, name))


def child(names):
    """One process per (MIRT_CUBE_BINS, MIRT_BIN_WG): both are read once."""
    sys.path[:0] = [os.path.join(ROOT, "cpp-raytracer-rasterizer_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
    import mirt
    from mirt_oracle import Oracle
    oracle = Oracle()
    mirt.init(0)
    try:
        for name in names:
            check_conditions(name, check_fans(mirt, oracle, name, with_oracle=False))
            check_shadows(mirt, oracle, name, with_oracle=False, origins=("inside",))
    finally:
        mirt.shutdown()
    print("ok")


@pytest.mark.gpu
@pytest.mark.parametrize("wg", [256, 512])
@pytest.mark.parametrize("bins", [64, 128, 256])
def test_fan_probes_on_every_grid(bins, wg):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "shell", "needles", "walls", "tips"],
                       env=dict(os.environ, MIRT_CUBE_BINS=str(bins), MIRT_BIN_WG=str(wg)), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("grid %d " % bins) == 8, r.stdout[-3000:]              # every scene's fans and its shadows say theirs


# ---- shadows -----------------------------------------------------------------------------------------------------------------------

def light_query(mirt, recs, lights, mode):
    mirt.set_query_mode(mode)
    try:
        out = mirt.direct_light(recs, lights)
        return out, mirt.query_stats()
    finally:
        mirt.set_query_mode(mirt.QUERY_AUTO)


def check_shadows(mirt, oracle, name, with_oracle=True, origins=("inside", "outside", "vertex")):
    """The probe origins as lights, one at a time; returns the share of lit records (brute force) per light."""
    import silhouette as sil
    tris, targets, crossings, scale = sil.scene_of(oracle, name)
    scene, first = sil.with_receivers(tris, scale, sil.offset_of(name))
    bins = expected_bins(len(scene))
    mirt.scene_upload(scene)
    mirt.set_soft_shadows(1)
    lit = {}
    for oname, L in sil.origins_of(tris, scale, sil.offset_of(name)).items():
        if oname not in origins:
            continue
        what = "%s lit from %s" % (name, oname)
        p = sil.probes(tris, L, targets, crossings)
        rec = sil.shadow_records(p, L, first, mirt.HIT_DTYPE)
        p, rec = sil.resolved(p, rec, L, name)
        lights = np.array([[L[0], L[1], L[2], 1.0, 1.0, 1.0, 14.0 * scale * scale]], np.float32)
        brute, sb = light_query(mirt, rec, lights, mirt.QUERY_BRUTE)
        binned, st = light_query(mirt, rec, lights, mirt.QUERY_BINNED)
        assert sb["mode_used"] == mirt.QUERY_BRUTE, (what, sb)
        assert st["mode_used"] == mirt.QUERY_BINNED and st["cube_bins"] == bins, (what, st)
        same_light(binned, brute, p, rec, tris, L, bins, what + ": binned vs brute")
        mirt.set_profiling(True)
        try:
            counted, st = light_query(mirt, rec, lights, mirt.QUERY_BINNED)
        finally:
            mirt.set_profiling(False)
        assert st["mode_used"] == mirt.QUERY_BINNED and st["shadow_rays"] == len(p) and st["fallback_records"] == 0, (what, st)
        same_light(counted, brute, p, rec, tris, L, bins, what + ": binned with counters vs brute")
        if with_oracle:
            from query_helpers import oracle_direct_light
            some = np.sort(np.random.default_rng(2).permutation(len(p))[:ORACLE_RAYS])
            same_light(binned[some], oracle_direct_light(oracle, scene, rec[some], lights), p[some], rec[some], tris, L, bins, what + ": binned vs oracle")
        assert np.isfinite(brute).all() and (brute >= 0).all()
        lit[oname] = (int(brute.any(axis=1).sum()), len(p), st["candidates"] / len(p))
    print(name, "grid", bins, "lit records, records, rows per record:", lit)
    return lit


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_shadow_probes(mirt_on, oracle, name):
    lit = check_shadows(mirt_on, oracle, name)
    if name == "shell":
        # neither outcome is rare: lit and shadowed records each make up a quarter at least
        n_lit, n = sum(v[0] for v in lit.values()), sum(v[1] for v in lit.values())
        assert 0.25 <= n_lit / n <= 0.75, lit
        assert 0.25 <= lit["inside"][0] / lit["inside"][1] <= 0.75, lit


# ---- camera tile-corner slivers ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("yaw", [0.0, 0.3])
def test_tile_corner_slivers(mirt_on, oracle, yaw):
    import silhouette as sil
    from devbuf import DeviceArray
    mirt = mirt_on
    W, H = sil.W, sil.H
    rot = oracle.rot_from_yaw(yaw, 1.0)
    tris, tgt, dl = sil.scene_slivers(rot)
    mirt.scene_upload(tris)
    view = mirt.make_view(sil.CAM, rot, sil.FOCAL, W, H)
    ref = oracle.raytrace(tris, sil.CAM, rot, sil.FOCAL, W, H, LIGHT, threads=4, want=("index",))["index"]
    share, per_delta = sil.sliver_ownership(ref, tgt, dl)
    print("yaw", yaw, "slivers owning their corner pixel: %.3f" % share, per_delta)
    assert share >= 0.8, (share, per_delta)
    for y0, y1 in ((0, H), BAND):
        out = {}
        for mode in (mirt.RT_BRUTE, mirt.RT_BINNED):
            planes = {"xrgb": DeviceArray((H, W), np.uint32, 0x11), "index": DeviceArray((H, W), np.int32, 0x11),
                      "dist": DeviceArray((H, W), np.float32, 0x11), "pos": DeviceArray((H, W, 3), np.float32, 0x11)}
            try:
                mirt.raytrace_device(view, LIGHT, (0.2, 0.2, 0.2), mode, y0, y1, 0, planes["xrgb"].ptr, W * 4,
                                     d_index=planes["index"].ptr, d_dist=planes["dist"].ptr, d_pos=planes["pos"].ptr)
                st = mirt.stats()
                assert st["mode_used"] == mode, (yaw, mode, st["mode_used"])
                out[mode] = {k: pl.read() for k, pl in planes.items()}
            finally:
                for pl in planes.values():
                    pl.free()
        for k in ("xrgb", "index", "dist", "pos"):
            a, b = out[mirt.RT_BINNED][k].view(np.uint32), out[mirt.RT_BRUTE][k].view(np.uint32)
            if not np.array_equal(a, b):
                ys, xs = np.nonzero((a != b).reshape(H, W, -1).any(axis=2))
                owners = [(int(x), int(y), int(out[mirt.RT_BRUTE]["index"][y, x]), int(out[mirt.RT_BINNED]["index"][y, x])) for x, y in zip(xs[:8], ys[:8])]
                lines = ["yaw %s rows %d..%d: %s differs at %d pixels; (x, y, brute index, binned index): %r" % (yaw, y0, y1, k, len(ys), owners)]
                for x, y, ib, _ in owners[:4]:
                    if ib >= 0:
                        lines.append("triangle %d: %r, tip %g pixels past the centre of pixel %r" % (ib, tris[ib, :9].tolist(), sil.SLIVER_DELTAS[dl[ib]], tgt[ib].tolist()))
                pytest.fail("\n".join(lines), pytrace=False)
        assert np.array_equal(out[mirt.RT_BINNED]["index"][y0:y1], ref[y0:y1]), "yaw %s rows %d..%d: index plane vs oracle" % (yaw, y0, y1)
        owned = out[mirt.RT_BINNED]["index"][tgt[:, 1], tgt[:, 0]] == np.arange(len(tgt))
        inband = (tgt[:, 1] >= y0) & (tgt[:, 1] < y1)
        assert owned[inband].mean() >= 0.8


if __name__ == "__main__":
    child(sys.argv[1:])
