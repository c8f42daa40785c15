"""The probe generators of silhouette.py against the CPU oracle: the conditions that keep test_gpu_silhouette_probes.py from being
vacuous, checked without a GPU.

Measured here (oracle's ClosestIntersection, every probe of the scene from the inside origin (0.125, -0.0625, 0.1875); share of probes
whose closest hit is their target triangle):

  scene     probes   all     inside  outside  inside at 2^-20  outside at 2^-20   border twin pairs in different bins
  shell     30288    0.507   0.919   0.095    0.774            0.268              0.331
  needles   27156    0.562   0.745   0.379    0.592            0.588              0.321
  soup150   31008    0.451   0.869   0.032    0.823            0.096              0.332
  grazing   12576    0.523   0.636   0.410    0.539            0.527              0.336
  walls     22464    0.300   0.543   0.056    0.470            0.126              0.331
  tips      30960    0.459   0.772   0.146    0.481            0.386              0.499

(tips: all 381 inside twins at 2^-20 of a tip vertex fall into another bin than the direction to their triangle's centroid.)

At delta = 2^-20 the probes straddle the float accept boundary in every scene: some inside twins are rejected and some outside
twins accepted.  From the two other origins the shares are lower (shell from outside: 0.323; from a vertex of triangle 0 every ray
that is not parallel to that triangle meets it at distance 0, so the share is that triangle's: 0.004) -- the condition of one third
is the inside origin's.  Tile-corner slivers that own their corner pixel in the oracle's index plane: 0.974 of 192 at yaw 0 (1.0 at
delta 2^-6, 2^-10 and 2^-14 pixels, 0.896 at 2^-17), 1.0 at yaw 0.3."""
import numpy as np
import pytest

import silhouette as sil

_cache = {}


def inside_case(oracle, name):
    """The scene's probes from the inside origin and the oracle's closest-hit index of each: computed once."""
    key = ("inside", name)
    if key not in _cache:
        tris, targets, crossings, scale = sil.scene_of(oracle, name)
        O = sil.origins_of(tris, scale, sil.offset_of(name))["inside"]
        p = sil.probes(tris, O, targets, crossings)
        idx = sil.oracle_index(oracle, tris, O, p["dir"])
        idx.setflags(write=False)
        _cache[key] = (tris, O, p, idx)
    return _cache[key]


@pytest.mark.parametrize("name", ["shell", "needles", "soup150", "grazing", "walls", "tips", "shell @ far", "needles @ far"])
def test_probes_reach_and_straddle_their_targets(oracle, name):
    tris, O, p, idx = inside_case(oracle, name)
    s = sil.shares(p, idx)
    split = sil.border_pairs_split(p)
    print(name, len(p), "probes", s, "border pairs split %.3f" % split)
    assert len(p) < 60000 and len(p) % 2 == 0
    assert np.array_equal(p["inside"][0::2], ~p["inside"][1::2]) and np.array_equal(p["target"][0::2], p["target"][1::2])
    for kind in (sil.EDGE, sil.VERTEX, sil.BORDER):
        assert (p["kind"] == kind).sum() >= 300, (name, kind)
    assert set(p["face"].tolist()) == set(range(6))
    if name in ("shell", "needles", "soup150", "tips", "shell @ far", "needles @ far"):
        assert s["all"] >= 1.0 / 3.0, s
    if name == "tips":
        # the tips reach into a bin of their own, and rays into them are accepted
        own, n = sil.tips_in_their_own_bin(p, tris, O)
        print("tips: inside twins at the tip in another bin than the centroid: %.3f of %d" % (own, n))
        assert n >= 0.95 * len(tris) and own >= 0.7, (own, n)
    # at the smallest delta the probes straddle the accept boundary: an inside twin rejected, an outside twin accepted
    small = p["delta"] == 0
    assert ((idx != p["target"]) & p["inside"] & small).any() and ((idx == p["target"]) & ~p["inside"] & small).any(), s
    assert split >= 0.1, split


def test_soup150_inside_the_full_soup(oracle):
    """Most of the first 150 triangles are hidden inside the 2000: equality only, no share asked (measured: 0.21 of inside twins)."""
    tris, targets, crossings, _ = sil.scene_of(oracle, "soup2000")
    p = sil.probes(tris, sil.INSIDE, targets, crossings)
    alone = inside_case(oracle, "soup150")[2]
    assert np.array_equal(p["dir"], alone["dir"]) and p["target"].max() == 149


def test_every_grid_and_both_bin_tests_are_reached(oracle):
    """Scene sizes on either side of the 2000 triangles at which the cube takes 128 bins a side, and walls whose boxes are more
    than 32 bins (the limit of the bin-by-bin test) and more than 64 bins of a face wide, across seams, with a vertex behind."""
    assert len(sil.scene_of(oracle, "shell")[0]) == 150 and len(sil.scene_of(oracle, "shell_dense")[0]) >= 2000 == len(sil.scene_of(oracle, "soup2000")[0])
    walls = sil.scene_of(oracle, "walls")[0].astype(np.float64)
    spans, behind = [], 0
    for t in walls:
        g = t[:9].reshape(3, 3) - sil.INSIDE
        k = np.abs(g.mean(0)).argmax()
        w = g[:, k] * np.sign(g[:, k].mean())
        behind += (w < 0).any()
        if (w > 0).all():
            u, v = g[:, (k + 1) % 3] / w, g[:, (k + 2) % 3] / w
            spans.append(((u.max() - u.min()) * 32, (v.max() - v.min()) * 32))
    spans = np.array(spans)
    assert ((spans > 32).all(axis=1) & (spans < 64).all(axis=1)).sum() >= 12 and (spans > 64).all(axis=1).sum() >= 6 and behind >= 6, (spans, behind)
    needles = sil.scene_of(oracle, "needles")[0].astype(np.float64)
    e = np.stack([needles[:, 3:6] - needles[:, 0:3], needles[:, 6:9] - needles[:, 3:6], needles[:, 0:3] - needles[:, 6:9]], axis=1)
    length = np.linalg.norm(e, axis=2).max(axis=1)
    height = np.linalg.norm(np.cross(e[:, 0], e[:, 1]), axis=1) / length
    assert np.median(length / height) >= 1000
    graz = sil.scene_of(oracle, "grazing")[0].astype(np.float64)
    n = np.cross(graz[:, 3:6] - graz[:, 0:3], graz[:, 6:9] - graz[:, 0:3])
    h = np.abs(((graz[:, 0:3] - sil.INSIDE) * n).sum(axis=1)) / np.linalg.norm(n, axis=1)
    assert h.max() < 1.1e-3 and h.min() > 0.5e-6 and (h < 2e-6).sum() >= 8, (h.min(), h.max())


def test_scaled_shells_keep_their_shape(oracle):
    for name, scale in (("shell x 3e-4", 3e-4), ("shell x 3e5", 3e5)):
        tris = sil.scene_of(oracle, name)[0]
        assert np.allclose(tris[:, :9], sil.scene_of(oracle, "shell")[0][:, :9].astype(np.float64) * scale, rtol=1e-6, atol=0)
        O = sil.origins_of(tris, scale)["inside"]
        p = sil.probes(tris, O)
        assert np.array_equal(p["target"], inside_case(oracle, "shell")[2]["target"])
    # part of the larger shell lies beyond the directions an origin fan bins (2^19): those rays sweep the table and are counted
    assert 0 < sil.outside_the_fan_window(p["dir"]).sum() < len(p) and not sil.outside_the_fan_window(inside_case(oracle, "shell")[2]["dir"]).any()


def test_shadow_records_lie_behind_their_probe(oracle):
    from mirt import HIT_DTYPE
    tris, O, p, idx = inside_case(oracle, "shell")
    scene, first = sil.with_receivers(tris)
    rec = sil.shadow_records(p, O, first, HIT_DTYPE)
    assert len(scene) == len(tris) + 6 and rec["index"].min() >= first and rec["index"].max() < len(scene)
    to_light = O.astype(np.float64) - rec["position"]
    assert ((scene[rec["index"], 9:12] * to_light).sum(axis=1) > 0).all()              # the receiver's normal faces the light
    k = np.linalg.norm(to_light, axis=1) / np.linalg.norm(p["point"] - O, axis=1)
    assert np.allclose(np.sort(np.unique(np.round(k, 3))), sil.SHADOW_STEPS)
    # a record behind a probe that reaches its target is in shadow, one behind a probe that reaches nothing is lit
    lights = np.array([[O[0], O[1], O[2], 1, 1, 1, 14]], np.float32)
    some = np.random.default_rng(1).permutation(len(p))[:256]
    lit = np.array([oracle.direct_light(scene, rec["position"][q], 1.0, int(rec["index"][q]), lights).any() for q in some])
    # (DirectLight normalises its own direction, so a probe within an ulp of a silhouette may fall to the other side)
    assert (lit == (idx[some] < 0)).mean() >= 0.9, (lit.mean(), (idx[some] < 0).mean())
    assert 0.25 <= lit.mean() <= 0.75


@pytest.mark.parametrize("name", ["shell", "needles", "shell @ far", "needles @ far"])
def test_shadow_records_a_position_resolves(oracle, name):
    """sil.resolved: at the world origin no record's float32 position is the light; at the far offset exactly the two 2^-20 twins
    of the light's own vertex are, and the oracle's DirectLight of every record that stays is finite."""
    from mirt import HIT_DTYPE
    tris, targets, crossings, scale = sil.scene_of(oracle, name)
    scene, first = sil.with_receivers(tris, scale, sil.offset_of(name))
    dropped = {}
    for oname, L in sil.origins_of(tris, scale, sil.offset_of(name)).items():
        p = sil.probes(tris, L, targets, crossings)
        rec = sil.shadow_records(p, L, first, HIT_DTYPE)
        assert rec["index"].min() >= first and ((scene[rec["index"], 9:12] * (L.astype(np.float64) - rec["position"])).sum(axis=1) >= 0).all()
        q, kept = sil.resolved(p, rec, L, name)
        dropped[oname] = len(p) - len(q)
        lights = np.array([[L[0], L[1], L[2], 1, 1, 1, 14]], np.float32)
        near = np.argsort(np.linalg.norm(kept["position"].astype(np.float64) - L, axis=1))[:32]            # the records nearest the light
        assert all(np.isfinite(oracle.direct_light(scene, kept["position"][k], 1.0, int(kept["index"][k]), lights)).all() for k in near), (name, oname)
    assert dropped == {"inside": 0, "outside": 0, "vertex": 2 if name.endswith("@ far") else 0}, dropped


@pytest.mark.parametrize("yaw", [0.0, 0.3])
def test_slivers_own_their_corner_pixels(oracle, yaw):
    rot = oracle.rot_from_yaw(yaw, 1.0)
    tris, tgt, dl = sil.scene_slivers(rot)
    assert len(tris) == 192 and np.bincount(dl).tolist() == [48] * 4
    assert set((tgt[:, 0] % 8).tolist()) == {0, 7} and set((tgt[:, 1] % 8).tolist()) == {0, 7}
    light = np.array([[0.0, -0.5, -0.7, 1, 1, 1, 14.0]], np.float32)
    r = oracle.raytrace(tris, sil.CAM, rot, sil.FOCAL, sil.W, sil.H, light, threads=4, want=("index",))
    share, per_delta = sil.sliver_ownership(r["index"], tgt, dl)
    print("yaw", yaw, "slivers owning their corner pixel: %.3f" % share, per_delta)
    assert share >= 0.8, (share, per_delta)
