"""What the placed scenes' tests (tests/placement.py, test_gpu_placement.py) show without a GPU: the placement arithmetic, and that
the oracle alone finds every batch of test_gpu_placement.py worth asking -- hit shares in [0.05, 0.95] and shadow bits that differ
between records, in every placement.  Likewise for test_gpu_placement_grid.py (placed_grid.py): hit shares in the same range, and floors --
half of what the oracle shows, placed_grid.FIGURES -- under the share of rays with two hits and with a full list at max_hits 4, the
tie scene's rays with an equal-distance pair and with one straddling a cut, and the phantom acceptances where the ray grid bins."""
import numpy as np
import pytest

import mirt
import placement as pl
import placed_grid as pg
from test_gpu_placement import Placed, vacuous


def test_place_rounds_once():
    x = np.array([[0.1, -0.7, 0.3], [1.0, 1.0, -1.0]], np.float32)
    T, s = (300.0, 200.0, -100.0), 2.0 ** -10
    got = pl.place(x, T, s)
    assert got.dtype == np.float32 and np.array_equal(got, (x.astype(np.float64) * s + np.array(T)).astype(np.float32))
    # not the float32 product rounded and then the float32 sum: one rounding
    assert np.array_equal(pl.place(x, (0, 0, 0), 1.0), x) and np.array_equal(pl.place_dirs(x, 2.0 ** 10), x * np.float32(1024))
    tris = mirt.scene_soup(41, 50, 0.2)
    placed = pl.place_tris(tris, T, s)
    assert np.array_equal(placed[:, 9:], tris[:, 9:]) and not np.array_equal(placed[:, :9], tris[:, :9])
    L = pl.place_lights(np.array([[0, -0.5, -0.75, 1, 1, 1, 14]], np.float32), T, 2.0)
    assert L[0, 6] == 56.0 and np.array_equal(L[0, :3], np.array([300, 199, -101.5], np.float32)) and np.array_equal(L[0, 3:6], [1, 1, 1])


def test_the_listed_placements():
    want = {((0, 0, 0), 1.0), ((3, 0, 0), 1.0), ((10, -7, 5), 1.0), ((300, 200, -100), 1.0), ((1000, 1000, 1000), 1.0), ((0, 0, 0), 2.0 ** 10),
            ((0, 0, 0), 2.0 ** -10), ((40, -25, 60), 2.0 ** -10), ((10, -7, 5), 2.0 ** -10), ((0, 0, 4096), 1.0)}
    assert {(tuple(T), s) for T, s in pl.PLACEMENTS.values()} == want
    for scene, rows in pl.ALONG_CLASS.items():
        assert set(rows) == set(pl.PLACEMENTS) and all(len(r) == len(pl.ALONG_DIRS) for r in rows.values()), scene
    # a scene hundreds of times farther from the origin than it is wide
    far = pl.placed_scene("soup2000", pl.FAR)
    v = far[:, :9].reshape(-1, 3)
    assert pl.extent_of(far) / (v.max(axis=0) - v.min(axis=0)).max() > 100


@pytest.mark.parametrize("pname", list(pl.PLACEMENTS))
def test_batches_are_not_vacuous(oracle, pname):
    shares = Placed(oracle, pname).everything()
    print(pname, {k: round(v, 3) for k, v in shares.items()})
    assert not vacuous(shares), vacuous(shares)


def test_the_grid_placements_and_the_tie_scene():
    assert list(pl.GRID_PLACEMENTS)[:len(pl.PLACEMENTS)] == list(pl.PLACEMENTS) and set(pl.GRID_PLACEMENTS) - set(pl.PLACEMENTS) == {pl.GRID_EDGE}
    assert pl.GRID_PLACEMENTS[pl.GRID_EDGE] == ((20.0, -14.0, 10.0), 1.0)
    for scene, rows in pl.RAY_GRID_CLASS.items():
        assert set(rows) == set(pl.GRID_PLACEMENTS) and set(rows.values()) <= {"binned", "gave_up", "no_grid"}, scene
    assert set(pg.FIGURES) == set(pl.GRID_PLACEMENTS)
    # placed duplicates stay exact duplicates, in every placement
    unit = pl.unit_scene(pl.TIE_SCENE)
    assert len(unit) == 2100 and np.array_equal(unit[:2000], pl.unit_scene("soup2000"))
    for pname in pl.GRID_PLACEMENTS:
        t = pl.placed_scene(pl.TIE_SCENE, pname)
        assert t[2000:].tobytes() == t[:pl.TIE_ROWS].tobytes() and np.array_equal(t[:2000], pl.placed_scene("soup2000", pname)), pname


@pytest.mark.parametrize("pname", list(pl.GRID_PLACEMENTS))
def test_grid_and_ordered_batches_are_not_vacuous(oracle, pname):
    """The ray grid's and the ordered hits' inputs, with the oracle alone: every hit share in [0.05, 0.95]; every other figure at or
    above half of what placed_grid.FIGURES records for the placement; the planted unfit rays of every kind among the rays."""
    case = pg.PlacedGrid(oracle, pname)
    shares, figures = case.everything()
    print(pname, {k: round(v, 3) for k, v in shares.items()})
    print(pname, {k: round(v, 3) for k, v in figures.items()})
    assert shares and not pg.floors_missed(pname, shares, figures), pg.floors_missed(pname, shares, figures)
    for scene in pg.SCENES:
        g = case.grid_rays(scene)
        r6, planted = g["r6"], np.arange(5, len(g["r6"]), pg.UNFIT_EVERY)
        assert len(r6) <= 1500 and g["unfit"][planted].all() and g["unfit"][:pg.NSMALL].sum() >= 2 and not g["unfit"].all()
        with np.errstate(invalid="ignore"):
            R = pl.extent_of(case.tris(scene))
            assert (np.abs(r6[planted, 0:3]).max(axis=1) > 2 * R).any() and (~r6[planted, 3:6].any(axis=1)).any() and np.isnan(r6[planted]).any()
            assert np.isinf(r6[planted, 3:6]).any() and (np.abs(r6[planted, 3:6]).max(axis=1) >= 2.0 ** 19).any()
            assert ((np.abs(r6[planted, 3:6]).max(axis=1) < 2.0 ** -32) & r6[planted, 3:6].any(axis=1)).any()
        assert g["nphantom_rays"] >= 20 or pl.RAY_GRID_CLASS[scene][pname] != "binned", "%s on %s: the phantom generators found %d rays" % (pname, scene, g["nphantom_rays"])
        if pname in pl.PLACEMENTS:
            assert case.ordered_alongs(scene)["planted"].sum() >= 3
