"""What the placed scenes' tests (tests/placement.py, test_gpu_placement.py) show without a GPU: the placement arithmetic, and that
the oracle alone finds every batch of test_gpu_placement.py worth asking -- hit shares in [0.05, 0.95] and shadow bits that differ
between records, in every placement."""
import numpy as np
import pytest

import mirt
import placement as pl
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
