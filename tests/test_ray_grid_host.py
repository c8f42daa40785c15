"""What the arbitrary-ray grid (mirt_set_ray_grid, mirt_get_ray_grid_stats) shows without a GPU: tests/cpp/ray_grid_test.cpp -- the
filing predicate and the walk of grid/ray_grid.hpp against the exact float test on seeded (ray, triangle) pairs, once per placement of
tests/placement.py, and how the suite's scenes are filed --, the calls' checks without a device, and the layout the Python shims hand
to the C side."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mirt
import ray_grid_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# accepted pairs whose exact half-line misses the triangle by more than a cell, over the ten placements and three grids: half of
# what the run shows (156)
PHANTOM_FLOOR = 78
OFFERED_CAP = 1.0 / 4.0                              # test_gpu_ray_grid.py: rows offered < rays * n / 4 on soup2000's uniform segments


@pytest.fixture(scope="module")
def grid_test(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ray_grid") / "ray_grid_test")
    # the header is HIP source: the host side alone, with the library's floating-point contract
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-w",
                    os.path.join(ROOT, "tests", "cpp", "ray_grid_test.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def test_every_accepted_pair_is_offered(grid_test):
    """The seeded pairs once per placement and grid size: no accepted pair is missed -- unbounded, and bounded by its own distance --,
    phantoms occur, and the same pairs do trip a structure whose rho, kappa, h and pads are zero."""
    import placement as pl
    args = ["placements"] + ["%.17g" % x for T, s in pl.PLACEMENTS.values() for x in tuple(T) + (s,)]
    r = subprocess.run([grid_test] + args, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    m = re.search(r"placements (\d+) grids (\d+) refused (\d+) gave_up (\d+) rays (\d+) unfit (\d+) pairs (\d+) accepted (\d+) phantoms (\d+) "
                  r"misses (\d+) bounded_misses (\d+) zero_margin_misses (\d+)", r.stdout)
    v = dict(zip(("placements", "grids", "refused", "gave_up", "rays", "unfit", "pairs", "accepted", "phantoms", "misses", "bounded", "zero"), map(int, m.groups())))
    assert v["placements"] == len(pl.PLACEMENTS) and v["grids"] == 3 * len(pl.PLACEMENTS)
    assert v["misses"] == 0 and v["bounded"] == 0
    assert v["accepted"] > 100000 and v["unfit"] > 0
    assert v["phantoms"] >= PHANTOM_FLOOR, "only %d phantom pairs: the generator no longer reaches the rounding-noise case" % v["phantoms"]
    assert v["zero"] > 0, "a structure without margins misses nothing: the pairs do not probe the margins"
    # some placement is binned at every grid size, some is refused or gives up
    assert v["refused"] + v["gave_up"] > 0 and v["refused"] + v["gave_up"] < v["grids"]


@pytest.mark.parametrize("name,cells", [("cornell", 4), ("wall", 8), ("soup2000", 16)])
def test_suite_scenes_are_filed(grid_test, tmp_path, name, cells):
    """The GPU tests rely on these: the three scenes do not give up at the origin, and soup2000's uniform segments are forecast
    fewer rows than the GPU test's bound allows."""
    tris = H.scene(name)
    path = str(tmp_path / "scene.f32")
    np.ascontiguousarray(tris, np.float32).tofile(path)
    r = subprocess.run([grid_test, path], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    m = re.search(r"n (\d+) G (\d+) pairs (\d+) cell_pairs (\d+) plane_pairs (\d+) every (\d+) every_share ([\d.]+) gave_up (\d) offered_share ([\d.]+) "
                  r"accepted (\d+) misses (\d+)", r.stdout)
    n, G, every, gave_up, offered, accepted, misses = (int(m.group(1)), int(m.group(2)), int(m.group(6)), int(m.group(8)), float(m.group(9)),
                                                        int(m.group(10)), int(m.group(11)))
    assert n == len(tris) and G == cells == H.grid_of(tris)[0]
    assert gave_up == 0 and every <= max(n // 8, 64) and misses == 0 and accepted > 0
    if name == "soup2000":
        assert offered < 0.8 * OFFERED_CAP, "a ray is offered %.4f of the scene: no room under the GPU test's bound" % offered


def test_placed_scenes_are_filed_as_the_class_table_says(grid_test, tmp_path):
    """placement.RAY_GRID entry by entry, from the header alone: the tool's scene-file mode on the placed scenes -- a descriptor or
    none, the every-ray list within grid_every_cap(n) or beyond it, the plane-index pairs and every-ray rows the GPU test compares the
    library's statistics with --, and no accepted pair of the tool's uniform segments missed anywhere."""
    import placement as pl
    seen = {}
    for scene, rows in pl.RAY_GRID.items():
        assert list(rows) and set(rows) == set(pl.GRID_PLACEMENTS), scene
        for pname, (want, plane_pairs, every_rows) in rows.items():
            tris = pl.placed_scene(scene, pname)
            path = str(tmp_path / "placed.f32")
            np.ascontiguousarray(tris, np.float32).tofile(path)
            r = subprocess.run([grid_test, path], capture_output=True, text=True, timeout=120)
            what = "%s at %s" % (scene, pname)
            print("%-17s %-18s %s" % (scene, pname, r.stdout.strip().replace("\n", " | ")))
            assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (what, r.stdout + r.stderr)
            n, cap = len(tris), max(len(tris) // 8, 64)             # ray_grid.hpp: grid_every_cap
            if "no_grid" in r.stdout:
                got = "no_grid"
            else:
                m = re.search(r"n (\d+) G (\d+) pairs \d+ cell_pairs \d+ plane_pairs (\d+) every (\d+) every_share [\d.]+ gave_up (\d) offered_share [\d.]+ "
                              r"accepted (\d+) misses (\d+)", r.stdout)
                gn, G, pp, every, gave_up, accepted, misses = map(int, m.groups())
                assert gn == n and G == pl.RAY_GRID_CELLS[scene] == H.grid_of(tris)[0], (what, r.stdout)
                assert " misses 0 " in r.stdout and misses == 0 and accepted > 0, (what, r.stdout)
                assert gave_up == (every > cap), (what, r.stdout)
                got = "gave_up" if gave_up else "binned"
                if got == "binned":
                    assert every <= cap, (what, r.stdout)
                assert (pp, every) == (plane_pairs, every_rows), "%s: %d plane pairs and %d every-ray rows, the table says %d and %d" % (what, pp, every, plane_pairs, every_rows)
            assert got == want, "%s is %s, the table says %s" % (what, got, want)
            seen.setdefault(got, set()).add((scene, pname))
    # the two placements of the test this one replaces, as it asserted them
    assert pl.RAY_GRID_CLASS["soup2000"]["3_0_0"] == "binned" and pl.RAY_GRID_CLASS["soup2000"]["1000_1000_1000"] != "binned"
    # every class the table names occurs, the edge placement bins, and the step behind it on the same line does not
    assert set(seen) == {c for rows in pl.RAY_GRID_CLASS.values() for c in rows.values()} and {"binned", "gave_up"} <= set(seen), seen
    assert pl.RAY_GRID_CLASS["soup2000"][pl.GRID_EDGE] == "binned" and pl.RAY_GRID_CLASS["cornell+soup2000"][pl.GRID_EDGE] == "binned"
    # the plane index grows with the offset until the grid gives up: what the edge placement is there for
    pp = [pl.RAY_GRID["soup2000"][p][1] for p in ("unit", "3_0_0", "10_-7_5", pl.GRID_EDGE)]
    assert pp == sorted(pp) and pp[-1] > 50 * pp[0], pp
    # a pure scaling moves nothing
    for rows in pl.RAY_GRID.values():
        assert rows["unit"] == rows["origin_x1024"] == rows["origin_div1024"]


def test_calls_need_a_device_and_the_layout_is_the_headers():
    assert C.sizeof(mirt.RayGridStats) == 6 * 4 + 4 * 4 + 6 * 8
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    body = re.search(r"typedef struct mirt_ray_grid_stats \{(.*?)\} mirt_ray_grid_stats;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(u?int\d+_t)\s+(\w+);", body, re.M)
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    assert [(n, ctype[t]) for t, n in fields] == list(mirt.RayGridStats._fields_)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.set_ray_grid(True)
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.ray_grid_stats()
