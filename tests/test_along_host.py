"""What the ray queries along one direction (mirt_intersect_along*, mirt_occluded_along*, mirt_get_along_stats) show without a GPU:
tests/cpp/along_bins_test.cpp -- the binning predicate against the exact test on seeded triples, and the forecast of the rows a
ray is offered on soup2000 under the GPU test's direction --, the argument checks, and the layout the Python shims hand to the C
side."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mirt
from along_helpers import OBLIQUE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOT_INITIALISED = -3, -2
NAMES = ("mirt_intersect_along", "mirt_intersect_along_device", "mirt_occluded_along", "mirt_occluded_along_device", "mirt_get_along_stats")
OFFERED_CAP = 1.0 / 8.0                             # test_gpu_along.py: candidates <= rays * n // 8


@pytest.fixture(scope="module")
def bins_test(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("along") / "along_bins_test")
    # the header is HIP source: the host side alone, with the library's floating-point contract
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-w",
                    os.path.join(ROOT, "tests", "cpp", "along_bins_test.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def test_accepted_starts_find_their_triangle(bins_test):
    """The seeded triples once per placement of placement.PLACEMENTS: no predicate failure anywhere, and filed, every-ray and
    refused triples each occur in some placement."""
    import placement as pl
    args = ["placements"] + ["%.17g" % x for T, s in pl.PLACEMENTS.values() for x in tuple(T) + (s,)]
    r = subprocess.run([bins_test] + args, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    m = re.search(r"placements (\d+) with filed (\d+) with every-ray (\d+) with refused (\d+)", r.stdout)
    assert int(m.group(1)) == len(pl.PLACEMENTS) and min(int(m.group(k)) for k in (2, 3, 4)) >= 1, r.stdout
    assert " failures 0\n" in r.stdout and r.stdout.count("placement (") == len(pl.PLACEMENTS)
    # the built-in list is the same one
    assert subprocess.run([bins_test], capture_output=True, text=True, timeout=300).stdout == r.stdout


def test_soup2000_leaves_the_rows_offered_bound_room(bins_test, tmp_path):
    tris = mirt.scene_soup(41, 2000, 0.2)                               # query_helpers.scene_of("soup2000")
    path = str(tmp_path / "soup2000.f32")
    np.ascontiguousarray(tris, np.float32).tofile(path)
    r = subprocess.run([bins_test, path] + ["%.9g" % x for x in OBLIQUE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    m = re.search(r"n (\d+) B (\d+) every (\d+) every_share ([\d.]+) offered_share ([\d.]+)", r.stdout)
    n, B, every, every_share, offered = int(m.group(1)), int(m.group(2)), int(m.group(3)), float(m.group(4)), float(m.group(5))
    print(r.stdout)
    assert n == 2000 and B == 32
    assert offered < OFFERED_CAP / 2, "a ray is offered %.4f of the scene: no room under the GPU test's bound" % offered
    assert every <= n // 100, "%d triangles on the every-ray list" % every


def test_placed_scenes_are_filed_as_the_class_table_says(bins_test, tmp_path):
    """placement.ALONG_CLASS entry by entry, from the header alone: the tool's scene-file mode on the placed suite scenes -- a
    descriptor or none; the every-ray list within along_every_cap(n) or beyond it.  along_helpers.grid_of agrees about "no
    descriptor".  Prints the every-ray shares (README, DESIGN 5.1 quote them)."""
    import placement as pl
    from along_helpers import grid_of
    seen = set()
    for scene in pl.ALONG_CLASS:
        for pname, (T, s) in pl.PLACEMENTS.items():
            tris = pl.placed_scene(scene, pname)
            path = str(tmp_path / "placed.f32")
            np.ascontiguousarray(tris, np.float32).tofile(path)
            v = tris[:, :9].reshape(-1, 3)
            lo, hi = v.min(axis=0), v.max(axis=0)
            line = []
            for dname, d in pl.ALONG_DIRS.items():
                want = pl.along_class(scene, pname, dname)
                d = pl.place_dirs(d, s)
                r = subprocess.run([bins_test, path] + ["%.9g" % x for x in d], capture_output=True, text=True, timeout=120)
                what = "%s at %s along %s" % (scene, pname, dname)
                grid = grid_of(d, lo, hi, len(tris))
                if want == "no_grid":
                    assert r.returncode == 1 and r.stdout.strip() == "no descriptor", (what, r.stdout + r.stderr)
                    assert grid is None, what
                    line.append("none")
                else:
                    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (what, r.stdout + r.stderr)
                    m = re.search(r"n (\d+) B (\d+) every (\d+) every_share ([\d.]+) offered_share [\d.]+ every_cap (\d+) pad ([\d.]+)", r.stdout)
                    n, B, every, cap, pad = int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(5)), float(m.group(6))
                    assert n == len(tris) and cap == max(n // 8, 64) and B == pl.ALONG_BINS.get(scene, 32), (what, r.stdout)
                    assert (every > cap) == (want == "gave_up"), "%s: %d of %d on the every-ray list, cap %d, but %s" % (what, every, n, cap, want)
                    assert grid is not None and grid["B"] == B and abs(grid["pad"] - pad) <= 1e-6 + 1e-4 * pad, (what, grid, pad)
                    line.append("%.3f%s" % (float(m.group(4)), "!" if want == "gave_up" else ""))
                seen.add(want)
            print("%-17s %-18s every-ray share along %s: %s" % (scene, pname, ", ".join(pl.ALONG_DIRS), "  ".join(line)))
    assert seen == {"binned", "gave_up", "no_grid"}, seen
    # the unit control is binned everywhere, and a pure scaling moves nothing
    for scene, rows in pl.ALONG_CLASS.items():
        assert rows["unit"] == rows["origin_x1024"] == rows["origin_div1024"] == ("binned",) * len(pl.ALONG_DIRS), scene


@pytest.mark.parametrize("name,targets,d,every_ray", [("soup2000 @ far", range(24), OBLIQUE, 50), ("needles @ far", range(0, 150, 6), [-0.6, 1.0, 0.35], 149)])
def test_far_probe_scenes(oracle, bins_test, tmp_path, name, targets, d, every_ray):
    """What test_gpu_along.py::test_silhouette_probes asks of its "@ far" scenes, from the header and the oracle alone: how the scene
    is filed (the soup binned, the needles beyond along_every_cap), and starts that take cells and hit."""
    import silhouette
    from along_helpers import cell_of, grid_of, silhouette_starts
    from query_helpers import oracle_intersect
    d = np.asarray(d, np.float32)
    tris = silhouette.scene_of(oracle, name)[0]
    path = str(tmp_path / "far.f32")
    np.ascontiguousarray(tris, np.float32).tofile(path)
    r = subprocess.run([bins_test, path] + ["%.9g" % x for x in d], capture_output=True, text=True, timeout=120)
    m = re.search(r"n (\d+) B (\d+) every (\d+) every_share [\d.]+ offered_share [\d.]+ every_cap (\d+)", r.stdout)
    print(r.stdout)
    assert int(m.group(3)) == every_ray and (every_ray > int(m.group(4))) == (name == "needles @ far"), r.stdout
    v = tris[:, :9].reshape(-1, 3)
    grid = grid_of(d, v.min(axis=0), v.max(axis=0), len(tris))
    starts = silhouette_starts(tris, d, targets, grid)
    i, j = cell_of(grid, starts)
    assert 500 < len(starts) < 9000 and (i >= 0).mean() > 0.9 and len(np.unique(i * grid["B"] + j)) > 10
    assert 0.2 < (oracle_intersect(oracle, tris, mirt.make_rays(starts, d))["index"] >= 0).mean() < 1.0
    # the scene's extent over its size: an ulp of a start against the smallest delta
    assert np.abs(v).max() / (v.max(axis=0) - v.min(axis=0)).max() > 30


def test_symbols():
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    declared = set(re.findall(r"MIRT_API\s+[\w\s\*]+?\b(mirt_\w+)\s*\(", hdr))
    lib = mirt.load()
    for name in NAMES:
        assert name in declared and name in mirt.EXPORTS and hasattr(lib, name), name
    assert lib.mirt_abi_version() == 4                        # additions only
    for name in ("intersect_along", "intersect_along_device", "occluded_along", "occluded_along_device", "along_stats"):
        assert callable(getattr(mirt, name)), name


def test_argument_checks():
    """The arguments are looked at before the library's state: a malformed call is MIRT_ERR_INVALID_ARGUMENT with or without a
    device, and nothing is written; a well-formed one without mirt_init is told to call it."""
    mirt.shutdown()
    lib = mirt.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    d = np.array([0, 0, 1], np.float32)
    origins = np.zeros((4, 3), np.float32)
    hits = mirt.fresh_hits(4)
    raw = hits.tobytes()
    limits = np.ones(4, np.float32)
    out = np.full(4 + 64, 0xAA, np.uint8)
    for f in (lib.mirt_intersect_along, lib.mirt_intersect_along_device):
        assert f(p(d), p(origins), -1, p(hits)) == INVALID and b"origin count -1 is negative" in lib.mirt_last_error()
        assert f(p(d), None, 4, p(hits)) == INVALID and b"origin arrays must not be NULL" in lib.mirt_last_error()
        assert f(p(d), p(origins), 4, None) == INVALID
        assert f(None, p(origins), 4, p(hits)) == INVALID and b"dir must not be NULL" in lib.mirt_last_error()
        assert f(p(d), p(origins), 4, p(hits)) == NOT_INITIALISED and b"mirt_init" in lib.mirt_last_error()
    for f in (lib.mirt_occluded_along, lib.mirt_occluded_along_device):
        assert f(p(d), p(origins), -1, p(limits), p(out)) == INVALID and b"origin count -1 is negative" in lib.mirt_last_error()
        assert f(p(d), None, 4, p(limits), p(out)) == INVALID and f(p(d), p(origins), 4, p(limits), None) == INVALID
        assert f(None, p(origins), 4, None, p(out)) == INVALID and b"dir must not be NULL" in lib.mirt_last_error()
        assert f(p(d), p(origins), 4, None, p(out)) == NOT_INITIALISED and b"mirt_init" in lib.mirt_last_error()
    assert hits.tobytes() == raw and (out == 0xAA).all()
    st = mirt.QueryStats()
    assert lib.mirt_get_along_stats(C.byref(st)) == NOT_INITIALISED and lib.mirt_get_along_stats(None) == NOT_INITIALISED
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.intersect_along(d, origins)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.along_stats()


class _Recorder:
    """Stands in for the loaded library: keeps what a shim passes, read back through the pointers as the C side would."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _floats(ptr, n):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), (n,)).copy()


def test_shims_lay_out_their_arguments_as_the_c_side_reads_them(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(mirt, "load", lambda: rec)
    d = [0.25, -2.0, 1.5]                                               # a list, float64 -> three float32
    origins = np.arange(24, dtype=np.float64).reshape(4, 6)[:, :3]     # not contiguous, not float32
    want = origins.astype(np.float32).ravel()
    hits = mirt.intersect_along(d, origins)
    name, (pd, po, n, ph) = rec.calls[-1]
    assert name == "mirt_intersect_along" and n == 4 and hits.dtype == mirt.HIT_DTYPE and hits.itemsize == 20
    assert np.array_equal(_floats(pd, 3), np.array(d, np.float32)) and np.array_equal(_floats(po, 12), want)
    assert ph.value == hits.ctypes.data and (hits["index"] == -1).all() and (hits["distance"] == np.finfo(np.float32).max).all()
    given = mirt.fresh_hits(4)
    given["distance"] = [1.0, -1.0, np.inf, np.nan]
    back = mirt.intersect_along(d, origins, given)
    assert back is not given and back.tobytes() == given.tobytes()      # the caller's records travel as they are, in a copy
    out = np.full(4, 0xAA, np.uint8)
    got = mirt.occluded_along(d, origins, 2.5, out)
    name, (pd, po, n, pl, pout) = rec.calls[-1]
    assert name == "mirt_occluded_along" and n == 4 and got is out and pout.value == out.ctypes.data
    assert np.array_equal(_floats(pl, 4), np.full(4, 2.5, np.float32)) and np.array_equal(_floats(po, 12), want)
    mirt.occluded_along(d, origins)
    assert rec.calls[-1][1][3] is None                                  # no limits: NULL
    mirt.intersect_along_device(d, 1234, 4, 5678)
    name, (pd, po, n, ph) = rec.calls[-1]
    assert name == "mirt_intersect_along_device" and (po, n, ph) == (1234, 4, 5678) and np.array_equal(_floats(pd, 3), np.array(d, np.float32))
    mirt.occluded_along_device(d, 1234, 4, None, 5678)
    assert rec.calls[-1][0] == "mirt_occluded_along_device" and rec.calls[-1][1][1:] == (1234, 4, None, 5678)
    with pytest.raises(ValueError, match="4 origins but 3 hit records"):
        mirt.intersect_along(d, origins, mirt.fresh_hits(3))
    with pytest.raises(ValueError, match="4 origins but 5 limits"):
        mirt.occluded_along(d, origins, np.ones(5, np.float32))
    with pytest.raises(ValueError, match="4 origins but 3 output bytes"):
        mirt.occluded_along(d, origins, None, np.zeros(3, np.uint8))
    with pytest.raises(ValueError):
        mirt.intersect_along([1.0, 2.0], origins)                       # not a direction
