"""What the ray queries along several directions in one call (mirt_intersect_alongs*, mirt_occluded_alongs*) show without a GPU:
tests/cpp/alongs_plan_test.cpp -- the slots of a group, the pass ranges, the sort key's round trip, and that a group of three
directions files exactly the union of what the three single-direction grids file --, the symbols, the argument checks and their
order, and the layout the Python shims hand to the C side."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mirt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOT_INITIALISED = -3, -2
NAMES = ("mirt_intersect_alongs", "mirt_intersect_alongs_device", "mirt_occluded_alongs", "mirt_occluded_alongs_device")


@pytest.fixture(scope="module")
def plan_test(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("alongs") / "alongs_plan_test")
    # the headers are HIP source: the host side alone, with the library's floating-point contract
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-w",
                    os.path.join(ROOT, "tests", "cpp", "alongs_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def test_plan_header(plan_test):
    """Slots per group at B = 8 .. 256, the pass ranges of 1 .. 256 directions, the key's round trip over every slot, and the
    largest key of a full group within one sort pass."""
    r = subprocess.run([plan_test], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_slot_lists_equal_the_single_grids(plan_test, tmp_path):
    """A seeded soup of 300 triangles under the oblique direction, an axis and a face diagonal: the group's (slot, cell, shell,
    triangle) set is the union of the three single-direction sets."""
    tris = mirt.scene_soup(43, 300, 0.2)
    path = str(tmp_path / "soup300.f32")
    np.ascontiguousarray(tris, np.float32).tofile(path)
    r = subprocess.run([plan_test, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    m = re.search(r"n (\d+) B (\d+) pairs (\d+) \((\d+) (\d+) (\d+)\)", r.stdout)
    assert int(m.group(1)) == 300 and int(m.group(2)) == 16 and int(m.group(3)) == sum(int(m.group(k)) for k in (4, 5, 6)), r.stdout


def test_symbols():
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    declared = set(re.findall(r"MIRT_API\s+[\w\s\*]+?\b(mirt_\w+)\s*\(", hdr))
    lib = mirt.load()
    for name in NAMES:
        assert name in declared and name in mirt.EXPORTS and hasattr(lib, name), name
    assert lib.mirt_abi_version() == 4                        # additions only
    for name in ("intersect_alongs", "intersect_alongs_device", "occluded_alongs", "occluded_alongs_device", "along_stats"):
        assert callable(getattr(mirt, name)), name


def test_argument_checks():
    """The arguments are looked at before the library's state: a malformed call is MIRT_ERR_INVALID_ARGUMENT with or without a
    device, and nothing is written; a well-formed one without mirt_init is told to call it.  The host forms refuse an index outside
    the list before that too."""
    mirt.shutdown()
    lib = mirt.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    dirs = np.array([[0, 0, 1], [0, 1, 0]], np.float32)
    of = np.array([0, 1, 1, 0], np.int32)
    origins = np.zeros((4, 3), np.float32)
    hits = mirt.fresh_hits(4)
    raw = hits.tobytes()
    limits = np.ones(4, np.float32)
    out = np.full(4 + 64, 0xAA, np.uint8)
    err = lambda: lib.mirt_last_error()
    for f in (lib.mirt_intersect_alongs, lib.mirt_intersect_alongs_device):
        assert f(p(dirs), -1, p(of), p(origins), 4, p(hits)) == INVALID and b"direction count -1 is negative" in err()
        assert f(p(dirs), 2, p(of), p(origins), -1, p(hits)) == INVALID and b"origin count -1 is negative" in err()
        assert f(p(dirs), 2, p(of), None, 4, p(hits)) == INVALID and b"origin arrays must not be NULL" in err()
        assert f(p(dirs), 2, p(of), p(origins), 4, None) == INVALID
        assert f(None, 2, p(of), p(origins), 4, p(hits)) == INVALID and b"dirs must not be NULL" in err()
        assert f(None, 0, p(of), p(origins), 4, p(hits)) == INVALID and b"4 rays but no direction" in err()
        assert f(p(dirs), 2, None, p(origins), 4, p(hits)) == INVALID and b"dir_of may be NULL only for a single direction" in err()
        assert f(p(dirs), 2, p(of), p(origins), 4, p(hits)) == NOT_INITIALISED and b"mirt_init" in err()
        assert f(p(dirs), 1, None, p(origins), 4, p(hits)) == NOT_INITIALISED          # one direction: no indices needed
        assert f(p(dirs), 2, p(of), p(origins), 0, p(hits)) == NOT_INITIALISED
    for f in (lib.mirt_occluded_alongs, lib.mirt_occluded_alongs_device):
        assert f(p(dirs), -1, p(of), p(origins), 4, p(limits), p(out)) == INVALID and b"direction count -1 is negative" in err()
        assert f(p(dirs), 2, p(of), p(origins), -1, p(limits), p(out)) == INVALID
        assert f(p(dirs), 2, p(of), None, 4, p(limits), p(out)) == INVALID and f(p(dirs), 2, p(of), p(origins), 4, p(limits), None) == INVALID
        assert f(None, 2, p(of), p(origins), 4, None, p(out)) == INVALID and b"dirs must not be NULL" in err()
        assert f(p(dirs), 0, p(of), p(origins), 4, None, p(out)) == INVALID and b"no direction" in err()
        assert f(p(dirs), 2, None, p(origins), 4, None, p(out)) == INVALID and b"dir_of may be NULL only" in err()
        assert f(p(dirs), 2, p(of), p(origins), 4, None, p(out)) == NOT_INITIALISED and b"mirt_init" in err()
    # the host forms look at every index first
    for bad in (-1, 2, 2 ** 30):
        idx = of.copy()
        idx[2] = bad
        assert lib.mirt_intersect_alongs(p(dirs), 2, p(idx), p(origins), 4, p(hits)) == INVALID and b"dir_of[2] = %d is outside [0, 2)" % bad in err()
        assert lib.mirt_occluded_alongs(p(dirs), 2, p(idx), p(origins), 4, None, p(out)) == INVALID and b"dir_of[2]" in err()
        assert lib.mirt_intersect_alongs_device(p(dirs), 2, p(idx), p(origins), 4, p(hits)) == NOT_INITIALISED     # (cannot look)
    assert hits.tobytes() == raw and (out == 0xAA).all()
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.intersect_alongs(dirs, of, origins)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.occluded_alongs(dirs, of, origins)


class _Recorder:
    """Stands in for the loaded library: keeps what a shim passes, read back through the pointers as the C side would."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _array(ptr, n, ctype):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (n,)).copy()


def test_shims_lay_out_their_arguments_as_the_c_side_reads_them(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(mirt, "load", lambda: rec)
    dirs = [[0.25, -2.0, 1.5], [1.0, 0.0, 0.0], [0.0, 0.5, 0.5]]       # lists, float64 -> 3 x 3 float32
    want_dirs = np.array(dirs, np.float32).ravel()
    of = np.array([2, 0, 1, 2], np.int64)                              # not int32
    origins = np.arange(24, dtype=np.float64).reshape(4, 6)[:, :3]     # not contiguous, not float32
    want = origins.astype(np.float32).ravel()
    hits = mirt.intersect_alongs(dirs, of, origins)
    name, (pd, nd, pof, po, n, ph) = rec.calls[-1]
    assert name == "mirt_intersect_alongs" and (nd, n) == (3, 4) and hits.dtype == mirt.HIT_DTYPE and hits.itemsize == 20
    assert np.array_equal(_array(pd, 9, C.c_float), want_dirs) and np.array_equal(_array(po, 12, C.c_float), want)
    assert np.array_equal(_array(pof, 4, C.c_int32), of.astype(np.int32))
    assert ph.value == hits.ctypes.data and (hits["index"] == -1).all() and (hits["distance"] == np.finfo(np.float32).max).all()
    given = mirt.fresh_hits(4)
    given["distance"] = [1.0, -1.0, np.inf, np.nan]
    back = mirt.intersect_alongs(dirs, of, origins, given)
    assert back is not given and back.tobytes() == given.tobytes()      # the caller's records travel as they are, in a copy
    mirt.intersect_alongs(dirs[:1], None, origins)
    assert rec.calls[-1][1][1] == 1 and rec.calls[-1][1][2] is None      # one direction: NULL indices
    out = np.full(4, 0xAA, np.uint8)
    got = mirt.occluded_alongs(dirs, of, origins, 2.5, out)
    name, (pd, nd, pof, po, n, pl, pout) = rec.calls[-1]
    assert name == "mirt_occluded_alongs" and (nd, n) == (3, 4) and got is out and pout.value == out.ctypes.data
    assert np.array_equal(_array(pl, 4, C.c_float), np.full(4, 2.5, np.float32)) and np.array_equal(_array(po, 12, C.c_float), want)
    assert np.array_equal(_array(pd, 9, C.c_float), want_dirs) and np.array_equal(_array(pof, 4, C.c_int32), of.astype(np.int32))
    mirt.occluded_alongs(dirs, of, origins)
    assert rec.calls[-1][1][5] is None                                  # no limits: NULL
    mirt.intersect_alongs_device(dirs, 1111, 1234, 4, 5678)
    name, (pd, nd, pof, po, n, ph) = rec.calls[-1]
    assert name == "mirt_intersect_alongs_device" and (nd, pof, po, n, ph) == (3, 1111, 1234, 4, 5678) and np.array_equal(_array(pd, 9, C.c_float), want_dirs)
    mirt.occluded_alongs_device(dirs, None, 1234, 4, None, 5678)
    assert rec.calls[-1][0] == "mirt_occluded_alongs_device" and rec.calls[-1][1][1:] == (3, None, 1234, 4, None, 5678)
    with pytest.raises(ValueError, match="4 origins but 3 direction indices"):
        mirt.intersect_alongs(dirs, of[:3], origins)
    with pytest.raises(ValueError, match="4 origins but 3 hit records"):
        mirt.intersect_alongs(dirs, of, origins, mirt.fresh_hits(3))
    with pytest.raises(ValueError, match="4 origins but 5 limits"):
        mirt.occluded_alongs(dirs, of, origins, np.ones(5, np.float32))
    with pytest.raises(ValueError, match="4 origins but 3 output bytes"):
        mirt.occluded_alongs(dirs, of, origins, None, np.zeros(3, np.uint8))
    with pytest.raises(ValueError):
        mirt.intersect_alongs([1.0, 2.0], None, origins)                # not a list of directions
