"""What mirt_intersect_fans* does without a GPU: the symbols, the loud failure without mirt_init -- the not-initialised status comes
before every argument check --, the Python wrappers' shape checks, and tests/cpp/fans_plan_test.cpp: the pass plan (which origin
ranges go to which cube, at which grid) as a pure function of the origin count and the scene's size."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mirt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_INITIALISED = -2


def test_pass_plan_tiles_the_origins_within_a_cubes_limits(tmp_path):
    exe = str(tmp_path / "fans_plan_test")
    # the headers are HIP source: the host side alone; a stand-alone program under the address and undefined-behaviour sanitizers
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "fans_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_symbols():
    lib = mirt.load()
    for name in ("mirt_intersect_fans", "mirt_intersect_fans_device"):
        assert hasattr(lib, name) and name in mirt.EXPORTS, name
    assert lib.mirt_abi_version() == 4                        # additions only


def test_calls_need_mirt_init():
    """Without mirt_init -- and so without a device -- both forms refuse, whatever their arguments: the status comes first."""
    mirt.shutdown()
    lib = mirt.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    origins = np.zeros((2, 3), np.float32)
    of = np.array([0, 1, 1, 0], np.int32)
    dirs, hits = np.ones((4, 3), np.float32), mirt.fresh_hits(4)
    before = hits.tobytes()
    for f in (lib.mirt_intersect_fans, lib.mirt_intersect_fans_device):
        assert f(p(origins), 2, p(of), p(dirs), 4, p(hits)) == NOT_INITIALISED
        assert b"mirt_init" in lib.mirt_last_error()
        # arguments that are invalid one by one: still the not-initialised status
        assert f(p(origins), -1, p(of), p(dirs), 4, p(hits)) == NOT_INITIALISED
        assert f(p(origins), 2, p(of), p(dirs), -1, p(hits)) == NOT_INITIALISED
        assert f(None, 2, p(of), p(dirs), 4, p(hits)) == NOT_INITIALISED
        assert f(p(origins), 2, None, p(dirs), 4, p(hits)) == NOT_INITIALISED
        assert f(p(origins), 0, p(of), p(dirs), 4, p(hits)) == NOT_INITIALISED
        assert f(p(origins), 2, p(of), None, 4, None) == NOT_INITIALISED
        assert f(None, 0, None, None, 0, None) == NOT_INITIALISED
    bad = of.copy()
    bad[2] = 2
    assert lib.mirt_intersect_fans(p(origins), 2, p(bad), p(dirs), 4, p(hits)) == NOT_INITIALISED
    assert hits.tobytes() == before
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.intersect_fans(origins, of, dirs)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.intersect_fans_device(origins, None, None, 0, None)


def test_wrappers_reject_mismatched_shapes():
    origins = np.zeros((2, 3), np.float32)
    dirs = np.ones((4, 3), np.float32)
    with pytest.raises(ValueError, match="hit records"):
        mirt.intersect_fans(origins, np.zeros(4, np.int32), dirs, mirt.fresh_hits(3))
    with pytest.raises(ValueError, match="origin indices"):
        mirt.intersect_fans(origins, np.zeros(5, np.int32), dirs)
    with pytest.raises(ValueError):
        mirt.intersect_fans(np.zeros(7, np.float32), np.zeros(4, np.int32), dirs)         # not a list of 3-vectors
    with pytest.raises(ValueError):
        mirt.intersect_fans(origins, np.zeros(4, np.int32), np.ones((4, 2), np.float32))
