"""What the occlusion queries (mirt_occluded*, mirt_occluded_fans*, mirt_get_occlusion_stats) do without a GPU: the symbols, the
loud failure without mirt_init -- the not-initialised status comes before every argument check and nothing is written --, and the
Python wrappers' checks of lengths and of the origin indices."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mirt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_INITIALISED = -2
NAMES = ("mirt_occluded", "mirt_occluded_device", "mirt_occluded_fans", "mirt_occluded_fans_device", "mirt_get_occlusion_stats")


def test_symbols():
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    declared = set(re.findall(r"MIRT_API\s+[\w\s\*]+?\b(mirt_\w+)\s*\(", hdr))
    lib = mirt.load()
    for name in NAMES:
        assert name in declared and name in mirt.EXPORTS and hasattr(lib, name), name
    assert lib.mirt_abi_version() == 4                        # additions only
    for name in ("occluded", "occluded_device", "occluded_fans", "occluded_fans_device", "occlusion_stats"):
        assert callable(getattr(mirt, name)), name


def test_calls_need_mirt_init():
    """Without mirt_init -- and so without a device -- every entry point refuses, whatever its arguments, and writes nothing."""
    mirt.shutdown()
    lib = mirt.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rays = mirt.make_rays(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32))
    limits = np.ones(4, np.float32)
    origins = np.zeros((2, 3), np.float32)
    of = np.array([0, 1, 1, 0], np.int32)
    dirs = np.ones((4, 3), np.float32)
    out = np.full(4 + 64, 0xAA, np.uint8)
    for f in (lib.mirt_occluded, lib.mirt_occluded_device):
        for args in ((p(rays), 4, p(limits), p(out)), (p(rays), 4, None, p(out)), (p(rays), -1, p(limits), p(out)),
                     (None, 4, p(limits), p(out)), (p(rays), 4, p(limits), None), (None, 0, None, None)):
            assert f(*args) == NOT_INITIALISED, args
            assert b"mirt_init" in lib.mirt_last_error()
    for f in (lib.mirt_occluded_fans, lib.mirt_occluded_fans_device):
        for args in ((p(origins), 2, p(of), p(dirs), 4, p(limits), p(out)), (p(origins), 2, p(of), p(dirs), 4, None, p(out)),
                     (p(origins), -1, p(of), p(dirs), 4, p(limits), p(out)), (p(origins), 2, p(of), p(dirs), -1, p(limits), p(out)),
                     (None, 2, p(of), p(dirs), 4, p(limits), p(out)), (p(origins), 2, None, p(dirs), 4, p(limits), p(out)),
                     (p(origins), 0, p(of), p(dirs), 4, p(limits), p(out)), (p(origins), 2, p(of), None, 4, p(limits), None),
                     (None, 0, None, None, 0, None, None)):
            assert f(*args) == NOT_INITIALISED, args
            assert b"mirt_init" in lib.mirt_last_error()
    bad = of.copy()
    bad[2] = 2
    assert lib.mirt_occluded_fans(p(origins), 2, p(bad), p(dirs), 4, p(limits), p(out)) == NOT_INITIALISED
    st = mirt.QueryStats()
    raw = bytes(st)
    assert lib.mirt_get_occlusion_stats(C.byref(st)) == NOT_INITIALISED and b"mirt_init" in lib.mirt_last_error()
    assert lib.mirt_get_occlusion_stats(None) == NOT_INITIALISED
    assert bytes(st) == raw
    assert (out == 0xAA).all()
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.occluded(rays, limits)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.occluded_device(None, 0, None, None)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.occluded_fans(origins, of, dirs)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.occluded_fans_device(origins, None, None, 0, None, None)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.occlusion_stats()


def test_wrappers_reject_mismatched_lengths():
    rays = mirt.make_rays(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32))
    with pytest.raises(ValueError, match="4 rays but 3 limits"):
        mirt.occluded(rays, np.ones(3, np.float32))
    with pytest.raises(ValueError, match="4 rays but 5 output bytes"):
        mirt.occluded(rays, None, np.zeros(5, np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        mirt.occluded(rays, None, np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="uint8"):
        mirt.occluded(rays, None, np.zeros(8, np.uint8)[::2])
    with pytest.raises(ValueError):
        mirt.occluded(np.zeros((4, 5), np.float32))                       # not rays
    origins = np.zeros((2, 3), np.float32)
    dirs = np.ones((4, 3), np.float32)
    of = np.array([0, 1, 1, 0], np.int32)
    with pytest.raises(ValueError, match="4 directions but 5 limits"):
        mirt.occluded_fans(origins, of, dirs, np.ones(5, np.float32))
    with pytest.raises(ValueError, match="4 directions but 3 output bytes"):
        mirt.occluded_fans(origins, of, dirs, None, np.zeros(3, np.uint8))
    with pytest.raises(ValueError, match="origin indices"):
        mirt.occluded_fans(origins, np.zeros(5, np.int32), dirs)
    with pytest.raises(ValueError):
        mirt.occluded_fans(np.zeros(7, np.float32), of, dirs)             # not a list of 3-vectors
    with pytest.raises(ValueError):
        mirt.occluded_fans(origins, of, np.ones((4, 2), np.float32))


def test_fans_wrapper_checks_the_origin_indices():
    """The host wrapper looks at every index before it calls the library: the caller's output array keeps its bytes."""
    origins = np.zeros((2, 3), np.float32)
    dirs = np.ones((4, 3), np.float32)
    out = np.full(4, 0xAA, np.uint8)
    for i, v in ((0, -1), (3, 2), (2, 2 ** 30), (1, -2 ** 31)):
        of = np.array([0, 1, 1, 0], np.int32)
        of[i] = v
        with pytest.raises(ValueError, match=r"origin_of\[%d\] = %d is outside \[0, 2\)" % (i, v)):
            mirt.occluded_fans(origins, of, dirs, None, out)
    assert (out == 0xAA).all()
