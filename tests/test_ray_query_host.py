"""Ray queries (mirt_intersect*, mirt_direct_light*), the part that needs no GPU: the layouts of mirt_ray / mirt_hit, the four
symbols, the loud failure without mirt_init, and the argument checks of the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mirt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY_SYMBOLS = ("mirt_intersect", "mirt_intersect_device", "mirt_direct_light", "mirt_direct_light_device")
FLT_MAX = np.finfo(np.float32).max


def test_ray_and_hit_layouts():
    assert C.sizeof(mirt.Ray) == 24
    assert C.sizeof(mirt.Hit) == 20                      # sizeof(struct Intersection), raytracer.cpp:91-96
    assert mirt.RAY_DTYPE.itemsize == 24 and mirt.HIT_DTYPE.itemsize == 20
    # the numpy layouts are the ctypes ones, field by field
    for ct, dt in ((mirt.Ray, mirt.RAY_DTYPE), (mirt.Hit, mirt.HIT_DTYPE)):
        for name, _ in ct._fields_:
            assert getattr(ct, name).offset == dt.fields[name][1], name
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    assert re.search(r"typedef struct mirt_ray \{ float start\[3\]; float dir\[3\]; \} mirt_ray;", hdr)
    assert re.search(r"typedef struct mirt_hit \{ float position\[3\]; float distance; int32_t index; \} mirt_hit;", hdr)
    assert "#define MIRT_ABI_VERSION 4" in hdr


def test_query_symbols_load():
    lib = mirt.load()
    for name in QUERY_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in mirt.EXPORTS
    assert lib.mirt_abi_version() == 4


def test_fresh_hits_are_the_update_reset():
    h = mirt.fresh_hits(5)
    assert h.dtype == mirt.HIT_DTYPE and len(h) == 5
    assert np.all(h["distance"] == FLT_MAX) and np.all(h["index"] == -1) and not h["position"].any()
    r = mirt.make_rays((1, 2, 3), [(0, 0, 1), (0, 1, 0)])
    assert r.dtype == mirt.RAY_DTYPE and len(r) == 2
    assert np.array_equal(r.view(np.float32).reshape(2, 6), np.array([[1, 2, 3, 0, 0, 1], [1, 2, 3, 0, 1, 0]], np.float32))


def test_calls_need_mirt_init():
    """Without mirt_init every query entry point fails with the message every other compute call gives: no CPU path."""
    mirt.shutdown()
    rays, hits = mirt.make_rays((0, 0, -2), [(0, 0, 1)] * 3), mirt.fresh_hits(3)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.intersect(rays)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.intersect(rays, hits)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.intersect_device(None, 0, None)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.direct_light(hits, mirt.DEFAULT_LIGHT)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.direct_light_device(None, 0, mirt.DEFAULT_LIGHT, None)
    # ... and straight through the C-ABI, with the status code
    lib = mirt.load()
    out = np.zeros((3, 3), np.float32)
    assert lib.mirt_intersect(rays.ctypes.data, 3, hits.ctypes.data) == -2
    assert lib.mirt_intersect_device(None, -1, None) == -2
    assert lib.mirt_direct_light(hits.ctypes.data, 3, None, 0, out.ctypes.data) == -2
    assert lib.mirt_direct_light_device(None, 0, None, 0, None) == -2
    assert b"mirt_init" in lib.mirt_last_error()
    assert np.all(hits["index"] == -1) and np.all(hits["distance"] == FLT_MAX)     # nothing was touched


def test_binding_argument_validation():
    with pytest.raises(ValueError, match="3 rays but 2 hit records"):
        mirt.intersect(mirt.make_rays((0, 0, 0), [(0, 0, 1)] * 3), mirt.fresh_hits(2))
    with pytest.raises(ValueError):
        mirt.intersect(np.zeros((4, 5), np.float32))          # not n x 6 floats
    # (n, 6) floats are taken as rays as they are
    assert mirt._as_rays(np.arange(12, dtype=np.float32).reshape(2, 6))["dir"].tolist() == [[3, 4, 5], [9, 10, 11]]
