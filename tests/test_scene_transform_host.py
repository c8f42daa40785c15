"""mirt_transform on the CPU -- the arithmetic mirt_scene_transform runs on the device (scene/scene_xform.hpp), on a host array --
and the part of the device-resident scene calls that needs no GPU: the symbols and the loud failure without mirt_init.

All bit comparisons are on uint32 views."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mirt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cpp-raytracer-rasterizer_amd")
F = np.float32
IDENTITY = np.eye(3, dtype=np.float32).ravel()
NEW_SYMBOLS = ("mirt_scene_upload_device", "mirt_scene_update_device", "mirt_scene_update", "mirt_scene_transform",
               "mirt_transform", "mirt_scene_download", "mirt_scene_info")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def restated(tris, rot9, tr):
    """mirt_transform in numpy float32, operation for operation: per vertex and row r of the column-major matrix the products
    m[r] x, m[3 + r] y, m[6 + r] z summed left to right, then the translation; the normal cross(v2 - v0, v1 - v0) times
    1 / sqrt(dot) with glm's (x + y) + z; the colour as it is.  (Every array below is float32, so every operation rounds once.)"""
    t = np.array(tris, F).reshape(-1, 15)
    m, tr = np.asarray(rot9, F), np.asarray(tr, F)
    out = t.copy()
    for v in range(3):
        x, y, z = t[:, 3 * v], t[:, 3 * v + 1], t[:, 3 * v + 2]
        for r in range(3):
            out[:, 3 * v + r] = ((m[r] * x + m[3 + r] * y) + m[6 + r] * z) + tr[r]
    v0, v1, v2 = out[:, 0:3], out[:, 3:6], out[:, 6:9]
    a, b = v2 - v0, v1 - v0                                   # glm::cross(a, b)
    cx = a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2]
    cy = a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0]
    cz = a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F(1.0) / np.sqrt((cx * cx + cy * cy) + cz * cz)
        out[:, 9], out[:, 10], out[:, 11] = cx * inv, cy * inv, cz * inv
    assert out.dtype == F and inv.dtype == F
    return out


@pytest.mark.parametrize("scene", ["cornell", "soup"])
def test_identity_is_a_fixed_point(scene):
    """Both scenes were last touched by ComputeNormal (and are pinned to the oracle by test_host_scene_functions_match_oracle): the
    identity moves no vertex, and the recomputed normal is the one they hold."""
    tris = mirt.scene_cornell() if scene == "cornell" else mirt.scene_soup(1, 2000, 0.05)
    moved = mirt.transform(tris, IDENTITY, (0.0, 0.0, 0.0))
    assert moved is not tris and np.array_equal(bits(moved), bits(tris))


def test_yaw_and_translation_equal_the_restatement():
    tris = mirt.scene_soup(3, 777, 0.2)
    rot, tr = mirt.rot_from_yaw(0.7, 1.01), (0.25, -0.5, 1.0)
    got, want = mirt.transform(tris, rot, tr), restated(tris, rot, tr)
    assert not np.array_equal(bits(got[:, :12]), bits(tris[:, :12]))
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
    assert np.array_equal(bits(got[:, 12:]), bits(tris[:, 12:]))             # the colour is untouched
    # ... and a second transform compounds on the first
    got2, want2 = mirt.transform(got, rot, tr), restated(want, rot, tr)
    assert np.array_equal(bits(got2), bits(want2))


def test_degenerate_triangle_gets_nan_normals():
    tris = mirt.scene_soup(5, 9, 0.2)
    tris[4, 3:6] = tris[4, 0:3]                                # v1 == v0: cross = 0, 0 * (1 / sqrt(0)) = NaN
    rot, tr = mirt.rot_from_yaw(0.7, 1.01), (0.25, -0.5, 1.0)
    got, want = mirt.transform(tris, rot, tr), restated(tris, rot, tr)
    assert np.isnan(got[4, 9:12]).all() and np.isnan(want[4, 9:12]).all()
    keep = np.ones(got.shape, bool)
    keep[4, 9:12] = False
    assert np.array_equal(bits(got)[keep], bits(want)[keep]) and not np.isnan(got[keep]).any()


def test_stand_alone_program_on_ranges_at_both_ends(tmp_path):
    exe = str(tmp_path / "scene_transform_test")
    # scene_host.cpp is HIP source (mirt_math.hpp): the host side alone, with the library's floating-point contract; a stand-alone
    # program under the address and undefined-behaviour sanitizers
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "scene_transform_test.cpp"), os.path.join(PKG, "csrc", "scene_host.cpp"),
                    "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_symbols():
    lib = mirt.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in mirt.EXPORTS, name
    assert lib.mirt_abi_version() == 4                        # additions only
    assert C.sizeof(mirt.SceneInfo) == 40


def test_host_arithmetic_needs_no_device():
    mirt.shutdown()
    one = np.zeros((1, 15), F)
    lib = mirt.load()
    assert lib.mirt_transform(one.ctypes.data_as(C.c_void_p), 1, IDENTITY.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p)) == 0
    assert lib.mirt_transform(None, 1, IDENTITY.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p)) == -3
    assert lib.mirt_transform(None, 0, IDENTITY.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p)) == 0


def test_device_calls_need_mirt_init():
    mirt.shutdown()
    tris = mirt.scene_cornell()
    calls = [lambda: mirt.scene_upload_device(None, 30), lambda: mirt.scene_update_device(0, 1, None),
             lambda: mirt.scene_update(0, tris[:1]), lambda: mirt.scene_transform(0, 1, IDENTITY),
             lambda: mirt.scene_download(0, 1), lambda: mirt.scene_info()]
    for call in calls:
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            call()
    lib = mirt.load()
    p = tris.ctypes.data_as(C.c_void_p)
    r = IDENTITY.ctypes.data_as(C.c_void_p)
    # the not-initialised status comes first, whatever else is wrong with the arguments
    assert lib.mirt_scene_upload_device(None, None, -1) == -2 and lib.mirt_scene_upload_device(p, None, 30) == -2
    assert lib.mirt_scene_update_device(-1, -1, None) == -2 and lib.mirt_scene_update_device(0, 1, p) == -2
    assert lib.mirt_scene_update(-1, 5, None) == -2 and lib.mirt_scene_update(0, 1, p) == -2
    assert lib.mirt_scene_transform(-1, 1, None, None) == -2 and lib.mirt_scene_transform(0, 1, r, r) == -2
    assert lib.mirt_scene_download(0, -1, None) == -2 and lib.mirt_scene_download(0, 1, p) == -2
    assert lib.mirt_scene_info(None) == -2 and lib.mirt_scene_info(C.byref(mirt.SceneInfo())) == -2
    assert b"mirt_init" in lib.mirt_last_error()
