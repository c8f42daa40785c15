"""tests/cpp/fan_dir_test.cpp on the CPU: fan_dir_of (query/rt_query.hpp), the power-of-two scaling k_query_fan_binned picks its
cube bin from, returns exactly dir * 2^k with the largest component in [0.5, 1) inside its window and "not formed" outside it;
and the part of mirt_intersect_from* that needs no GPU: the symbols and the loud failure without mirt_init."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mirt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scaling_is_exact_inside_the_window_and_refused_outside(tmp_path):
    exe = str(tmp_path / "fan_dir_test")
    # the header is HIP source: the host side alone, with the library's floating-point contract; a stand-alone program under the
    # address and undefined-behaviour sanitizers
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "fan_dir_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_symbols():
    lib = mirt.load()
    for name in ("mirt_intersect_from", "mirt_intersect_from_device", "mirt_get_fan_stats"):
        assert hasattr(lib, name) and name in mirt.EXPORTS, name
    assert lib.mirt_abi_version() == 4                        # additions only


def test_calls_need_mirt_init():
    mirt.shutdown()
    dirs = np.array([[0, 0, 1], [1, 0, 0]], np.float32)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.intersect_from((0, 0, 0), dirs)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.intersect_from_device((0, 0, 0), None, 0, None)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.fan_stats()
    lib = mirt.load()
    s = mirt.QueryStats()
    assert lib.mirt_get_fan_stats(C.byref(s)) == -2 and lib.mirt_get_fan_stats(None) == -2     # the not-initialised status comes first
    assert lib.mirt_intersect_from(None, None, 4, None) == -2
    assert b"mirt_init" in lib.mirt_last_error()
