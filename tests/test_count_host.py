"""What the hit counts (mirt_count_hits*, mirt_count_hits_along*, mirt_count_hits_alongs*) show without a GPU:
tests/cpp/count_rule_test.cpp -- the admission rule of count/count_rule.hpp and a model of the count walk along a direction against a
plain count, around the origin and in a far regime, with two planted faults (a reject that is not strict, a row offered twice) that
must be caught in each --; the six wrappers and their refusal without a device; every invalid-argument case; and that the
expectations used on the GPU (test_gpu_count_hits.py) reach the cases they are there for, on the oracle alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mirt
import count_helpers as K
from along_helpers import OBLIQUE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "count_rule_test.cpp")
INVALID = -3


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr, r.stdout + r.stderr
    pattern = (r"rays (\d+) calls (\d+) wrong (\d+) not_strict_caught (\d+) offered_twice_caught (\d+) deep (\d+) zero (\d+) near_at_threshold (\d+) "
               r"limit_cuts (\d+) rows (\d+) offered (\d+)")
    for regime in (r"^", r"^far: "):
        m = re.search(regime + pattern, r.stdout, re.M)
        rays, calls, wrong, strict, twice, deep, zero, at_thr, cuts, rows, offered = map(int, m.groups())
        assert wrong == 0 and rays >= 5000 and calls >= 100000
        assert strict > 1000 and twice > 1000, "a planted fault is not caught"
        assert deep > 1000 and zero > 1000 and at_thr > 1000 and cuts > 1000, "the inputs miss one of the cases they are there for"
        assert offered < rows, "no limit ever ended a list early"
    assert re.search(r"rule ok; the threshold without a limit -> shell 7 of 8, 0 with no shell width", r.stdout)
    return r.stdout


def test_the_walk_equals_a_plain_count(tmp_path):
    exe = str(tmp_path / "count_rule_test")
    # plain C++ with the library's floating-point contract; a stand-alone program under the address and undefined-behaviour sanitizers
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True, timeout=300)
    assert "shell_model:" in _run(exe)


def test_the_walk_on_the_librarys_own_shells(tmp_path):
    exe = str(tmp_path / "count_rule_test_lib")
    # bin_shell_of's header is HIP source: the host side alone, with the library's floating-point contract
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-DCOUNT_RULE_LIBRARY_SHELL",
                    SRC, "-o", exe], check=True, timeout=300)
    assert "bin_shell_of: model_differs 0;" in _run(exe)


def test_wrappers_and_refusal_without_a_device():
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    for name in K.NAMES:
        assert name in mirt.EXPORTS and re.search(r"MIRT_API int %s\(" % name, hdr), name
        assert callable(getattr(mirt, name[len("mirt_"):]))
    assert mirt.load().mirt_abi_version() == 4
    starts = np.zeros((3, 3), np.float32)
    rays = mirt.make_rays(starts, OBLIQUE)
    with pytest.raises(ValueError):
        mirt.count_hits(rays, after=mirt.fresh_hits(2))
    with pytest.raises(ValueError):
        mirt.count_hits_along(OBLIQUE, starts, max_distance=[1.0, 2.0])
    with pytest.raises(ValueError):
        mirt.count_hits_alongs([OBLIQUE, OBLIQUE], [0, 1], starts)
    import torch
    if not torch.cuda.is_available():
        p = C.c_void_p(64)                                          # (never dereferenced: the library refuses first)
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.count_hits(rays)
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.count_hits_device(p, 3, None, None, p)
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.count_hits_along(OBLIQUE, starts, max_distance=2.0)
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.count_hits_along_device(OBLIQUE, p, 3, None, p, p)
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.count_hits_alongs([OBLIQUE, -OBLIQUE], [0, 1, 1], starts, after=mirt.fresh_hits(3))
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.count_hits_alongs_device([OBLIQUE, -OBLIQUE], p, p, 3, C.c_void_p(4096), None, p)


def test_invalid_arguments_are_refused_without_a_device():
    """-3 and a text for every bad argument of the along forms, with or without mirt_init; the host form of several directions also
    refuses an index outside the list.  Nothing is written.  (mirt_count_hits* looks at the library's state first, as
    mirt_intersect_ordered* does: its cases run on the GPU, test_gpu_count_hits.py.)"""
    lib = mirt.load()
    cases, keep, snapshot = K.bad_calls()
    before = snapshot()
    assert len(cases) == 2 * 4 + 2 * 5 + 2 * 8
    cases = [c for c in cases if "along" in c[0]]
    for name, args, why in cases:
        assert getattr(lib, name)(*args) == INVALID, (name, why)
        assert lib.mirt_last_error(), (name, why)
    P = mirt._ptr
    rays, d, dirs, of, origins, counts, after = keep
    for bad in (-1, 2):
        idx = of.copy()
        idx[3] = bad
        assert lib.mirt_count_hits_alongs(P(dirs), 2, P(idx), P(origins), len(idx), None, None, P(counts)) == INVALID
        assert re.search(r"dir_of\[3\] = %d is outside \[0, 2\)" % bad, lib.mirt_last_error().decode())
    assert snapshot() == before, "a refused call wrote something"


# ---- the GPU expectations reach their cases, on the oracle alone ---------------------------------------------------------------------

def test_the_plates_are_deep_along_three_directions(oracle):
    """257 starts along each direction: at least 70 rays above 8 hits, 35 above 16, 25 with none, and the most hits 24 (about half of
    what was measured: 163 / 148 / 76, 141 / 71 / 57 and 161 / 113 / 63)."""
    for d in K.PLATE_DIRS:
        tris, starts, planted, rec = K.along_case(oracle, "plates", d, 257)
        c = K.expected(rec)
        print("plates along %r: above 8 %d, above 16 %d, none %d, most %d" % (d.tolist(), (c > 8).sum(), (c > 16).sum(), (c == 0).sum(), c.max()))
        assert (c > 8).sum() >= 70 and (c > 16).sum() >= 35 and (c == 0).sum() >= 25 and c.max() == 24, d
        assert planted.sum() >= 3


def test_the_plates_are_deep_for_the_sweep(oracle):
    """odd_rays(make_batch(257, 1.5, 1.0)): at least 60 rays above 8 hits and 25 above 16 (measured: 134 and 54)."""
    c = K.expected(K.table_of(oracle, "plates", K.rays_of("plates", 257)))
    print("plates, sweep rays: above 8 %d, above 16 %d, most %d" % ((c > 8).sum(), (c > 16).sum(), c.max()))
    assert (c > 8).sum() >= 60 and (c > 16).sum() >= 25


def test_the_existing_scenes_along_the_oblique_direction(oracle):
    """soup65x2: every count even, at least 35 rays with 2 or more hits (measured 76); soup2000, 1025 starts: at least 3 rays above 8
    hits and 190 with none (6 and 384); cornell: at least 50 rays with 2 or more hits (109)."""
    c = K.expected(K.along_case(oracle, "soup65x2", OBLIQUE, 257)[3])
    print("soup65x2: 2 or more hits %d, odd counts %d" % ((c >= 2).sum(), (c % 2).sum()))
    assert (c % 2 == 0).all() and (c >= 2).sum() >= 35
    c = K.expected(K.along_case(oracle, "soup2000", OBLIQUE, 1025)[3])
    print("soup2000: above 8 %d, none %d, most %d" % ((c > 8).sum(), (c == 0).sum(), c.max()))
    assert (c > 8).sum() >= 3 and (c == 0).sum() >= 190
    c = K.expected(K.along_case(oracle, "cornell", OBLIQUE, 257)[3])
    print("cornell: 2 or more hits %d" % (c >= 2).sum())
    assert (c >= 2).sum() >= 50
