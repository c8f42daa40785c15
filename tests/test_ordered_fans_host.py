"""What the ordered hits from shared origins (mirt_intersect_ordered_from*, mirt_intersect_ordered_fans*) show without a GPU:
tests/cpp/fan_order_test.cpp -- the bound rule of order/fan_order.hpp together with the list rule of order/hit_list.hpp against a
plain sort, rows laid out as a cube bin lays them out, with a planted fault that must be caught, and what bin_shell_of returns for
bounds of +inf and FLT_MAX, with a shell width and without --; the four wrappers and their refusal without a device; every
invalid-argument case; and that the expectations used on the GPU (test_gpu_ordered_fans.py) meet the floors of their table on the
oracle alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mirt
import ordered_fans_helpers as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "fan_order_test.cpp")
INVALID = -3
NAMES = F.NAMES


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr, r.stdout + r.stderr
    m = re.search(r"rays (\d+) calls (\d+) wrong (\d+) planted_fault_caught (\d+) short_lists (\d+) ties_at_cut (\d+) near_at_dist (\d+) "
                  r"offered_twice (\d+) no_width (\d+) no_width_wrong (\d+) rows (\d+) offered (\d+)", r.stdout)
    rays, calls, wrong, caught, short, ties, at_dist, twice, flat, flat_wrong, rows, offered = map(int, m.groups())
    assert wrong == 0 and flat_wrong == 0 and caught > 0 and rays >= 5000 and calls >= 50000
    assert short > 1000 and ties > 1000 and at_dist > 1000 and twice > 1000 and flat > 100, "the inputs miss one of the cases they are there for"
    assert offered < rows, "the bound never moved an end"
    # +inf and FLT_MAX both fall into the last shell, into shell 0 where the shells have no width, and there is one shell only
    assert re.search(r"\+inf -> 15, FLT_MAX -> 15 of 16 shells, FLT_MAX -> 0 of 1 shell; with no shell width \+inf -> 0 \(inf \* 0 is NaN\), FLT_MAX -> 0", r.stdout)
    return r.stdout


def test_the_walk_equals_a_plain_sort(tmp_path):
    exe = str(tmp_path / "fan_order_test")
    # plain C++ with the library's floating-point contract; a stand-alone program under the address and undefined-behaviour sanitizers
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True, timeout=300)
    assert "shell_model:" in _run(exe)


def test_the_walk_on_the_librarys_own_shells(tmp_path):
    exe = str(tmp_path / "fan_order_test_lib")
    # bin_shell_of's header is HIP source: the host side alone, with the library's floating-point contract
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-DFAN_ORDER_LIBRARY_SHELL",
                    SRC, "-o", exe], check=True, timeout=300)
    assert "bin_shell_of: model_differs 0;" in _run(exe)


def test_wrappers_and_refusal_without_a_device():
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    for name in NAMES:
        assert name in mirt.EXPORTS and re.search(r"MIRT_API int %s\(" % name, hdr), name
        assert callable(getattr(mirt, name[len("mirt_"):]))
    dirs = np.ones((3, 3), np.float32)
    with pytest.raises(ValueError):
        mirt.intersect_ordered_from([0, 0, 0], dirs, 2, after=mirt.fresh_hits(2))
    with pytest.raises(ValueError):
        mirt.intersect_ordered_fans([[0, 0, 0], [1, 0, 0]], [0, 1], dirs, 2)
    import torch
    if not torch.cuda.is_available():
        p = C.c_void_p(64)                                          # (never dereferenced: the library refuses first)
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.intersect_ordered_from([0, 0, 0], dirs, 2)
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.intersect_ordered_from_device([0, 0, 0], p, 3, None, 2, p, p)
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.intersect_ordered_fans([[0, 0, 0], [1, 0, 0]], [0, 1, 1], dirs, 2)
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.intersect_ordered_fans_device([[0, 0, 0], [1, 0, 0]], p, p, 3, None, 2, p, p)


def test_invalid_arguments_are_refused_without_a_device():
    """-3 and a text for every bad argument, with or without mirt_init: the arguments are checked first, then the library's state.  The
    host form of several origins also refuses an index outside the list.  Nothing is written."""
    lib = mirt.load()
    cases, keep, snapshot = F.bad_calls()
    before = snapshot()
    assert len(cases) == 2 * 10 + 2 * 13
    for name, args, why in cases:
        assert getattr(lib, name)(*args) == INVALID, (name, why)
        assert lib.mirt_last_error(), (name, why)
    P = mirt._ptr
    origin, origins, of, dirs, hits, counts = keep
    for bad in (-1, 2):
        idx = of.copy()
        idx[3] = bad
        assert lib.mirt_intersect_ordered_fans(P(origins), 2, P(idx), P(dirs), len(idx), None, 2, P(hits), P(counts)) == INVALID
        assert re.search(r"origin_of\[3\] = %d is outside \[0, 2\)" % bad, lib.mirt_last_error().decode())
    assert snapshot() == before, "a refused call wrote something"


def test_the_gpu_expectations_meet_their_floors(oracle):
    """The floors of the issue's table hold on the oracle alone, for exactly the batches the GPU tests use."""
    for key in F.FLOORS:
        want = F.case(oracle, *key)[5]
        share, deep, tie = F.floors_hold(key, want)
        print(key, "shares of rays with >= 1, 2, 4, 8 hits: %.3f %.3f %.3f %.3f; rays with more than 8 hits: %d; tie pair in slots 0 / 1: %.3f"
              % (tuple(share) + (deep, tie)))
    tris, origins, of, dirs, rays, want = F.case(oracle, "soup2000", 33, 6534)
    assert len(dirs) == 6534 and len(np.unique(of)) == 33
    # soup65x2: every hit has a partner at the same distance, the later index first
    h, c = F.case(oracle, "soup65x2", 5, 1025)[5]
    hit = c >= 2
    assert (c[c > 0] >= 2).all() and (h["distance"][hit, 0] == h["distance"][hit, 1]).all() and (h["index"][hit, 0] == h["index"][hit, 1] + 65).all()
