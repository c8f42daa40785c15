"""What the ordered hits along parallel rays (mirt_intersect_ordered_along*, mirt_intersect_ordered_alongs*) show without a GPU:
tests/cpp/along_order_test.cpp -- the bound rule of order/along_order.hpp together with the list rule of order/hit_list.hpp against
a plain sort, around the origin and in a far regime (|rs| up to 2^12: distinct distances on one float threshold), with a planted fault
that must be caught in each, and what bin_shell_of returns for thresholds of +inf and FLT_MAX --; the four
wrappers and their refusal without a device; every invalid-argument case; and that the expectations used on the GPU
(test_gpu_ordered_along.py) meet their conditions on the oracle alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mirt
import ordered_along_helpers as A
from along_helpers import OBLIQUE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "along_order_test.cpp")
INVALID = -3
NAMES = A.NAMES
# along_order_test.cpp's far regime: rays with two distinct distances of one float sum rs + d, and with such a pair at a cut -- half of
# what the runs show (4832 and 4070 of 6000 rays in the lower of the two builds)
FAR_COLLISIONS_FLOOR, FAR_AT_CUT_FLOOR = 2400, 2000


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr, r.stdout + r.stderr
    m = re.search(r"rays (\d+) calls (\d+) wrong (\d+) planted_fault_caught (\d+) short_lists (\d+) ties_at_cut (\d+) near_at_sum (\d+) "
                  r"in_cell_and_on_list (\d+) rows (\d+) offered (\d+)", r.stdout)
    rays, calls, wrong, caught, short, ties, at_sum, both, rows, offered = map(int, m.groups())
    assert wrong == 0 and caught > 0 and rays >= 5000 and calls >= 50000
    assert short > 1000 and ties > 1000 and at_sum > 1000 and both > 1000, "the inputs miss one of the cases they are there for"
    assert offered < rows, "the bound never moved an end"
    # the far regime (|rs| up to 2^12, distances a few floats apart): right, the planted fault caught by it alone, and rays in which
    # two distinct distances share one float threshold -- at the K-th cut too -- above the program's floors; none around the origin
    m = re.search(r"far: rays (\d+) calls (\d+) wrong (\d+) planted_fault_caught (\d+) short_lists \d+ ties_at_cut (\d+) near_at_sum (\d+) collisions (\d+) "
                  r"collisions_at_cut (\d+) rows (\d+) offered (\d+) \(collisions around the origin: (\d+)\)", r.stdout)
    frays, fcalls, fwrong, fcaught, fties, fat_sum, collide, at_cut, frows, foffered, near_collide = map(int, m.groups())
    assert fwrong == 0 and fcaught > 0 and frays >= 5000 and fcalls >= 50000
    assert collide >= FAR_COLLISIONS_FLOOR and at_cut >= FAR_AT_CUT_FLOOR and near_collide == 0, "the far regime misses the case it is there for"
    assert fties > 1000 and fat_sum > 1000 and foffered < frows
    # +inf and FLT_MAX both fall into the last shell, and into shell 0 where the shells have no width
    assert re.search(r"\+inf -> 7, FLT_MAX -> 7, rs \+ FLT_MAX -> 7 of 8 shells; with no shell width \+inf -> 0 \(inf \* 0 is NaN\), FLT_MAX -> 0", r.stdout)
    return r.stdout


def test_the_walk_equals_a_plain_sort(tmp_path):
    exe = str(tmp_path / "along_order_test")
    # plain C++ with the library's floating-point contract; a stand-alone program under the address and undefined-behaviour sanitizers
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True, timeout=300)
    assert "shell_model:" in _run(exe)


def test_the_walk_on_the_librarys_own_shells(tmp_path):
    exe = str(tmp_path / "along_order_test_lib")
    # bin_shell_of's header is HIP source: the host side alone, with the library's floating-point contract
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-DALONG_ORDER_LIBRARY_SHELL",
                    SRC, "-o", exe], check=True, timeout=300)
    assert "bin_shell_of: model_differs 0;" in _run(exe)


def test_wrappers_and_refusal_without_a_device():
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    for name in NAMES:
        assert name in mirt.EXPORTS and re.search(r"MIRT_API int %s\(" % name, hdr), name
        assert callable(getattr(mirt, name[len("mirt_"):]))
    starts = np.zeros((3, 3), np.float32)
    with pytest.raises(ValueError):
        mirt.intersect_ordered_along(OBLIQUE, starts, 2, after=mirt.fresh_hits(2))
    with pytest.raises(ValueError):
        mirt.intersect_ordered_alongs([OBLIQUE, OBLIQUE], [0, 1], starts, 2)
    import torch
    if not torch.cuda.is_available():
        p = C.c_void_p(64)                                          # (never dereferenced: the library refuses first)
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.intersect_ordered_along(OBLIQUE, starts, 2)
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.intersect_ordered_along_device(OBLIQUE, p, 3, None, 2, p, p)
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.intersect_ordered_alongs([OBLIQUE, -OBLIQUE], [0, 1, 1], starts, 2)
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.intersect_ordered_alongs_device([OBLIQUE, -OBLIQUE], p, p, 3, None, 2, p, p)


def test_invalid_arguments_are_refused_without_a_device():
    """-3 and a text for every bad argument, with or without mirt_init; the host form of several directions also refuses an index
    outside the list.  Nothing is written."""
    lib = mirt.load()
    cases, keep, snapshot = A.bad_calls()
    before = snapshot()
    assert len(cases) == 2 * 10 + 2 * 13
    for name, args, why in cases:
        assert getattr(lib, name)(*args) == INVALID, (name, why)
        assert lib.mirt_last_error(), (name, why)
    P = mirt._ptr
    d, dirs, of, origins, hits, counts = keep
    for bad in (-1, 2):
        idx = of.copy()
        idx[3] = bad
        assert lib.mirt_intersect_ordered_alongs(P(dirs), 2, P(idx), P(origins), len(idx), None, 2, P(hits), P(counts)) == INVALID
        assert re.search(r"dir_of\[3\] = %d is outside \[0, 2\)" % bad, lib.mirt_last_error().decode())
    assert snapshot() == before, "a refused call wrote something"


def test_the_gpu_expectations_meet_their_conditions(oracle):
    """The floors of the issue's table on the oracle alone, on the first 257 starts along OBLIQUE; some soup2000 ray has more than
    8 hits."""
    for name in ("soup2000", "cornell", "soup65x2"):
        tris, starts, planted, back, want = A.case(oracle, name, OBLIQUE, 257, 8)
        c = want[1]
        print(name, "pulled back: >= 1 hit %.2f, >= 2 hits %.2f; as drawn: %.2f, %.2f" %
              ((c[back] >= 1).mean(), (c[back] >= 2).mean(), (c[~back] >= 1).mean(), (c[~back] >= 2).mean()))
        A.floors_hold(name, want, back, name)
    tris, starts, planted, back, _ = A.case(oracle, "soup2000", OBLIQUE, 257, 8)
    deep = A.O.peel(oracle, tris, mirt.make_rays(starts, OBLIQUE)[np.flatnonzero(A.case(oracle, "soup2000")[4][1] == 8)], 12)
    print("soup2000: the most hits of a ray:", int(deep[1].max()))
    assert deep[1].max() > 8, "no soup2000 ray has more than 8 hits"
    assert planted.sum() >= 3 and (planted & back).sum() == 0
