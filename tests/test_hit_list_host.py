"""What the ordered hits (mirt_intersect_ordered*) show without a GPU: tests/cpp/hit_list_test.cpp -- the list rule of
order/hit_list.hpp (the key, the `after` predicate, hit_list_offer) against a plain sort over seeded offer sequences, with a planted
fault that must be caught --, the header's constant and the Python shim's, and the calls' refusal without a device."""
import os
import re
import subprocess

import numpy as np
import pytest

import mirt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_list_equals_a_plain_sort(tmp_path):
    exe = str(tmp_path / "hit_list_test")
    # plain C++ with the library's floating-point contract; a stand-alone program under the address and undefined-behaviour sanitizers
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "hit_list_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "runtime error" not in r.stderr, r.stdout + r.stderr
    m = re.search(r"sequences (\d+) offers (\d+) full_lists (\d+) wrong (\d+) planted_fault_caught (\d+)", r.stdout)
    sequences, offers, full, wrong, caught = map(int, m.groups())
    assert wrong == 0 and caught > 0 and sequences >= 10000 and offers > 100000 and full > 1000


def test_constant_and_refusal_without_a_device():
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    assert int(re.search(r"#define MIRT_MAX_ORDERED_HITS (\d+)", hdr).group(1)) == mirt.MAX_ORDERED_HITS == 8
    assert "mirt_intersect_ordered" in mirt.EXPORTS and "mirt_intersect_ordered_device" in mirt.EXPORTS
    with pytest.raises(ValueError):
        mirt.intersect_ordered(mirt.make_rays(np.zeros((3, 3)), np.ones((3, 3))), 2, after=mirt.fresh_hits(2))
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(mirt.MirtError, match="mirt_init"):
            mirt.intersect_ordered(mirt.make_rays(np.zeros((3, 3)), np.ones((3, 3))), 2)
