"""The bucket sort (csrc/bin_bucket_sort.hip: k_bs_scatter, k_bs_local) and the device-wide exclusive scan (csrc/scan.hpp) called
directly, against a host counting sort and a host prefix sum (tools/sortcheck.hip, built by __graft_entry__.build() from the library's
own kernel sources): every shift from 4 to 12 on both sides of each change-over, the scatter's chunk edges, the register and the looped
path of k_bs_local, more than 1024 buckets, grids sized from a wrong guess, an overflowed list -- and, beyond the sorted list itself,
what a frame never looks at: counters left zero, bin_off[nbins], count_out, nothing written past the used part of any array; the scan
on both sides of 1024 and of 1024 x 1024 items.  All integers, compared for equality."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bucket_sort_and_scan_equal_a_host_sort():
    exe = os.path.join(ROOT, "tools", "sortcheck")
    assert os.path.exists(exe), "tools/sortcheck not built (python -c 'import __graft_entry__ as g; g.build()')"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    if r.returncode != 0 or "MISMATCH" in out:           # the case lines that name the shape, then the end of the run
        out = "\n".join([ln for ln in out.splitlines() if "MISMATCH" in ln or "not as the sort" in ln][:60] + out.splitlines()[-12:])
    assert r.returncode == 0, out
    assert re.search(r"^sort: [1-9]\d* cases, 0 mismatching$", r.stdout, re.M), out
    assert re.search(r"^scan: [1-9]\d* cases, 0 mismatching$", r.stdout, re.M), out
