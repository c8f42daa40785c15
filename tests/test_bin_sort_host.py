"""tools/sortcheck.hip --selftest on the CPU: the checks that judge the bucket sort (csrc/bin_bucket_sort.hip) and the device scan
(csrc/scan.hpp) on the GPU -- verify_sort, verify_scan -- must report every corruption they are there for (entries swapped across a
bin border, a duplicated entry, inclusive offsets, a missing bin_off[nbins], a counter left non-zero, a stale count_out, a changed guard
word in each array, a wrong carry at a 1024 boundary of the scan, ...) and pass the outputs a host counting sort builds; and
bucket_sort_shift / bucket_sort_buckets keep 4 <= shift <= 12, buckets << shift >= nbins + 1 and buckets <= BUCKET_SORT_MAX_BUCKETS
for every nbins, with the change-overs where they are.  No HIP call is made.  tests/test_gpu_bin_sort.py runs the device part."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sort_checker_catches_every_corruption_and_sizing_holds(tmp_path):
    exe = str(tmp_path / "sortcheck")
    # the program includes the kernels' sources as they are: the full compile, with the library's flags
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-w",
                    os.path.join(ROOT, "tools", "sortcheck.hip"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe, "--selftest"], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    m = re.search(r"^selftest: (\d+) checks, 0 failing$", r.stdout, re.M)
    assert m and int(m.group(1)) >= 40 and "FAILED" not in r.stdout, out
