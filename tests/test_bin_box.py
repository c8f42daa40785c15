"""tests/cpp/bin_box_test.cpp on the CPU: add_bbox (csrc/rt_binned.hpp) with one-ulp reciprocals and reciprocal square roots never
places a smaller box than the exact-division code it replaced, gives a box up only for the sharpest corners, and never says "no ray
can hit" where that code did not; box_to_bins with a reciprocal contains the bin range a division gives."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_box_contains_the_exact_division_box_and_empty_stays_conservative(tmp_path):
    exe = str(tmp_path / "bin_box_test")
    # the header is HIP source: the host side alone, with the library's floating-point contract
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-w",
                    os.path.join(ROOT, "tests", "cpp", "bin_box_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
