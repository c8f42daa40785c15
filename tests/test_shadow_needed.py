"""tests/cpp/shadow_needed_test.cpp on the CPU: shadow_ray_needed (csrc/rt_common.hpp), the test by which the binned trace kernel
decides that a pixel's shadow ray cannot change the frame, on signed zeros, NaN, infinities, denormals and ordinary values -- and the
IEEE argument beside it: adding a D it calls unneeded leaves the bits that adding +0 leaves."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "shadow_needed_test.cpp")
HOST = ["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-w"]


def test_predicate_and_the_sums_it_rests_on(tmp_path):
    exe = str(tmp_path / "shadow_needed_test")
    subprocess.run(HOST + [SRC, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same program, stand-alone, with the host code instrumented."""
    exe = str(tmp_path / "shadow_needed_test_san")
    subprocess.run(HOST + ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           SRC, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
