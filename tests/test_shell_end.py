"""tests/cpp/shell_end_test.cpp on the CPU: bin_shell_of (csrc/rt_binned.hpp) is monotone and its host twin returns what the
device returns, and the trace kernel's early end of a shell-sorted list never drops a candidate within the bound."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shell_rule_is_monotone_and_drops_nothing_within_the_bound(tmp_path):
    exe = str(tmp_path / "shell_end_test")
    # the header is HIP source: the host side alone, with the library's floating-point contract
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-w",
                    os.path.join(ROOT, "tests", "cpp", "shell_end_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
