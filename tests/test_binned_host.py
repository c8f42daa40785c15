"""What the binned ray tracer's host side decides without a GPU: tests/cpp/pass_plan_test.cpp checks capi/pass_plan.hpp -- whether a
kept pass still serves, how a pair list is sized, the depth shells within the sort's key space, the light cubes' frame descriptors and
the empty-cube rule of the view makers -- as pure functions."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pass_plan_decisions(tmp_path):
    exe = str(tmp_path / "pass_plan_test")
    # the headers are HIP source: the host side alone; a stand-alone program under the address and undefined-behaviour sanitizers
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "pass_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
