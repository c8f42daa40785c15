"""tests/cpp/covers_whole_test.cpp on the CPU: covers_whole (csrc/shadowed.hpp), the predicate by which the binned trace kernel decides
that every shadow ray from a triangle towards a light position ends occluded -- against the reference's own arithmetic on ten thousand
hit points of every triple it calls covered, and on the constructed triples it must refuse."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "covers_whole_test.cpp")
HOST = ["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-w"]


def test_predicate_against_the_reference_arithmetic(tmp_path):
    exe = str(tmp_path / "covers_whole_test")
    subprocess.run(HOST + [SRC, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same program, stand-alone, with the host code instrumented."""
    exe = str(tmp_path / "covers_whole_test_san")
    subprocess.run(HOST + ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           SRC, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
