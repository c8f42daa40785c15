"""tests/cpp/trace_flags_test.cpp on the CPU: the trace kernel's flags word as the host derives it (csrc/rt_trace_frame.hpp) and the
layout of RtTraceFrame, which the kernel and capi/binned.cpp share through that header -- the host pass and the device pass of the
compiler must lay it out alike."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "trace_flags_test.cpp")
HOST = ["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-w"]


def test_flags_word_and_host_layout(tmp_path):
    exe = str(tmp_path / "trace_flags_test")
    subprocess.run(HOST + [SRC, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_device_pass_lays_the_block_out_alike(tmp_path):
    """The file's static_asserts name every offset as a number: they must hold in the device pass too."""
    subprocess.run(["hipcc", "-x", "hip", "--cuda-device-only", "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-w",
                    "-c", SRC, "-o", str(tmp_path / "device.o")], check=True, timeout=300)


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same program, stand-alone, with the host code instrumented."""
    exe = str(tmp_path / "trace_flags_test_san")
    subprocess.run(HOST + ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           SRC, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
