"""What soft shadows past 32 light positions do without a GPU: tests/cpp/light_passes_test.cpp -- the pass plan of a DirectLight
call of up to 256 positions and the order of its accumulator updates, as pure functions of the light count, the sample count and the
scene's size --, the symbols, the ABI version and the limit the Python package exports."""
import os
import re
import subprocess

import mirt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_passes_tile_the_positions_and_keep_the_accumulators_order(tmp_path):
    exe = str(tmp_path / "light_passes_test")
    # the headers are HIP source: the host side alone; a stand-alone program under the address and undefined-behaviour sanitizers
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "light_passes_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_symbols_and_limits():
    lib = mirt.load()
    for name in ("mirt_set_soft_shadows", "mirt_direct_light", "mirt_direct_light_device", "mirt_get_query_stats", "mirt_raytrace",
                 "mirt_raytrace_device", "mirt_raytrace_ex", "mirt_raytrace_device_ex"):
        assert hasattr(lib, name) and name in mirt.EXPORTS, name
    assert lib.mirt_abi_version() == 4                        # additions only
    assert mirt.MAX_LIGHT_POSITIONS == 256 and mirt.MAX_LIGHTS == 32


def test_header_states_the_limit_the_package_exports():
    text = open(os.path.join(ROOT, "include", "mirt.h")).read()
    m = re.search(r"^#define MIRT_MAX_LIGHT_POSITIONS (\d+)", text, re.M)
    assert m and int(m.group(1)) == mirt.MAX_LIGHT_POSITIONS
    assert "randomPositions[256]" in text and "supersampling" in text.lower()
