"""What supersampled frames past 32 light positions do without a GPU: tests/cpp/aa_versions_test.cpp -- the per-pixel state machine
of lights/aa_versions.hpp against a restatement of Draw()'s loop that shades every sub-ray --, tests/cpp/aa_plan_test.cpp -- the
chunks of capi/aa_plan.hpp --, the two new symbols in the header, the library and the package, and the guards of the GPU cases
(test_gpu_aa_many_lights.py), from aa_many_lights.replay on the oracle alone: the replay is the oracle's frame, and every frame has
the partial pixels, the pixels of several versions and the saving its case is about."""
import os
import re
import subprocess

import numpy as np
import pytest

import aa_many_lights as am
import mirt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_versions_counts_and_resolve_order_equal_shading_every_sub_ray(tmp_path):
    exe = str(tmp_path / "aa_versions_test")
    # the headers are HIP source: the host side alone, as test_many_lights_host.py builds the pass plan's program
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "aa_versions_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_chunks_tile_the_band(tmp_path):
    exe = str(tmp_path / "aa_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "aa_plan_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_symbols_header_and_package():
    lib = mirt.load()
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    for name in ("mirt_set_supersampled_many_lights", "mirt_get_supersample_stats"):
        assert hasattr(lib, name) and name in mirt.EXPORTS, name
        assert re.search(r"^MIRT_API int %s\(" % name, hdr, re.M), name
    assert "#define MIRT_ABI_VERSION 4" in hdr and lib.mirt_abi_version() == 4     # additions only
    assert callable(mirt.set_supersampled_many_lights) and callable(mirt.supersample_stats)
    assert "Off by default" in hdr and "later" in hdr
    # before mirt_init both answer with the not-initialised status
    assert lib.mirt_set_supersampled_many_lights(1) == -2 and lib.mirt_get_supersample_stats(None, None) == -2


@pytest.mark.parametrize("name", list(am.FRAMES))
def test_replay_is_the_oracles_frame_and_the_case_has_what_it_is_about(oracle, name):
    f = am.frame(oracle, name)
    ref, rep, aa = f["ref"], f["rep"], f["aa"]
    hits, versions = am.totals(rep)
    assert hits * f["npos"] == ref["nshadow"], (hits, f["npos"], ref["nshadow"])
    assert np.array_equal(rep["index"], ref["index"])
    assert np.array_equal(rep["dist"].view(np.uint32), ref["dist"].view(np.uint32))
    assert np.array_equal(rep["pos"].view(np.uint32), ref["pos"].view(np.uint32))
    partial = int(((rep["hits"] > 0) & (rep["hits"] < aa * aa)).sum())
    several = int((rep["versions"] >= 3).sum())
    print("%s: hit pixels %d, partial %d, hit sub-rays %d, versions %d (%.2f sub-rays per version), pixels of >= 3 versions %d, most %d"
          % (name, int((rep["hits"] > 0).sum()), partial, hits, versions, hits / versions, several, int(rep["versions"].max())))
    assert partial >= 40, partial
    assert several >= 100, several
    assert versions < hits, (versions, hits)
    assert (rep["versions"] <= rep["hits"]).all() and ((rep["versions"] > 0) == (rep["hits"] > 0)).all()
    if name == "cornell_aa8":
        assert int(rep["versions"].max()) == 64
