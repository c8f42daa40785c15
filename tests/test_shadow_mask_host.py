"""What the shadow masks (mirt_shadow_mask*, mirt_direct_light_masked*) do without a GPU: tests/cpp/light_mask_test.cpp -- the word
and bit arithmetic of query/light_mask.hpp over every pass and every pass plan a call can run --, the symbols, the ABI version, the
order of the entry points' checks and the shapes the Python wrappers insist on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mirt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mirt_shadow_mask", "mirt_shadow_mask_device", "mirt_direct_light_masked", "mirt_direct_light_masked_device",
           "mirt_get_shadow_mask_stats")
MIRT_ERR_NOT_INITIALISED = -2


def test_passes_put_their_bits_into_the_right_words(tmp_path):
    exe = str(tmp_path / "light_mask_test")
    # the headers are HIP source: the host side alone; a stand-alone program under the address and undefined-behaviour sanitizers
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "light_mask_test.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_symbols_header_and_abi():
    lib = mirt.load()
    text = open(os.path.join(ROOT, "include", "mirt.h")).read()
    declared = set(re.findall(r"MIRT_API\s+[\w\s\*]+?\b(mirt_\w+)\s*\(", text))
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in mirt.EXPORTS and name in declared, name
    assert lib.mirt_abi_version() == 4                        # additions only
    assert re.search(r"^#define MIRT_ABI_VERSION 4$", text, re.M)


def test_mask_words_macro_agrees_with_the_package():
    text = open(os.path.join(ROOT, "include", "mirt.h")).read()
    m = re.search(r"^#define MIRT_MASK_WORDS\(npositions\) (.+)$", text, re.M)
    assert m, "MIRT_MASK_WORDS is not defined as the issue states it"
    expr = m.group(1).replace("/", "//")                      # C's integer division
    for npos in list(range(0, 70)) + [255, 256]:
        assert eval(expr, {"npositions": npos}) == mirt.mask_words(npos) == (npos + 31) // 32, npos


def test_every_entry_point_asks_for_init_first():
    """Before mirt_init every new entry point answers MIRT_ERR_NOT_INITIALISED -- with arguments each of which a later check would
    refuse (negative counts, NULL arrays, too many lights)."""
    lib = mirt.load()
    lib.mirt_shutdown()
    bad = (None, -1, None, 99)
    assert lib.mirt_shadow_mask(*bad, None) == MIRT_ERR_NOT_INITIALISED
    assert lib.mirt_shadow_mask_device(*bad, None) == MIRT_ERR_NOT_INITIALISED
    assert lib.mirt_direct_light_masked(*bad, None, None) == MIRT_ERR_NOT_INITIALISED
    assert lib.mirt_direct_light_masked_device(*bad, None, None) == MIRT_ERR_NOT_INITIALISED
    assert lib.mirt_get_shadow_mask_stats(None) == MIRT_ERR_NOT_INITIALISED
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.shadow_mask(mirt.fresh_hits(3), mirt.DEFAULT_LIGHT)


def test_wrappers_refuse_a_mask_of_the_wrong_shape_or_type():
    hits = mirt.fresh_hits(5)
    L = np.array([[0, 0, 0, 1, 1, 1, 1]] * 3, np.float32)
    for mask in (np.zeros((1, 5), np.int32), np.zeros((1, 5), np.float32), np.zeros(5, np.uint32), np.zeros((1, 4), np.uint32),
                 np.zeros((5, 1), np.uint32), np.zeros((0, 5), np.uint32), [[0] * 5]):
        with pytest.raises(ValueError, match="mask"):
            mirt.direct_light_masked(hits, L, mask)
    # (a mask of the right shape gets as far as the library, which has no context here)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.direct_light_masked(hits, L, np.zeros((1, 5), np.uint32))
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.direct_light_masked(hits, L, np.zeros((2, 5), np.uint32))     # more planes than the lights need: a prefix is read
