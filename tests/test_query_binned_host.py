"""The DirectLight query mode and statistics (mirt_set_query_mode, mirt_get_query_stats), the part that needs no GPU: the
symbols, the layouts of the binding, and the loud failure without mirt_init."""
import ctypes as C
import os
import re

import pytest

import mirt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_header():
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    lib = mirt.load()
    for name in ("mirt_set_query_mode", "mirt_get_query_stats"):
        assert hasattr(lib, name) and name in mirt.EXPORTS, name
    # the header / EXPORTS equality of test_capi_symbols.py, with the new entry points in it
    declared = set(re.findall(r"MIRT_API\s+[\w\s\*]+?\b(mirt_\w+)\s*\(", hdr))
    assert declared == set(mirt.EXPORTS), declared ^ set(mirt.EXPORTS)
    assert re.search(r"MIRT_QUERY_AUTO = 0, MIRT_QUERY_BRUTE = 1, MIRT_QUERY_BINNED = 2", hdr)
    assert (mirt.QUERY_AUTO, mirt.QUERY_BRUTE, mirt.QUERY_BINNED) == (0, 1, 2)
    assert "#define MIRT_ABI_VERSION 4" in hdr and lib.mirt_abi_version() == 4     # additions only


def test_query_stats_layout():
    # four int32 then four uint64, no padding: as the header declares mirt_query_stats
    assert C.sizeof(mirt.QueryStats) == 4 * 4 + 4 * 8
    assert [n for n, _ in mirt.QueryStats._fields_] == ["mode_used", "cube_source", "cube_bins", "shells", "shadow_rays", "candidates", "tests",
                                                        "fallback_records"]
    hdr = open(os.path.join(ROOT, "include", "mirt.h")).read()
    body = re.search(r"typedef struct mirt_query_stats \{(.*?)\} mirt_query_stats;", hdr, re.S).group(1)
    assert re.findall(r"\b(?:int32_t|uint64_t)\s+(\w+);", body) == [n for n, _ in mirt.QueryStats._fields_]


def test_calls_need_mirt_init():
    mirt.shutdown()
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.set_query_mode(mirt.QUERY_BINNED)
    with pytest.raises(mirt.MirtError, match="mirt_init"):
        mirt.query_stats()
    lib = mirt.load()
    s = mirt.QueryStats()
    assert lib.mirt_set_query_mode(0) == -2 and lib.mirt_set_query_mode(7) == -2      # the not-initialised status comes first
    assert lib.mirt_get_query_stats(C.byref(s)) == -2 and lib.mirt_get_query_stats(None) == -2
    assert b"mirt_init" in lib.mirt_last_error()
