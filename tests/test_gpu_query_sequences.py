"""tests/fuzz_queries.py inside the suite: the seeded call sequences over ray queries, scene changes and frames with up to 48 light
positions, every result against the CPU oracle (the fuzzer's docstring says what a sequence holds; test_query_sequences_host.py
checks, without a GPU, that these very seeds contain the op kinds, forms, modes and ordered pairs they are there for).

Three runs of the same seeds that differ in the environment only: the defaults; MIRT_QUERY_WAVE_RAYS=128, with which batches of 96
to 320 rays reach both the wave-per-ray and the lane-per-ray kernels of intersect and occluded; MIRT_MANY_LIGHTS_MIN=1, with which
every frame without supersampling is deferred.

The seed count (fuzz_queries.SUITE_SEEDS: 20 seeds, 640 ops) is chosen so that a case takes no longer than the
`fuzz_sequence.py 1000 20` case of test_gpu_fuzz_smoke.py.  Wall times on an MI355X, measured in one run of the suite:

    test_fuzzer_finds_no_mismatch[fuzz_sequence.py-args0]          15.96 s
    test_query_sequences_find_no_mismatch[default]                  5.60 s
    test_query_sequences_find_no_mismatch[wave-rays-128]            5.58 s
    test_query_sequences_find_no_mismatch[many-lights-min-1]        5.45 s

(about half of a case is the oracle on the CPU).  The long run, 300 seeds, is in the fuzz stage of tools/collect_profiles.sh;
its summary: profiles/fuzz_query_call_sequences.txt."""
import os
import subprocess
import sys

import pytest

import fuzz_queries as fq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"MIRT_QUERY_WAVE_RAYS": "128"}, {"MIRT_MANY_LIGHTS_MIN": "1"}], ids=["default", "wave-rays-128", "many-lights-min-1"])
def test_query_sequences_find_no_mismatch(env):
    """One child process per case (it initialises the library itself; the environment is read once)."""
    first, count = fq.SUITE_SEEDS
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_queries.py"), str(first), str(count)], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout, (r.stdout[-6000:] + r.stderr[-3000:])
