"""capi/dof_plan.hpp on the CPU: tests/cpp/dof_plan_test.cpp as a stand-alone program, plain and under the sanitizers, and the rule the
halo exists for, simulated with the oracle alone: a band blurred from its own rows plus dof_halo_rows(K, W) rows on either side --
everything else zeroed, which is what the kernels make of a tap outside the rows a call rendered -- equals the same rows of the
frame blurred whole, bit for bit.  The blur addresses its taps by flat index, so on a frame narrower than about K / 2 a tap column
wraps by more than one row; the halo the library rendered before, max(-zlo, zhi - 1) + 1, allowed for one."""
import math
import os
import subprocess

import numpy as np
import pytest

import mirt
from mirt_oracle import DEFAULT_LIGHT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dof_plan_test.cpp")
HOST = ["hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-w"]

# (W, H, K): frames so narrow that a tap column wraps by two rows or more
NARROW = [(6, 120, 24), (4, 96, 16), (12, 160, 48), (3, 96, 12), (5, 120, 17)]


def bands_of(H):
    return [(0, H // 2), (H // 2, H // 2 + 1), (H // 2 + 1, H)]


def one_wrap_halo(K):
    """The halo before dof_halo_rows, the thing guarded against: one row beyond the tap rows, for a column that wraps once."""
    zlo, zhi = math.ceil(K / -2.0), math.ceil(K / 2.0)
    return max(-zlo, zhi - 1) + 1


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dof_plan") / "dof_plan_test")
    subprocess.run(HOST + [SRC, "-o", exe], check=True, timeout=300)
    return exe


def halo_rows(program, pairs):
    """dof_halo_rows for (K, W) pairs, from the library's own header."""
    r = subprocess.run([program] + [str(v) for kw in pairs for v in kw], capture_output=True, text=True, timeout=120, check=True)
    out = [int(s) for s in r.stdout.split()]
    assert len(out) == len(pairs)
    return out


def narrow_planes(oracle, W, H):
    """pixelColours and focalDistances of the narrow cases' frame: every |fd| >= 1 where a ray hit, so each off-centre tap weighs 1 / K^2."""
    tris = np.concatenate([mirt.scene_cornell(), mirt.scene_soup(9, 400, 0.12)])
    ref = oracle.raytrace(tris, (0.3, 0, -2), oracle.rot_from_yaw(0.1, 1.0), H / 2.0, W, H, DEFAULT_LIGHT)
    fd = np.where(ref["index"] >= 0, ref["dist"] - np.float32(0.2), np.float32(0)).astype(np.float32)
    return ref["rgb"], fd


def banded(oracle, rgb, fd, K, halo):
    """The frame blurred band by band, each band seeing its rows and `halo` rows on either side, zeros elsewhere."""
    H, W = fd.shape
    out = np.full((H, W), 0x5A5A5A5A, np.uint32)
    for y0, y1 in bands_of(H):
        lo, hi = max(0, y0 - halo), min(H, y1 + halo)
        brgb, bfd = np.zeros_like(rgb), np.zeros_like(fd)
        brgb[lo:hi], bfd[lo:hi] = rgb[lo:hi], fd[lo:hi]
        oracle.dof(brgb, bfd, K, xrgb=out, y0=y0, y1=y1)
    return out


def test_stand_alone_program(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same program, stand-alone, with the host code instrumented."""
    exe = str(tmp_path / "dof_plan_test_san")
    subprocess.run(HOST + ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           SRC, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_printed_halos(program):
    assert halo_rows(program, [(24, 6), (16, 4), (64, 3), (8, 1920), (8, 3840), (2, 97), (64, 32768)]) == [14, 10, 43, 5, 5, 2, 33]
    pairs = [(K, W) for K in (2, 3, 8, 16, 17, 64) for W in (64, 129, 1920)]
    assert halo_rows(program, pairs) == [one_wrap_halo(K) for K, W in pairs]      # wide frames: the halo they always had


@pytest.mark.parametrize("W,H,K", NARROW)
def test_a_band_of_a_narrow_frame_equals_the_frame(oracle, program, W, H, K):
    rgb, fd = narrow_planes(oracle, W, H)
    assert (np.abs(fd[1:-1, 1:-1]) >= 1).all()
    full = oracle.dof(rgb, fd, K, xrgb=np.full((H, W), 0x5A5A5A5A, np.uint32))
    halo, = halo_rows(program, [(K, W)])
    assert halo > one_wrap_halo(K)
    got = banded(oracle, rgb, fd, K, halo)
    assert np.array_equal(got, full), "%d pixels differ with a halo of %d rows" % (int((got != full).sum()), halo)
    # the case has teeth: with the one-wrap halo some tap of some band falls on a zeroed row and changes a pixel
    old = banded(oracle, rgb, fd, K, one_wrap_halo(K))
    differing = int((old != full).sum())
    print("%dx%d K %d: halo %d (was %d), %d pixels differ with the old one" % (W, H, K, halo, one_wrap_halo(K), differing))
    assert differing >= 1
