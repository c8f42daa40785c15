"""The rasteriser's edge walk on tall triangles, and the read-back sizing of its span table, against the CPU oracle.

launch_raster (csrc/raster_kernels.hip) picks the edge kernel and the size of the span table from the triangle count (<= 64, <= 4096,
more), the rows of the band, the tallest triangle's rows inside it, MIRT_RASTER_LDS_ROWS (default and cap 2560), the frames in flight
(edge_segments) and whether n x band rows x 48 B fits 64 MiB.  The frames here are NARROW and TALL, so that the regimes no other test
reaches cost milliseconds: k_raster_edges with several 512-step chunks (double buffer, tail chunk, skip > 0, the hand-over
`rows <= handled_rows`), both edge kernels in one frame (the `tall` branch), the LDS kernel at its 2560-row cap, the 1024-thread LDS
kernel with a spoilt prediction and with the whole-chain walk, read-back sizing combined with `tall`, regrowth of the tables, and
walks that start ~10^5 rows outside the band.

Nothing reports which edge kernel ran, so every case first asserts -- from the oracle alone -- that its frame is in the regime it
names (`_guard`): a triangle of more than T rows that owns >= 1000 pixels, a triangle of 1..T rows that owns pixels, and for the
multi-chunk cases an owning triangle more than 1024 rows above what the LDS kernel takes (two full chunks and a tail).  A guard that
fails is a failed test.

What the guards saw when the frames were chosen (cull flags 0, m11 = 1.01, focal = H, the reference's light; rows and owned pixels from
the oracle's VertexShader and index plane):
  a  Cornell box, camera (-0.1,0,-2.75), yaw 0.45, 48x2700    2 triangles > 2560 rows, one owns 119 558 px (2700 rows); 3 shorter owners
  b  Cornell box, camera (0.3,0,-3), yaw 0.45, 64x4320        5 triangles > 2560 rows, two own 122 411 and 64 473 px; tallest owner 3687 rows
  c  soup(5,300,0.4) + Cornell, as a                          n = 330: key buffer, worst-case table (42.8 MB), `tall`; tall owner 115 608 px; 6 shorter owners
  d  soup(5,1500,0.3) + Cornell, as a                         n = 1530, 198 MB > 64 MiB: read-back after the single-launch scan, `tall`; 115 918 px; 9 shorter owners
  e  soup(6,5000,0.2) + Cornell, as a                         n = 5030: three-pass scan, read-back, `tall`; tall owner 54 801 px; 24 shorter owners
  f  Cornell box, camera (-0.2,-0.2,-1.5), yaw 0.15, 40x1300  14 triangles > 512 rows (4 own pixels, 17 362 the most), 10 of <= 512 (4 owners);
                                                              22 > 40 rows (6 owners), 2 of <= 40 rows (both owners); tallest owner 1108 rows
  g  soup(7,200,0.4) + Cornell, as f                          n = 230; 36 > 512 rows (5 owners, 9016 px the most); 177 > 40 rows (24 owners), 8 of <= 40 (2 owners);
                                                              tallest owner 1243 rows
  h  soup(8,4200,0.1) + Cornell, as f                         n = 4230; 15 > 512 rows (4 owners, 8271 px the most); 2312 > 40 rows (99 owners), 680 of <= 40
                                                              (11 owners); tallest owner 1108 rows; an owner of exactly 41 rows; in the band
                                                              [0,185) an owner (586 px) of exactly 40 rows, which has 41 in [0,186)
  i  Cornell box, camera (0,0,-3), yaw 0.1, 33x200            26 triangles > 40 rows (10 owners, 1451 px the most); 4 of <= 40 rows (1 owner)
  j  soup(9,90,0.6), camera (0,0,-2.5), yaw 0.1, 33x200       30 triangles > 40 rows (15 owners, 1216 px the most); 60 of <= 40 rows (21 owners)
With the cameras (0,0,-3) for a, c-e and (0.1,0,-3) for f-h the tallest OWNING triangle has 2439 and 687 rows: those frames are not in
the regimes they name, hence the cameras above.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import mirt
from mirt_oracle import DEFAULT_LIGHT

pytestmark = pytest.mark.gpu

TOL = 1e-4                  # per-channel colour tolerance of the project's bar (the planes are in fact compared as bits)
COORD_LIMIT = 1 << 20       # RASTER_COORD_LIMIT (csrc/raster_common.hpp): a projected vertex beyond it puts the triangle out of contract
LDS_CAP = 2560              # MIRT_RASTER_LDS_ROWS: default and cap
CHUNK = 512                 # EDGE_CHUNK of k_raster_edges
FILL = 0x5A                 # byte a device surface starts with
FILL_WORD = 0x5A5A5A5A
INDIRECT = (0.2, 0.2, 0.2)
M11 = 1.01

# name -> (scene, camera, yaw, W, H); focal = H.  scene: None = the Cornell box alone, (seed, n, s) = that soup in front of the Cornell box,
# (seed, n, s, False) = the soup alone
FRAMES = {
    "a": (None, (-0.1, 0.0, -2.75), 0.45, 48, 2700),
    "b": (None, (0.3, 0.0, -3.0), 0.45, 64, 4320),
    "c": ((5, 300, 0.4), (-0.1, 0.0, -2.75), 0.45, 48, 2700),
    "d": ((5, 1500, 0.3), (-0.1, 0.0, -2.75), 0.45, 48, 2700),
    "e": ((6, 5000, 0.2), (-0.1, 0.0, -2.75), 0.45, 48, 2700),
    "f": (None, (-0.2, -0.2, -1.5), 0.15, 40, 1300),
    "g": ((7, 200, 0.4), (-0.2, -0.2, -1.5), 0.15, 40, 1300),
    "h": ((8, 4200, 0.1), (-0.2, -0.2, -1.5), 0.15, 40, 1300),
    "i": (None, (0.0, 0.0, -3.0), 0.1, 33, 200),
    "j": ((9, 90, 0.6, False), (0.0, 0.0, -2.5), 0.1, 33, 200),
}
BANDS_2700 = [(0, 100), (100, 2650), (2650, 2700)]
BANDS_1300 = [(0, 37), (37, 1290), (1290, 1300)]
HANDOVER_BANDS_H = [(0, 185), (0, 186)]                      # frame h under MIRT_RASTER_LDS_ROWS=40: an owner of exactly 40 / 41 rows in the band
SKIP_INTO_LAST_BAND = {"a": 2550, "c": 2550, "h": 512}      # rows some owner of the last band starts above it (guarded)


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)          # raises MirtError (fails loudly) when libmirt.so or the GPU is missing
    yield
    mirt.shutdown()


# ---- the oracle's side: scenes, frames, and the rows / owned pixels the guards are stated in -------------------------------------

def scene_of(oracle, spec):
    if spec is None:
        return oracle.cornell()
    soup = oracle.soup(*spec[:3])
    return soup if len(spec) > 3 else np.concatenate([soup, oracle.cornell()])


def projected_rows(oracle, tris, culled, cam, rot, focal, W, H):
    """(minY, maxY, in_contract) per triangle from the oracle's VertexShader; culled triangles are out."""
    n = len(tris)
    ymin, ymax, ok = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
    for t in range(n):
        if culled[t]:
            continue
        xs, ys = [], []
        for k in range(3):
            x, y, _, _ = oracle.vertex_shader(tris[t, 3 * k:3 * k + 3], cam, rot, focal, W, H)
            xs.append(x); ys.append(y)
        ymin[t], ymax[t] = min(ys), max(ys)
        ok[t] = all(-COORD_LIMIT < v < COORD_LIMIT for v in xs + ys)
    return ymin, ymax, ok


def band_rows(proj, y0, y1):
    """Rows of each triangle inside the band [y0, y1): clamp(maxY, y1-1) - clamp(minY, y0) + 1, 0 for culled / out-of-contract ones."""
    ymin, ymax, ok = proj
    rows = np.minimum(ymax, y1 - 1) - np.maximum(ymin, y0) + 1
    return np.where(ok & (rows > 0), rows, 0)


def owned_pixels(index, n, y0=0, y1=None):
    own = index[y0:y1]
    return np.bincount(own[own >= 0].ravel(), minlength=n)[:n]


class Case:
    """One view of one scene: the oracle's frame, computed once and left unchanged, and what the guards need."""

    def __init__(self, oracle, tris, cam, yaw, W, H, cull_flags=0, lights=DEFAULT_LIGHT):
        self.tris, self.cam, self.W, self.H, self.lights = tris, cam, W, H, lights
        self.focal = float(H)
        self.rot = oracle.rot_from_yaw(yaw, M11)
        self.cull_flags = cull_flags
        self.culled = oracle.cull(tris, cam, self.rot, self.focal, W, H, cull_flags)
        self.ref = oracle.rasterise(tris, self.culled, cam, self.rot, self.focal, W, H, lights)
        for plane in self.ref.values():
            if plane is not None:
                plane.setflags(write=False)
        self.proj = projected_rows(oracle, tris, self.culled, cam, self.rot, self.focal, W, H)
        self.rows = band_rows(self.proj, 0, H)
        self.owned = owned_pixels(self.ref["index"], len(tris))

    def view(self):
        return mirt.make_view(self.cam, self.rot, self.focal, self.W, self.H)


_cases = {}


def frame_case(oracle, name):
    if name not in _cases:
        spec, cam, yaw, W, H = FRAMES[name]
        _cases[name] = Case(oracle, scene_of(oracle, spec), cam, yaw, W, H)
    return _cases[name]


def _guard(rows, owned, T, multi_chunk_above=None, what=""):
    """The frame (or band) is in the regime the case names; returns the figures it saw, for the record."""
    tall = (rows > T) & (owned >= 1000)
    short = (rows >= 1) & (rows <= T) & (owned > 0)
    seen = "%s T=%d: %d triangles > T rows (%d owning, largest %d px), %d of 1..T rows (%d owning), tallest owner %d rows" % (
        what, T, int((rows > T).sum()), int(((rows > T) & (owned > 0)).sum()), int(owned[rows > T].max(initial=0)),
        int(((rows >= 1) & (rows <= T)).sum()), int(short.sum()), int(rows[owned > 0].max(initial=0)))
    print(seen)
    assert tall.any(), "no triangle of more than T rows owns 1000 pixels -- " + seen
    assert short.any(), "no triangle of 1..T rows owns a pixel -- " + seen
    if multi_chunk_above is not None:
        assert rows[owned > 0].max() > multi_chunk_above + 2 * CHUNK, "the tallest owner does not walk two full chunks and a tail -- " + seen
    return seen


# ---- the GPU's side ----------------------------------------------------------------------------------------------------------

def assert_planes(got, ref, what=""):
    """The comparisons of _raster_compare (test_gpu_parity.py): owner index, depth bits, float colour bits and XRGB words all equal."""
    assert np.array_equal(got["index"], ref["index"]), "%sowner triangle differs in %d pixels" % (what, int((got["index"] != ref["index"]).sum()))
    assert np.array_equal(got["depth"].view(np.uint32), ref["depth"].view(np.uint32)), "%sdepth differs in %d pixels" % (
        what, int((got["depth"].view(np.uint32) != ref["depth"].view(np.uint32)).sum()))
    assert np.max(np.abs(got["rgb"] - ref["rgb"])) <= TOL, what
    assert np.array_equal(got["rgb"].view(np.uint32), ref["rgb"].view(np.uint32)), what + "float colours not bit-identical"
    assert np.array_equal(got["xrgb"], ref["xrgb"]), "%s%d XRGB words differ" % (what, int((got["xrgb"] != ref["xrgb"]).sum()))


def compare_planes(case):
    """_raster_compare of test_gpu_parity.py with the reference already computed: cull flags and every plane equal."""
    view = case.view()
    assert np.array_equal(mirt.cull(case.tris, view, case.cull_flags), case.culled)
    mirt.scene_upload(case.tris, case.culled)
    assert_planes(mirt.rasterise(view, case.lights), case.ref)


def compare_bands(case, bands):
    """Each band through mirt.rasterise_device into a surface of its own: the band's rows are the oracle's, every other row keeps its
    fill word."""
    from devbuf import DeviceArray
    view = case.view()
    mirt.scene_upload(case.tris, case.culled)
    for (y0, y1) in bands:
        with DeviceArray((case.H, case.W), np.uint32, FILL) as surf:
            mirt.rasterise_device(view, case.lights, INDIRECT, y0, y1, 0, surf.ptr, case.W * 4)
            got = surf.read()
        want = case.ref["xrgb"][y0:y1]
        assert np.array_equal(got[y0:y1], want), "band [%d, %d): %d words differ" % (y0, y1, int((got[y0:y1] != want).sum()))
        assert (got[:y0] == FILL_WORD).all() and (got[y1:] == FILL_WORD).all(), "band [%d, %d) wrote outside its rows" % (y0, y1)


def guard_band_is_drawn(case, y0, y1):
    """Some triangle has rows inside the band and owns pixels there."""
    rows, owned = band_rows(case.proj, y0, y1), owned_pixels(case.ref["index"], len(case.tris), y0, y1)
    assert ((rows > 0) & (owned > 0)).any(), "nothing is drawn in band [%d, %d)" % (y0, y1)
    return rows, owned


# ---- 1. default thresholds ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_flight", [1, 3])
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_tall_frames_at_the_default_thresholds(oracle, name, in_flight):
    """Frames taller than the LDS kernel's cap: k_raster_edges_lds (1024 threads, 153 840 B of LDS) for the triangles of up to 2560
    rows and k_raster_edges, six to eight 512-step chunks a triangle, for the taller ones, in one frame.  a, b: small-scene kernel; c: key buffer with the
    worst-case table; d: read-back sizing after the single-launch vertex scan; e: after the three-pass scan.  One frame in flight walks
    the LDS chains as 64 checked segments, three walk them whole."""
    case = frame_case(oracle, name)
    _guard(case.rows, case.owned, LDS_CAP, multi_chunk_above=LDS_CAP if name == "b" else None, what="frame " + name)
    n, worst = len(case.tris), len(case.tris) * case.H * 48
    assert {"a": n <= 64, "b": n <= 64, "c": 64 < n <= 4096 and worst <= 64 << 20, "d": n <= 4096 and worst > 64 << 20, "e": n > 4096}[name]
    mirt.set_frames_in_flight(in_flight)
    try:
        compare_planes(case)
    finally:
        mirt.set_frames_in_flight(1)


# ---- 2. bands of a tall frame --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["a", "c", "h"])
def test_bands_of_a_tall_frame(oracle, name):
    """A tall frame in three bands: every edge that comes down into a later band is walked `skip` steps before its first stored
    sample (~2650 of them in the last band of a and c, whose LDS table holds 50 rows)."""
    case = frame_case(oracle, name)
    bands = BANDS_1300 if name == "h" else BANDS_2700
    _guard(case.rows, case.owned, 512 if name == "h" else LDS_CAP, what="frame " + name)
    for (y0, y1) in bands:
        rows, owned = guard_band_is_drawn(case, y0, y1)
        if y0 > 0:
            # an owner of this band starts above it: by at least SKIP_INTO_LAST_BAND rows in the last one
            far = SKIP_INTO_LAST_BAND[name] if y1 == case.H else 1
            starts_above = (rows > 0) & (owned > 0) & (case.proj[0] <= y0 - far)
            print("frame %s band [%d, %d): %d owners walk in from >= %d rows above" % (name, y0, y1, int(starts_above.sum()), far))
            assert starts_above.any(), "no edge walks into band [%d, %d) from %d rows above it" % (y0, y1, far)
    compare_bands(case, bands)


# ---- 3. long skip --------------------------------------------------------------------------------------------------------------

def _long_skip_case(oracle):
    if "skip" not in _cases:
        tris = np.zeros((3, 15), np.float32)
        tris[0, 0:9] = [0.02, -50, 0.1, -0.5, 0.3, 1.0, 0.5, 0.4, 1.0]
        tris[1, 0:9] = [-0.6, -0.8, 1.5, 0.6, -0.8, 1.5, 0, 0.9, 1.5]
        tris[2, 0:9] = [0.3, 0.2, 0.6, -0.01, 60, 0.12, -0.3, 0.1, 0.6]
        tris[:, 9:15] = oracle.cornell()[[0, 4, 8], 9:15]           # normals and colours of three Cornell triangles
        _cases["skip"] = Case(oracle, tris, (0.0, 0.0, 0.0), 0.0, 33, 200)
    return _cases["skip"]


@pytest.mark.parametrize("how", ["one-in-flight", "three-in-flight", "two-bands"])
def test_edges_that_start_far_outside_the_frame(oracle, how):
    """Vertices ~10^5 rows above and below the frame (inside RASTER_COORD_LIMIT): the walk before the first stored sample is
    ~10^5 additions, or a 64-lane prediction over T = skip + L, and must still end on the reference's sums."""
    case = _long_skip_case(oracle)
    ymin, ymax, ok = case.proj
    owning = ok & (case.owned > 0)
    print("long skip: minY %s maxY %s owned %s" % (ymin.tolist(), ymax.tolist(), case.owned.tolist()))
    assert (owning & (ymin < -50000)).any() and (owning & (ymax > 50000)).any()
    if how == "two-bands":
        for (y0, y1) in [(0, 77), (77, 200)]:
            guard_band_is_drawn(case, y0, y1)
        compare_bands(case, [(0, 77), (77, 200)])
        return
    mirt.set_frames_in_flight(1 if how == "one-in-flight" else 3)
    try:
        compare_planes(case)
    finally:
        mirt.set_frames_in_flight(1)


# ---- 4. read-back sizing over a sequence ---------------------------------------------------------------------------------------

# (camera z, cull flags, what launch_raster does with the frame on a stream whose tables start empty)
SIZING_SEQUENCE = [(-6.5, 0, "read-back, grows"), (-6.5, 0, "reuse"), (-3.0, 0, "read-back, grows"), (-3.0, 1, "read-back"), (-3.0, 3, "read-back"),
                   (-2.2, 0, "read-back, grows"), (-6.5, 0, "read-back"), (-6.5, 0, "reuse")]
ROWS_AT_INIT = 4096 + 4096 // 8 + 1024      # raster_scratch_ensure: ensure_rows(4096) on a stream's first frame


def _sizing_case(oracle, z, flags):
    key = ("sizing", z, flags)
    if key not in _cases:
        spec, _, yaw, W, H = FRAMES["h"]
        _cases[key] = Case(oracle, scene_of(oracle, spec), (0.1, 0.0, z), yaw, W, H, cull_flags=flags)
    return _cases[key]


@pytest.mark.parametrize("in_flight", [1, 3])
def test_read_back_sizing_follows_the_view(oracle, in_flight):
    """n = 4230 > 4096: the tables are sized from the row count read back when the frame's inputs change (view, band, triangle count,
    scene and cull versions: frame_key), and the count -- with max_rows, from which lds_rows and `tall` follow -- is reused while they
    stand still.  The library is started afresh, so every stream's tables begin at 5632 rows; the scene is uploaded ONCE and the cull
    flags are set only where they change, so a repeated view really repeats its key.  On each stream, in this order:
      0  camera z = -6.5, flags 0   81 631 rows in all     read-back; the tables grow to 92 858 rows
      1  the same again                                    REUSE: no read-back, no new flags
      2  z = -3                     180 459                read-back (the view changed); > 92 858: the tables regrow, to 204 040
      3  z = -3, flags 1            92 237 (2154 culled)   read-back (new flags); tables kept
      4  z = -3, flags 3            7035 (4054 culled)     read-back; tallest triangle 114 rows after 1300: max_rows and lds_rows change,
                                                           the 256-thread LDS kernel after the 1024-thread one
      5  z = -2.2, flags 0          223 992                read-back; > 204 040: regrows, to 253 015
      6  z = -6.5, flags 0          81 631                 read-back; tables three times what the frame needs
      7  the same again                                    REUSE, of a count that is not the tables' size
    (figures: the oracle's, asserted below as relations, not as absolute numbers).  One frame in flight: the eight frames queue on one
    stream.  Three in flight: calls take the streams in turn, so every entry is rendered three times in a row -- frame 3k + s is entry k
    on stream s, each stream sizes its own tables through the whole sequence and reuses its own count at entries 1 and 7 -- and up to
    nine frames are queued before anything waits.  Every plane of every frame is read after mirt.sync(), which also reports a table
    that a reused count left too small."""
    from devbuf import DeviceArray
    cases = [_sizing_case(oracle, z, flags) for z, flags, _ in SIZING_SEQUENCE]
    total = [int(c.rows.sum()) for c in cases]
    print("rows in all: %s, culled: %s, tallest: %s" % (total, [int(c.culled.sum()) for c in cases], [int(c.rows.max()) for c in cases]))
    assert all(len(c.tris) > 4096 for c in cases)
    cap, new_flags = ROWS_AT_INIT, []
    for i, (c, (z, flags, does)) in enumerate(zip(cases, SIZING_SEQUENCE)):
        prev = cases[i - 1] if i else None
        new_flags.append(i > 0 and not np.array_equal(c.culled, prev.culled))
        same_key = i > 0 and not new_flags[i] and c.cam == prev.cam            # (size, yaw, focal length and scene are the same throughout)
        assert same_key == (does == "reuse"), "entry %d" % i
        assert (total[i] > cap) == does.endswith("grows"), "entry %d: %d rows, tables of %d" % (i, total[i], cap)
        if total[i] > cap:
            cap = total[i] + total[i] // 8 + 1024                                # ensure_rows
    assert total[3] < total[2] and cases[3].culled.sum() > 0
    assert total[4] < total[3] and cases[4].rows.max() <= 512 < cases[2].rows.max()
    assert 3 * total[6] < cap

    mirt.shutdown()                       # every stream's RasterScratch starts empty, whatever the tests before this one rendered
    mirt.init(0)
    mirt.scene_upload(cases[0].tris, cases[0].culled)
    H, W = cases[0].H, cases[0].W
    shapes = {"xrgb": ((H, W), np.uint32), "rgb": ((H, W, 3), np.float32), "depth": ((H, W), np.float32), "index": ((H, W), np.int32)}
    planes = []
    try:
        for _ in range(len(cases) * in_flight):         # allocated first (an allocation waits for the device), so that the frames can queue
            planes.append({k: DeviceArray(shape, dtype, FILL) for k, (shape, dtype) in shapes.items()})
        mirt.set_frames_in_flight(in_flight)
        for i, c in enumerate(cases):
            if new_flags[i]:
                mirt.scene_set_culled(c.culled)
            for s in range(in_flight):
                d = planes[i * in_flight + s]
                mirt.rasterise_device(c.view(), c.lights, INDIRECT, 0, H, 0, d["xrgb"].ptr, W * 4, d["rgb"].ptr, d["depth"].ptr, d["index"].ptr)
        mirt.sync()
        for i, c in enumerate(cases):
            for s in range(in_flight):
                got = {k: a.read() for k, a in planes[i * in_flight + s].items()}
                assert_planes(got, c.ref, "entry %d (%s) on stream %d: " % (i, SIZING_SEQUENCE[i][2], s))
    finally:
        mirt.set_frames_in_flight(1)
        for d in planes:
            for a in d.values():
                a.free()


# ---- 5. lowered thresholds (the knobs are read once per process) ------------------------------------------------------------------

LOWERED = ["MIRT_RASTER_LDS_ROWS=40", "MIRT_RASTER_LDS_ROWS=0", "MIRT_RASTER_LDS_ROWS=40 MIRT_EDGE_SEGMENTS=2", "MIRT_EDGE_SEGMENTS=2",
           "MIRT_RASTER_SMALL=0 MIRT_RASTER_LDS_ROWS=40"]

LOWERED_CODE = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import test_gpu_raster_tall
test_gpu_raster_tall.lowered_child(%r)
print("ok")
"""


def lowered_child(knobs):
    """What a child process of test_lowered_thresholds runs under `knobs`: frames f-j whole, f and h in bands; a and c as well when
    only the prediction is spoilt (the 1024-thread LDS kernel at 2560 rows then falls back to the whole-chain walk)."""
    from mirt_oracle import Oracle
    oracle = Oracle()
    env = dict(k.split("=") for k in knobs.split())
    lds = int(env.get("MIRT_RASTER_LDS_ROWS", LDS_CAP))
    mirt.init(0)
    try:
        for name in "fghij":
            case = frame_case(oracle, name)
            if lds == 40:
                # both edge kernels in every frame; on f-h the chunked one walks three chunks
                _guard(case.rows, case.owned, 40, what="frame " + name)
                if name in "fgh":
                    _guard(case.rows, case.owned, 512, multi_chunk_above=40, what="frame " + name)
            elif name in "fgh":
                # 0: every triangle takes the chunked kernel, up to three chunks; default: the 1024-thread LDS kernel takes them all
                _guard(case.rows, case.owned, 512, multi_chunk_above=0 if lds == 0 else None, what="frame " + name)
            else:
                # i, j: no triangle above 512 rows.  0: the chunked kernel with one partial chunk for every triangle; default: the
                # 256-thread LDS kernel (200-row table) for every triangle, each chain with a spoilt prediction
                drawn = (case.rows >= 1) & (case.owned > 0)
                print("frame %s: %d owners, tallest triangle %d rows" % (name, int(drawn.sum()), int(case.rows.max())))
                assert drawn.any() and case.rows.max() <= CHUNK
            compare_planes(case)
        if lds == 40:
            # the hand-over between the kernels, from both sides: one owner of frame h has exactly 40 rows inside [0, 185), the last
            # height the LDS kernel takes (`rows > lds_rows` returns), and exactly 41 inside [0, 186), the first the chunked kernel
            # takes (`rows <= handled_rows` returns); the whole frame has another owner of exactly 41 rows
            case = frame_case(oracle, "h")
            assert ((case.rows == 41) & (case.owned > 0)).any(), "no owner of exactly 41 rows"
            for (y0, y1), exactly in zip(HANDOVER_BANDS_H, (40, 41)):
                rows, owned = guard_band_is_drawn(case, y0, y1)
                at = (rows == exactly) & (owned > 0)
                print("frame h band [%d, %d): %d owners of exactly %d rows, %s px; tallest %d rows" % (
                    y0, y1, int(at.sum()), exactly, owned[at].tolist(), int(rows.max())))
                assert at.any(), "no owner of exactly %d rows in band [%d, %d)" % (exactly, y0, y1)
                assert (rows > 40).any() and ((rows >= 1) & (rows <= 40)).any()          # both kernels have triangles in the band
            compare_bands(case, HANDOVER_BANDS_H)
        for name in "fh":
            case = frame_case(oracle, name)
            for (y0, y1) in BANDS_1300:
                rows, owned = guard_band_is_drawn(case, y0, y1)
                if lds == 40 and y1 - y0 > 40:
                    _guard(rows, owned, 40, multi_chunk_above=40, what="frame %s band [%d, %d)" % (name, y0, y1))
            compare_bands(case, BANDS_1300)
        if "MIRT_RASTER_LDS_ROWS" not in env:
            for name in "ac":
                case = frame_case(oracle, name)
                _guard(case.rows, case.owned, LDS_CAP, what="frame " + name)
                compare_planes(case)
                compare_bands(case, BANDS_2700)
    finally:
        mirt.shutdown()


@pytest.mark.parametrize("knobs", LOWERED)
def test_lowered_thresholds(knobs):
    """MIRT_RASTER_LDS_ROWS=40: both edge kernels on every frame, the chunked one with three chunks; =0: chunked only, read-back
    sizing for every scene; MIRT_EDGE_SEGMENTS=2: a spoilt prediction in every chain, so the whole-chain walk runs -- with 40-row
    tables (256 threads) and, alone, in the 1024-thread kernel up to the 2560-row cap; MIRT_RASTER_SMALL=0 sends the Cornell frames
    through the key buffer.  Each in a fresh child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = LOWERED_CODE % (os.path.join(root, "cpp-raytracer-rasterizer_amd"), os.path.join(root, "oracle"), os.path.join(root, "tests"), knobs)
    env = dict(os.environ)
    env.update(k.split("=") for k in knobs.split())
    mirt.shutdown()                      # the child process owns the GPU context for this test
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    finally:
        mirt.init(0)
    print(r.stdout)
    print("child under %s: %.1f s" % (knobs, time.time() - t0))
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
