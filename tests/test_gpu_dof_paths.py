"""The depth-of-field resolve (csrc/dof_kernel.hip) on each of its three kernels, bit for bit against oracle.dof over the oracle's own
render.  launch_dof picks the kernel from K, the frame size and the caller's pitch:

    k_dof_tile<8>   K == 8 with 32-bit byte offsets: the frame below 2^31 bytes and the surface span 4 (y1 - row_origin) pitch_words too
    k_dof_tile<0>   every other K up to 16, and K == 8 beyond those limits; its LDS tile grows with K, its centre tap sits at K / 2
    k_dof_direct    K = 17 .. 64, one thread per pixel, taps through dof_fetch

Tiles are 64 x 32 outputs, dealt over eight XCDs as t = (id & 7) * per + (id >> 3) with an early return for t >= tiles.  What each
test reaches is said in its docstring.  Besides the blurred surface the unblurred rgb and index planes are compared, and every test
asserts that the blur changed the picture.

The scene is the Cornell box plus soup(9, 400, 0.12).  The main shapes use camera (0, 0, -2), yaw 0.1, focal about H and focal
length 1.3, where each weight regime -- fd == 0 (a miss: centre weight 1), 0 < |fd| < 1 (both weights fractional) and |fd| >= 1 (every
tap 1 / K^2) -- covers at least 5 % of the interior pixels (about 12 / 60 / 28 %); `regimes` asserts it on the reference planes.  The
narrow frames use focal length 0.2: every off-centre weight is the full 1 / K^2, so a tap lost or gained always shows.

Narrow frames: the taps are addressed by flat index, so on a frame narrower than about K / 2 a tap column wraps by more than one
row, a band needs more halo than one row beyond its tap rows (capi/dof_plan.hpp), and one tile row is a run of pixels spanning
several frame rows."""
import ctypes as C

import numpy as np
import pytest

import mirt
from devbuf import DeviceArray, hip
from mirt_oracle import DEFAULT_LIGHT

pytestmark = pytest.mark.gpu

IND = (0.2, 0.2, 0.2)
FILL, FILLW = 0x5A, 0x5A5A5A5A                   # what every surface starts as (PutPixelSDL's words have a zero top byte: never this)
RENDERERS = ("rt", "raster")
NARROW = [(6, 120, 24), (4, 96, 16), (12, 160, 48), (3, 96, 12), (5, 120, 17)]     # (W, H, K): a tap column wraps by two rows or more


@pytest.fixture(scope="module", autouse=True)
def device():
    mirt.init(0)
    yield
    mirt.shutdown()


_tris, _refs, _wants = [], {}, {}


def scene():
    if not _tris:
        _tris.append(np.concatenate([mirt.scene_cornell(), mirt.scene_soup(9, 400, 0.12)]))
    return _tris[0]


def reference(oracle, renderer, W, H, narrow=False, focal=None, culled_for=None):
    """The oracle's render of one frame, computed once, shared and never changed: the view, the rasteriser's cull flags, the unblurred
    rgb / index (/ depth) planes and surface, and focalDistances.  culled_for: a reference whose cull flags to use instead of the view's own."""
    key = (renderer, W, H, narrow, focal, None if culled_for is None else id(culled_for))
    if key not in _refs:
        cam, FL = ((0.3, 0, -2), 0.2) if narrow else ((0, 0, -2), 1.3)
        if focal is None:
            focal = H / 2.0 if narrow else float(round(H * 12 / 13))
        rot = oracle.rot_from_yaw(0.1, 1.0)
        view = mirt.make_view(cam, rot, focal, W, H)
        if renderer == "rt":
            r = oracle.raytrace(scene(), cam, rot, focal, W, H, DEFAULT_LIGHT)
            # focalDistances as ClosestIntersection leaves them (raytracer.cpp:249), the zero-initialised global where no ray hit
            r["fd"] = np.where(r["index"] >= 0, r["dist"] - np.float32(FL), np.float32(0)).astype(np.float32)
            r["culled"] = None
        else:
            culled = mirt.cull(scene(), view, 3) if culled_for is None else culled_for["culled"]
            r = oracle.rasterise(scene(), culled, cam, rot, focal, W, H, DEFAULT_LIGHT, want=("rgb", "index", "xrgb", "depth", "fd"), focal_plane=FL)
            r["culled"] = culled
        r.update(renderer=renderer, view=view, W=W, H=H, FL=FL, key=key)
        _refs[key] = r
    return _refs[key]


def wanted(oracle, ref, K):
    """The blurred frame over a surface of FILLW: the ray tracer leaves the border alone, the rasteriser's becomes 0 (rasteriser.cpp:190)."""
    key = (ref["key"], K)
    if key not in _wants:
        W, H = ref["W"], ref["H"]
        want = oracle.dof(ref["rgb"], ref["fd"], K, clear_border=ref["renderer"] == "raster", xrgb=np.full((H, W), FILLW, np.uint32))
        border = np.ones((H, W), bool)
        border[1:-1, 1:-1] = False
        assert (want[border] == (0 if ref["renderer"] == "raster" else FILLW)).all()
        assert not np.array_equal(want[1:-1, 1:-1], ref["xrgb"][1:-1, 1:-1]), "the blur changed nothing"
        _wants[key] = want
    return _wants[key]


def regimes(ref):
    a = np.abs(ref["fd"][1:-1, 1:-1])
    for name, part in (("fd == 0", a == 0), ("0 < |fd| < 1", (a > 0) & (a < 1)), ("|fd| >= 1", a >= 1)):
        assert part.mean() >= 0.05, "%s covers %.1f %% of the interior of %dx%d" % (name, 100 * part.mean(), ref["W"], ref["H"])


def upload(ref):
    if ref["renderer"] == "rt":
        mirt.scene_upload(scene())
    else:
        mirt.scene_upload(scene(), ref["culled"])


def render(ref, y0, y1, row_origin, ptr, pitch_bytes, mode=mirt.RT_AUTO, planes=None):
    """One device call; planes: the caller's rgb / index (/ depth) DeviceArrays, full-frame."""
    p = planes or {}
    ptr_of = lambda name: p[name].ptr if name in p else None
    if ref["renderer"] == "rt":
        mirt.raytrace_device(ref["view"], DEFAULT_LIGHT, IND, mode, y0, y1, row_origin, ptr, pitch_bytes, ptr_of("rgb"), ptr_of("index"))
    else:
        mirt.rasterise_device(ref["view"], DEFAULT_LIGHT, IND, y0, y1, row_origin, ptr, pitch_bytes, ptr_of("rgb"), ptr_of("depth"), ptr_of("index"))


def differing(got, want):
    return "%d of %d words differ" % (int((got != want).sum()), want.size)


def full_frame(oracle, ref, K, mode=mirt.RT_AUTO):
    """One call for the whole frame into a surface of FILLW with the caller's planes; everything against the oracle."""
    W, H = ref["W"], ref["H"]
    want = wanted(oracle, ref, K)
    upload(ref)
    mirt.set_depth_of_field(K, ref["FL"])
    try:
        with DeviceArray((H, W), np.uint32, FILL) as surf, DeviceArray((H, W, 3), np.float32) as rgb, DeviceArray((H, W), np.int32) as index, \
                DeviceArray((H, W), np.float32) as depth:
            planes = {"rgb": rgb, "index": index}
            if ref["renderer"] == "raster":
                planes["depth"] = depth
            render(ref, 0, H, 0, surf.ptr, W * 4, mode, planes)
            got, got_rgb, got_index, got_depth = surf.read(), rgb.read(), index.read(), depth.read()
    finally:
        mirt.set_depth_of_field(0)
    what = "%s %dx%d K %d" % (ref["renderer"], W, H, K)
    assert np.array_equal(got_index, ref["index"]), what
    assert np.array_equal(got_rgb.view(np.uint32), ref["rgb"].view(np.uint32)), what          # the unblurred pixelColours
    if ref["renderer"] == "raster":
        assert np.array_equal(got_depth.view(np.uint32), ref["depth"].view(np.uint32)), what
    assert np.array_equal(got, want), "%s: %s" % (what, differing(got, want))


def banded(oracle, ref, K, bands):
    """The bands into one full-frame surface (row_origin 0)."""
    W, H = ref["W"], ref["H"]
    want = wanted(oracle, ref, K)
    upload(ref)
    mirt.set_depth_of_field(K, ref["FL"])
    try:
        with DeviceArray((H, W), np.uint32, FILL) as surf:
            for y0, y1 in bands:
                render(ref, y0, y1, 0, surf.ptr, W * 4)
            got = surf.read()
    finally:
        mirt.set_depth_of_field(0)
    rows = [y for y in range(H) if (got[y] != want[y]).any()]
    assert np.array_equal(got, want), "%s %dx%d K %d, bands %s: %s, in rows %s" % (ref["renderer"], W, H, K, bands, differing(got, want), rows)


# ---- a. every kernel size that changes a code path, full frame ----

@pytest.mark.parametrize("renderer", RENDERERS)
@pytest.mark.parametrize("K", [2, 3, 4, 7, 8, 9, 15, 16, 17, 18, 31, 32, 63, 64])
def test_every_kernel_size(oracle, renderer, K):
    """129x65: 3 x 3 = 9 tiles, one more than the eight-way deal (per = 2, sixteen workgroups, seven of them leave at once), the last
    tile column 1 pixel wide and the last tile row 1 pixel high.  K == 8: k_dof_tile<8>; other K <= 16: k_dof_tile<0>, odd and even K
    (the centre tap's index), K = 16 its largest LDS tile; K >= 17: k_dof_direct, one workgroup per frame row."""
    ref = reference(oracle, renderer, 129, 65)
    regimes(ref)
    full_frame(oracle, ref, K)


@pytest.mark.parametrize("renderer", RENDERERS)
@pytest.mark.parametrize("W,H", [(63, 31), (64, 32), (65, 33), (128, 64)])
def test_frames_on_and_beside_tile_edges(oracle, renderer, W, H):
    """1, 1, 4 and 4 tiles, exact multiples of the 64 x 32 tile among them, on k_dof_tile<8> (K 8), k_dof_tile<0> (K 16) and
    k_dof_direct (K 17): the switch between the last two."""
    ref = reference(oracle, renderer, W, H)
    regimes(ref)
    for K in (8, 16, 17):
        full_frame(oracle, ref, K)


def test_binned_ray_tracer_with_the_direct_kernel(oracle):
    """RT_BINNED in front of k_dof_direct (K 17): the binned trace kernel stores fd and rgb for the blur."""
    ref = reference(oracle, "rt", 129, 65)
    full_frame(oracle, ref, 17, mode=mirt.RT_BINNED)


# ---- b. bands cut on tile rows and beside them ----

BANDS = [(0, 1), (1, 32), (32, 33), (33, 64), (64, 65)]


@pytest.mark.parametrize("renderer", RENDERERS)
@pytest.mark.parametrize("K", [8, 13, 16, 17, 40])
def test_bands_on_tile_rows(oracle, renderer, K):
    """Bands of 1, 31, 1, 31 and 1 rows of 129x65, each with its own halo, tile grid (y0 is the tiles' origin) and store guard:
    once into one full-frame surface, once into a buffer per band that starts at the band's first row (row_origin = y0) with a
    pitch of W + 7 words -- words beyond W and rows beyond the band keep what they held.  k_dof_tile<8> (K 8), k_dof_tile<0> (13, 16),
    k_dof_direct (17, 40)."""
    ref = reference(oracle, renderer, 129, 65)
    regimes(ref)
    W, H, pitch_words = 129, 65, 129 + 7
    want = wanted(oracle, ref, K)
    banded(oracle, ref, K, BANDS)
    upload(ref)
    mirt.set_depth_of_field(K, ref["FL"])
    try:
        for y0, y1 in BANDS:
            rows = y1 - y0
            with DeviceArray((rows + 2, pitch_words), np.uint32, FILL) as surf:            # (two rows of slack behind the band)
                render(ref, y0, y1, y0, surf.ptr, pitch_words * 4)
                got = surf.read()
            what = "%s K %d band [%d, %d)" % (renderer, K, y0, y1)
            assert np.array_equal(got[:rows, :W], want[y0:y1]), "%s: %s" % (what, differing(got[:rows, :W], want[y0:y1]))
            assert (got[:rows, W:] == FILLW).all() and (got[rows:] == FILLW).all(), what
    finally:
        mirt.set_depth_of_field(0)


# ---- c. narrow frames ----

def narrow_bands(H):
    return [(0, H // 2), (H // 2, H // 2 + 1), (H // 2 + 1, H)]


@pytest.mark.parametrize("renderer", RENDERERS)
@pytest.mark.parametrize("W,H,K", NARROW)
def test_narrow_frame_in_bands(oracle, renderer, W, H, K):
    """A tap column of these frames wraps by two rows or more, so a band's farthest tap lies beyond one row past its tap rows: the
    halo is dof_halo_rows (capi/dof_plan.hpp).  With a halo of max(-zlo, zhi - 1) + 1 rows these differed from the frame blurred
    whole in the rows next to a cut -- ray tracer: 6, 4, 5, 2 and 3 words in the order of NARROW, as tests/test_dof_plan_host.py
    finds with the oracle alone; rasteriser: 2, 0, 5, 0 and 1 (its picture is another: the taps lost on the 4- and 3-wide frames
    did not change a word).  k_dof_tile<0> (K 12, 16), k_dof_direct (17, 24, 48)."""
    banded(oracle, reference(oracle, renderer, W, H, narrow=True), K, narrow_bands(H))


@pytest.mark.parametrize("renderer", RENDERERS)
@pytest.mark.parametrize("W,H,K", NARROW)
def test_narrow_frame_in_one_call(oracle, renderer, W, H, K):
    full_frame(oracle, reference(oracle, renderer, W, H, narrow=True), K)


@pytest.mark.parametrize("renderer", RENDERERS)
@pytest.mark.parametrize("W", [3, 4, 5, 6, 9])
def test_a_tile_row_spans_many_frame_rows(oracle, renderer, W):
    """H = 40, one call: a tile row of 64 + K - 1 pixels is a run through up to 27 frame rows of a frame 3 wide, the direct kernel's
    taps wrap by up to 11 rows, and most of a tile lies beyond x = W.  k_dof_tile<8> (K 8), k_dof_tile<0> (16), k_dof_direct (17, 64)."""
    ref = reference(oracle, renderer, W, 40, narrow=True)
    for K in (8, 16, 17, 64):
        full_frame(oracle, ref, K)


# ---- d. the 32-bit boundary of k_dof_tile<8> ----

class Pitched:
    """A surface of `rows` rows `pitch` bytes apart, of which only the first `words` words of each row are ever filled or read."""

    def __init__(self, rows, pitch, words):
        h = hip()
        h.hipMemset2D.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t]
        h.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
        self.rows, self.pitch, self.words, self.ptr = rows, pitch, words, C.c_void_p()
        assert h.hipMalloc(C.byref(self.ptr), rows * pitch) == 0
        self.fill()

    def fill(self):
        mirt.sync()
        assert hip().hipMemset2D(self.ptr, self.pitch, FILL, self.words * 4, self.rows) == 0
        assert hip().hipDeviceSynchronize() == 0

    def read(self):
        mirt.sync()
        out = np.zeros((self.rows, self.words), np.uint32)
        assert hip().hipMemcpy2D(out.ctypes.data_as(C.c_void_p), self.words * 4, self.ptr, self.pitch, self.words * 4, self.rows, 2) == 0
        return out

    def free(self):
        hip().hipFree(self.ptr)


@pytest.mark.parametrize("renderer", RENDERERS)
def test_surface_span_at_two_to_the_31_bytes(oracle, renderer):
    """K = 8 on a 70x6 frame whose rows lie 2^29 bytes apart (3 GB of address space, 6 x 78 words of it touched).  k_dof_tile<8>
    describes the surface up to y1 as a buffer of 4 (y1 - row_origin) pitch_words bytes, a signed 32-bit size: band [0, 3) spans
    3 * 2^29 < 2^31 bytes and takes it, band [3, 6) spans 6 * 2^29 and goes to k_dof_tile<0> -- the only way K = 8 reaches that
    kernel at a small shape.  Were the test in launch_dof off, k_dof_tile<8> would get a negative size and drop or misplace its
    stores.  Then the whole frame in one call (k_dof_tile<0>) and into a surface of its own width (k_dof_tile<8>): the two kernels
    agree on the same picture."""
    W, H, K, pitch = 70, 6, 8, 1 << 29
    ref = reference(oracle, renderer, W, H, focal=20.0)
    want = wanted(oracle, ref, K)
    upload(ref)
    surf = Pitched(H, pitch, W + 8)
    mirt.set_depth_of_field(K, ref["FL"])
    try:
        assert 4 * 3 * (pitch // 4) < 2 ** 31 <= 4 * 6 * (pitch // 4)
        for y0, y1 in [(0, 3), (3, 6)]:
            render(ref, y0, y1, 0, surf.ptr, pitch)
        got = surf.read()
        assert np.array_equal(got[:, :W], want), "in two bands: %s" % differing(got[:, :W], want)
        assert (got[:, W:] == FILLW).all()
        surf.fill()
        render(ref, 0, H, 0, surf.ptr, pitch)
        got = surf.read()
        assert np.array_equal(got[:, :W], want), "k_dof_tile<0>: %s" % differing(got[:, :W], want)
        assert (got[:, W:] == FILLW).all()
        with DeviceArray((H, W), np.uint32, FILL) as small:
            render(ref, 0, H, 0, small.ptr, W * 4)
            got = small.read()
        assert np.array_equal(got, want), "k_dof_tile<8>: %s" % differing(got, want)
    finally:
        mirt.set_depth_of_field(0)
        surf.free()


# ---- e. two frames in flight on the direct kernel ----

def test_two_frames_in_flight_with_a_large_kernel(oracle):
    """K = 20 (k_dof_direct) with two frames in flight, two frame sizes and both renderers in turn: each stream's own pixelColours /
    focalDistances planes are resized from call to call while the other stream's frame is still being blurred."""
    K = 20
    a_rt, b_rt = reference(oracle, "rt", 129, 65), reference(oracle, "rt", 70, 40)
    a_ra = reference(oracle, "raster", 129, 65)
    b_ra = reference(oracle, "raster", 70, 40, culled_for=a_ra)                  # (one set of cull flags is uploaded at a time)
    frames = [a_rt, b_ra, b_rt, a_ra]
    wants = [wanted(oracle, f, K) for f in frames]
    mirt.scene_upload(scene(), a_ra["culled"])
    surf = [DeviceArray((f["H"], f["W"]), np.uint32, FILL) for f in frames]
    mirt.set_depth_of_field(K, 1.3)
    try:
        mirt.set_frames_in_flight(2)
        for _ in range(10):
            for f, s in zip(frames, surf):
                render(f, 0, f["H"], 0, s.ptr, f["W"] * 4)
        for i, (s, want) in enumerate(zip(surf, wants)):
            got = s.read()
            assert np.array_equal(got, want), "surface %d: %s" % (i, differing(got, want))
    finally:
        mirt.set_frames_in_flight(1)
        mirt.set_depth_of_field(0)
        for s in surf:
            s.free()
