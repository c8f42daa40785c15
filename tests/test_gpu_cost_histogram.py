"""The cost histogram of a binned ray-traced frame (k_prep_select, csrc/rt_binned.hip) -- what the weighted partition of a sharded
frame is derived from on every rank without any exchange.

Its output only moves band boundaries, so no frame parity test can see an error in it.  Here:
* it must not depend on the rows a call renders (bit for bit: the whole frame, the top tile row, a band whose edges are not
  multiples of 8, the bottom band) -- every rank renders other rows and must still file the same numbers;
* it must lie inside a float64 bracket of its definition: make_origin_row (rt_common.hpp), the classification and box of
  frame_may_see (rt_binned.hpp), the clamp to the grid and the sums per coarse tile row (k_prep_select).  The kernel uses the
  hardware's one-ulp rcp / rsq, so the reference bounds each triangle's box from both sides by the rounding its float32
  arithmetic can carry, and lets a triangle whose classification lies within that rounding of a threshold add [0, grown box];
* mirt_cost_histogram must return the histogram of the frame just rendered, whichever stream it ran on.
The reference itself is checked without a GPU: a float32 restatement of the kernel lies inside the bracket, and a histogram
shifted by one coarse row or with every box one bin wider does not.
"""
import numpy as np
import pytest

import mirt

EPS = 2.0 ** -23           # one ulp of a float32 in [1, 2)
SEL_HIST_MAX = 256


def hist_shift_for(tile_rows):
    sh = 0
    while ((tile_rows - 1) >> sh) + 1 > SEL_HIST_MAX:
        sh += 1
    return sh


def camera_frame(pos, rot9, focal, W, H, aa):
    """make_camera_frame (capi/rt_frame.cpp): the fields frame_may_see reads, as the float32 values the kernel gets."""
    f32 = np.float32
    R = np.asarray(rot9, f32)
    hw, hh = f32(W) / f32(2), f32(H) / f32(2)
    dm = f32(0)
    for i in range(3):
        dm = max(dm, f32(f32(abs(R[i]) * (hw + f32(1))) + f32(abs(R[3 + i]) * (hh + f32(1)))) + f32(abs(R[6 + i]) * abs(f32(focal))))
    M = [float(x) for x in R]
    MM = lambda c, r: M[c * 3 + r]
    det = MM(0, 0) * (MM(1, 1) * MM(2, 2) - MM(2, 1) * MM(1, 2)) - MM(1, 0) * (MM(0, 1) * MM(2, 2) - MM(2, 1) * MM(0, 2)) + \
        MM(2, 0) * (MM(0, 1) * MM(1, 2) - MM(1, 1) * MM(0, 2))
    inv = [(MM(1, 1) * MM(2, 2) - MM(2, 1) * MM(1, 2)) / det, -(MM(1, 0) * MM(2, 2) - MM(2, 0) * MM(1, 2)) / det, (MM(1, 0) * MM(2, 1) - MM(2, 0) * MM(1, 1)) / det,
           -(MM(0, 1) * MM(2, 2) - MM(2, 1) * MM(0, 2)) / det, (MM(0, 0) * MM(2, 2) - MM(2, 0) * MM(0, 2)) / det, -(MM(0, 0) * MM(2, 1) - MM(2, 0) * MM(0, 1)) / det,
           (MM(0, 1) * MM(1, 2) - MM(1, 1) * MM(0, 2)) / det, -(MM(0, 0) * MM(1, 2) - MM(1, 0) * MM(0, 2)) / det, (MM(0, 0) * MM(1, 1) - MM(1, 0) * MM(0, 1)) / det]
    rwd = [-inv[6 + i] / float(f32(focal)) for i in range(3)]
    as32 = lambda v: np.array(v, np.float64).astype(f32).astype(np.float64)
    return {
        "S": np.asarray(pos, f32).astype(np.float64),
        "Pu": (-R[0:3]).astype(np.float64), "Pv": (-R[3:6]).astype(np.float64),
        "rw": as32(rwd), "ru": as32([-inv[i] + float(hw) * rwd[i] for i in range(3)]), "rv": as32([-inv[3 + i] + float(hh) * rwd[i] for i in range(3)]),
        "dmax": float(dm), "du": 8.0, "dv": 8.0, "ulo": 0.0, "vlo": 0.0,
        "pad_lo": -0.5 if aa > 1 else 0.0, "pad_hi": -0.5 if aa > 1 else -1.0,
        "nbu": (W + 7) // 8, "nbv": (H + 7) // 8,
    }


def _boxes(tris, fr, xp):
    """make_origin_row + frame_may_see per triangle, evaluated in `xp` arithmetic in the kernel's order of operations (float64: the
    definition; float32: what the kernel computes, but with correctly rounded reciprocals and square roots where it uses the
    hardware's one-ulp rcp / rsq).  Returns the box in bins (lou, hiu, lov, hiv), whether it is valid, and the intermediates the
    tolerances below are taken from."""
    f = lambda a: np.asarray(a, xp)
    t = f(tris[:, 0:9]).reshape(-1, 3, 3)
    v0, v1, v2 = t[:, 0], t[:, 1], t[:, 2]
    S = f(fr["S"])
    e1, e2, b = v1 - v0, v2 - v0, S - v0
    cross = lambda p, q: np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1)
    e1e2, be2, e1b = cross(e1, e2), cross(b, e2), cross(e1, b)
    nbv = (e1e2[:, 0] * b[:, 0] + e1e2[:, 1] * b[:, 1]) + e1e2[:, 2] * b[:, 2]
    rw, ru, rv = f(fr["rw"]), f(fr["ru"]), f(fr["rv"])
    g = S[None, None, :] - t                                        # (n, 3 vertices, 3)
    dot = lambda r: (r[0] * g[..., 0] + r[1] * g[..., 1]) + r[2] * g[..., 2]
    adot = lambda r: (np.abs(r[0] * g[..., 0]) + np.abs(r[1] * g[..., 1])) + np.abs(r[2] * g[..., 2])
    w, wm = dot(rw), adot(rw)
    un, vn, um, vm = dot(ru), dot(rv), adot(ru), adot(rv)
    c256 = xp(0.00390625)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iw = xp(1) / w                                              # (the kernel multiplies by reciprocals: rcp, rsq)
        us, vs = un * iw, vn * iw
        aiw = np.abs(iw)
        k21 = xp(4.76837158203125e-07)
        pad = (k21 * ((um + np.abs(us) * wm) * aiw + (vm + np.abs(vs) * wm) * aiw) + k21 * (np.abs(us) + np.abs(vs))).max(1)
        Pu, Pv = f(fr["Pu"]), f(fr["Pv"])
        rows = [e1e2, be2, e1b]
        cu = [(r[:, 0] * Pu[0] + r[:, 1] * Pu[1]) + r[:, 2] * Pu[2] for r in rows]
        cv = [(r[:, 0] * Pv[0] + r[:, 1] * Pv[1]) + r[:, 2] * Pv[2] for r in rows]
        mg = [xp(7.62939453125e-06) * (((np.abs(r[:, 0]) + np.abs(r[:, 1])) + np.abs(r[:, 2])) * xp(fr["dmax"])) + xp(9.5367431640625e-07) for r in rows]
        scu, scv = (cu[0] - cu[1]) - cu[2], (cv[0] - cv[1]) - cv[2]
        sm = xp(1.25) * ((mg[0] + mg[1]) + mg[2])
        dp = mg[1] * (xp(1) / np.sqrt(cu[1] * cu[1] + cv[1] * cv[1]))
        dq = mg[2] * (xp(1) / np.sqrt(cu[2] * cu[2] + cv[2] * cv[2]))
        ds = sm * (xp(1) / np.sqrt(scu * scu + scv * scv))
        d = np.maximum(np.maximum(dp, dq), ds) * xp(1.0000019073486328125) + pad
        u0, u1, v0_, v1_ = us.min(1), us.max(1), vs.min(1), vs.max(1)
        extu, extv = u1 - u0, v1_ - v0_
        ax, ay, bx, by = us[:, 1] - us[:, 0], vs[:, 1] - vs[:, 0], us[:, 2] - us[:, 0], vs[:, 2] - vs[:, 0]
        t1, t2 = ax * by, ay * bx
        area_lo = np.abs(t1 - t2) - xp(4) * pad * (extu + extv) - k21 * (np.abs(t1) + np.abs(t2))
        disp = (xp(2.5) * d) * (extu * extu + extv * extv) * (xp(1) / area_lo) * xp(1.0000019073486328125)
        slack = xp(2) * pad + xp(1.0e-6) * np.maximum(extu, extv)
        bu0, bu1, bv0, bv1 = u0 - disp - slack, u1 + disp + slack, v0_ - disp - slack, v1_ + disp + slack
        idu, idv = xp(1) / xp(fr["du"]), xp(1) / xp(fr["dv"])
        lou = (bu0 - xp(fr["ulo"]) - xp(fr["pad_hi"])) * idu
        hiu = (bu1 - xp(fr["ulo"]) - xp(fr["pad_lo"])) * idu
        lov = (bv0 - xp(fr["vlo"]) - xp(fr["pad_hi"])) * idv
        hiv = (bv1 - xp(fr["vlo"]) - xp(fr["pad_lo"])) * idv
        k17 = xp(7.62939453125e-06)
        lou, hiu = lou - k17 * (1 + np.abs(lou)), hiu + k17 * (1 + np.abs(hiu))
        lov, hiv = lov - k17 * (1 + np.abs(lov)), hiv + k17 * (1 + np.abs(hiv))
        big = xp(1.0e30)
        finite_box = (bu0 > -big) & (bu1 < big) & (bv0 > -big) & (bv1 < big)
    box = [np.asarray(x, np.float64) for x in (lou, hiu, lov, hiv)]
    tests = {"nbv": np.abs(nbv) >= xp(1.6940658945086007e-21), "front": (w > c256 * wm).all(1), "area": area_lo > 0, "finite": finite_box}
    boxed = tests["nbv"] & tests["front"] & tests["area"] & tests["finite"]
    mid = {k: np.asarray(v, np.float64) for k, v in dict(nbv=nbv, w=w, wm=wm, area_lo=area_lo, t12=np.abs(t1) + np.abs(t2), disp=disp, slack=slack,
                                                        uv=np.abs(u0) + np.abs(u1) + np.abs(v0_) + np.abs(v1_), vmag=(np.abs(us) + np.abs(vs)).max(1),
                                                        diffs=np.abs(ax) + np.abs(ay) + np.abs(bx) + np.abs(by), ext=extu + extv, ext2=extu * extu + extv * extv, edge=np.maximum(np.maximum(np.abs(bu0), np.abs(bu1)), np.maximum(np.abs(bv0), np.abs(bv1)))).items()}
    return box, boxed, tests, mid


def _accumulate(lou, hiu, lov, hiv, use, nbu, nbv, shift):
    """k_prep_select's sums: the box's bins clamped to the grid, width times rows per coarse tile row (int64, no wrap)."""
    hist_rows = ((nbv - 1) >> shift) + 1
    out = np.zeros(hist_rows, np.int64)
    with np.errstate(invalid="ignore"):
        flo_u = np.maximum(np.ceil(lou) - 1, 0)
        fhi_u = np.minimum(np.floor(hiu), nbu - 1)
        flo_v = np.maximum(np.ceil(lov) - 1, 0)
        fhi_v = np.minimum(np.floor(hiv), nbv - 1)
        ok = use & (flo_u <= fhi_u) & (flo_v <= fhi_v)
    wi = (fhi_u[ok] - flo_u[ok] + 1).astype(np.int64)
    ja, jb = flo_v[ok].astype(np.int64), fhi_v[ok].astype(np.int64)
    for cr in range(hist_rows):
        lo = np.maximum(ja, cr << shift)
        hi = np.minimum(jb, ((cr + 1) << shift) - 1)
        out[cr] = int((wi * np.maximum(hi - lo + 1, 0)).sum())
    return out


def reference_bracket(tris, fr, tol=16.0):
    """(lo, hi, mid, detail): the bracket of the kernel's histogram, and the plain float64 histogram (mid).

    Per triangle the definition is evaluated in float64 and in float32 (the kernel's own precision and order of operations).  The
    kernel differs from the float32 evaluation by its one-ulp rcp / rsq only: a few ulps of every projected vertex -- of its
    MAGNITUDE, which far from the frame's centre is much more than of the triangle's extent --, margin distance and displacement.
    `tol` ulps of each quantity that feeds a box edge widen the box from both evaluations (the displacement's relative error grows
    as its area bound cancels): the shrunk box goes to lo, the grown one to hi.  A triangle whose
    evaluations disagree on a test, or whose value lies within that tolerance of a threshold (the determinant test, the 1/256
    front rule, area_lo > 0, the 1e30 guard), adds [0, grown box]; if its area bound may vanish, the grown box is the whole grid."""
    nbu, nbv = fr["nbu"], fr["nbv"]
    shift = hist_shift_for(nbv)
    box64, boxed64, t64, m = _boxes(tris, fr, np.float64)
    box32, boxed32, t32, m32 = _boxes(tris, fr, np.float32)
    u = tol * EPS
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        area_err = u * m["t12"]
        rel_disp = u + area_err / np.abs(m["area_lo"])
        e_box = u * (m["uv"] + m["slack"] + 4 * m["edge"]) + m["disp"] * rel_disp
        e_u = e_box / fr["du"] + u * (1 + np.abs(box64[0]) + np.abs(box64[1]))
        e_v = e_box / fr["dv"] + u * (1 + np.abs(box64[2]) + np.abs(box64[3]))
        near = {"nbv": np.abs(np.abs(m["nbv"]) - 1.6940658945086007e-21) <= u * np.abs(m["nbv"]),
                "front": (np.abs(np.abs(m["w"]) - 0.00390625 * m["wm"]) <= u * m["wm"]).any(1),
                "area": np.abs(m["area_lo"]) <= area_err,
                "finite": np.abs(m["edge"] - 1e30) <= 1e27}
    certain = np.ones(len(tris), bool)
    possible = np.ones(len(tris), bool)
    for k in t64:
        certain &= t64[k] & t32[k] & ~near[k]
        possible &= t64[k] | t32[k] | near[k]
    unbounded = possible & ~(np.minimum(m["area_lo"], m32["area_lo"]) - area_err > 0)
    lo_box = (np.maximum(box64[0], box32[0]) + e_u, np.minimum(box64[1], box32[1]) - e_u,
              np.maximum(box64[2], box32[2]) + e_v, np.minimum(box64[3], box32[3]) - e_v)
    hi_box = (np.minimum(box64[0], box32[0]) - e_u, np.maximum(box64[1], box32[1]) + e_u,
              np.minimum(box64[2], box32[2]) - e_v, np.maximum(box64[3], box32[3]) + e_v)
    lo = _accumulate(*lo_box, certain, nbu, nbv, shift)
    hi = _accumulate(*hi_box, possible & ~unbounded, nbu, nbv, shift)
    inf = np.full(len(tris), np.inf)
    hi += _accumulate(-inf, inf, -inf, inf, unbounded, nbu, nbv, shift)
    mid = _accumulate(*box64, boxed64, nbu, nbv, shift)
    detail = {"boxed": int(boxed64.sum()), "certain": int(certain.sum()), "on_threshold": int((possible & ~certain).sum()), "unbounded": int(unbounded.sum())}
    return lo, hi, mid, detail


def kernel_in_float32(tris, fr):
    """The kernel's histogram as the float32 evaluation computes it (correctly rounded reciprocals and square roots)."""
    box, boxed, _, _ = _boxes(tris, fr, np.float32)
    return _accumulate(*box, boxed, fr["nbu"], fr["nbv"], hist_shift_for(fr["nbv"]))


# ---- scenes and views ---------------------------------------------------------------------------------------------------

def _orbit_view(yaw, dist, W, H, focal, height=0.0):
    """A camera `dist` from the origin looking at it (forward = third column of the rotation: (-sin yaw, 0, cos yaw))."""
    pos = (dist * np.sin(yaw), height, -dist * np.cos(yaw))
    return mirt.make_view(pos, mirt.rot_from_yaw(yaw, 1.0), focal, W, H)


def _soup():
    return mirt.scene_soup(11, 3000, 0.08)


# name: (scene, view args, aa, bands) -- bands None: the whole frame, the top tile row, an unaligned band, the bottom band
CASES = {
    "soup_front": ("soup", (0.1, 2.6, 320, 240, 200.0), 1, None),
    "camera_inside": ("soup", (0.3, 0.05, 320, 240, 160.0), 1, None),
    "cornell_walls_clamped": ("cornell", (0.05, 2.0, 320, 240, 420.0), 1, None),
    "rotated_past_90": ("soup", (2.2, 2.6, 320, 240, 200.0), 1, None),
    "height_not_multiple_of_8": ("soup", (-0.2, 2.6, 200, 131, 150.0), 1, None),
    "one_tile_row": ("soup", (0.0, 2.6, 320, 6, 200.0), 1, None),
    "8k_shift_2": ("soup", (0.15, 2.6, 7680, 4320, 3000.0), 1, "thin"),
    "2056_rows_shift_1": ("soup", (0.0, 2.6, 1200, 2056, 1100.0), 1, "thin"),
    "aa3": ("soup", (0.1, 2.6, 320, 240, 200.0), 3, None),
}


def _bands(H, kind):
    if kind == "thin":                       # thin bands only: the histogram still covers the whole frame
        m = (H // 2) // 8 * 8
        return [(0, 8), (m + 3, m + 21), (H - 8, H)]
    bands = [(0, H), (0, min(8, H))]
    if H > 16:
        bands.append((H // 3 + 3, H // 3 + 3 + max(5, H // 5) | 1))     # neither edge a multiple of 8
    bands.append(((H - 1) // 8 * 8 if H > 8 else 0, H))
    return bands


def _scene(name):
    return mirt.scene_cornell() if name == "cornell" else _soup()


def _case_frame(case):
    scene, (yaw, dist, W, H, focal), aa, bands = CASES[case]
    view = _orbit_view(yaw, dist, W, H, focal, 0.05 if dist < 1 else 0.0)
    return scene, view, aa, bands


def _frame_desc(view, aa):
    return camera_frame(list(view.pos), list(view.rot), view.focal, view.width, view.height, aa)


# ---- without a GPU: the reference has teeth ----------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["soup_front", "camera_inside", "rotated_past_90", "height_not_multiple_of_8", "aa3"])
def test_reference_bracket_is_tight_and_holds_the_float32_kernel(case):
    """The float32 restatement of the kernel lies inside the bracket; the bracket is narrow (<= 1 %% of the histogram); the
    histogram shifted by one coarse row and the one with every box one bin wider both fall outside it."""
    scene, view, aa, _ = _case_frame(case)
    tris = mirt.scene_soup(11, 3000, 0.08) if scene == "soup" else None
    fr = _frame_desc(view, aa)
    lo, hi, mid, detail = reference_bracket(tris, fr)
    k32 = kernel_in_float32(tris, fr)
    assert mid.sum() > 0 and detail["boxed"] > 100, detail
    assert (lo <= mid).all() and (mid <= hi).all(), (detail, lo, mid, hi)
    assert (lo <= k32).all() and (k32 <= hi).all(), (detail, np.nonzero((k32 < lo) | (k32 > hi)))
    assert (hi - lo).sum() <= 0.01 * k32.sum(), (detail, int((hi - lo).sum()), int(k32.sum()))
    _assert_teeth(tris, fr, lo, hi, mid)


def _assert_teeth(tris, fr, lo, hi, mid):
    if len(mid) > 1:
        shifted = np.roll(mid, 1)
        assert ((shifted < lo) | (shifted > hi)).any(), "a histogram one coarse row off passes the bracket"
    (lou, hiu, lov, hiv), boxed, _, _ = _boxes(tris, fr, np.float64)
    wider = _accumulate(lou, hiu + 1.0, lov, hiv, boxed, fr["nbu"], fr["nbv"], hist_shift_for(fr["nbv"]))
    assert ((wider < lo) | (wider > hi)).any(), "a histogram with boxes one bin wider passes the bracket"


# ---- on the GPU ----------------------------------------------------------------------------------------------------------

LIGHT = np.array([[0.0, -0.5, -0.7, 1, 1, 1, 14]], np.float32)


@pytest.fixture
def lib():
    mirt.init(0)
    try:
        yield mirt
    finally:
        mirt.shutdown()


def _gpu_histogram(view, y0, y1, buf):
    """Rows [y0, y1) of the view, binned, and the histogram that frame left."""
    mirt.raytrace_device(view, LIGHT, (0.2, 0.2, 0.2), mirt.RT_BINNED, y0, y1, y0, buf.ptr, view.width * 4)
    h, shift = mirt.cost_histogram()
    assert h is not None, "no cost histogram after a binned frame"
    return h.astype(np.int64), shift


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_cost_histogram_against_float64_reference(lib, case):
    from devbuf import DeviceArray
    scene, view, aa, kind = _case_frame(case)
    tris = _scene(scene)
    mirt.scene_upload(tris)
    mirt.set_antialiasing(aa)
    mirt.set_cost_histogram(True)
    W, H = view.width, view.height
    bands = _bands(H, kind)
    rows = max(b - a for a, b in bands)
    with DeviceArray((rows, W), np.uint32) as buf:
        got = [(band,) + _gpu_histogram(view, band[0], band[1], buf) for band in bands]
    fr = _frame_desc(view, aa)
    want_rows = ((fr["nbv"] - 1) >> hist_shift_for(fr["nbv"])) + 1
    # independent of the rows rendered: bit for bit
    (band0, h0, s0) = got[0]
    for band, h, s in got[1:]:
        assert s == s0 and np.array_equal(h, h0), (case, band0, band, np.nonzero(h != h0))
    assert s0 == hist_shift_for(fr["nbv"]) and len(h0) == want_rows, (s0, len(h0), want_rows)
    if kind == "thin":
        assert s0 >= 1
    # inside the bracket of the float64 definition
    lo, hi, mid, detail = reference_bracket(tris, fr)
    bad = np.nonzero((h0 < lo) | (h0 > hi))[0]
    assert len(bad) == 0, (case, detail, [(int(i), int(lo[i]), int(h0[i]), int(hi[i])) for i in bad[:8]])
    assert h0.sum() > 0
    assert (hi - lo).sum() <= 0.01 * h0.sum(), (case, detail, int((hi - lo).sum()), int(h0.sum()))
    _assert_teeth(tris, fr, lo, hi, mid)


@pytest.mark.gpu
@pytest.mark.parametrize("flight", [2, 3, 4])
def test_cost_histogram_of_the_newest_frame_with_frames_in_flight(lib, flight):
    """After each frame, mirt_cost_histogram returns THAT frame's histogram, whichever stream rendered it: the same words as
    the view's histogram with one frame in flight."""
    from devbuf import DeviceArray
    mirt.scene_upload(_soup())
    mirt.set_cost_histogram(True)
    W, H = 320, 240
    views = [_orbit_view(0.07 * i, 2.6 - 0.05 * i, W, H, 200.0) for i in range(7)]
    bufs = [DeviceArray((H, W), np.uint32) for _ in range(4)]
    try:
        mirt.set_frames_in_flight(1)
        single = [_gpu_histogram(v, 0, H, bufs[0])[0] for v in views]
        assert any(not np.array_equal(single[0], s) for s in single[1:])
        mirt.set_frames_in_flight(flight)
        for i, v in enumerate(views):
            h, _ = _gpu_histogram(v, 0, H, bufs[i % flight])
            assert np.array_equal(h, single[i]), (flight, i, [j for j, s in enumerate(single) if np.array_equal(h, s)])
        mirt.sync()
    finally:
        for b in bufs:
            b.free()
