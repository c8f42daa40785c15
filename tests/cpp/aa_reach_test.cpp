// Supersampling reaches a few ulp beyond the half pixel, and the binning's half-pixel pad relies on the edge-function margin for it.
//
// Draw() walks a pixel's sub-rays with x1 = x - 0.5f and x1 += 1.0f / (realSamples - 1) (raytracer.cpp:566-596; aa_start / aa_step
// of csrc/rt_common.hpp): a chain of rounded sums.  At 4, 6, 7 and 8 samples the chain ends ABOVE x + 0.5 for many coordinates, while
// a supersampled camera frame pads its bins by exactly half a pixel (make_camera_frame, capi/rt_frame.cpp) and the tile kernel widens
// its rectangles by exactly 0.5 (reach, csrc/rt_tile.hip).  A triangle that begins inside that sliver beyond a bin's last column is
// kept for the bin only by the margin m of its edge function (make_edge_fn, csrc/rt_binned.hpp).  Checked here on the CPU, built with
// -ffp-contract=off like the library:
//   (a) the chain for 2 .. 8 samples over every coordinate of the largest frame side the binning accepts: worst overshoot in pixels
//       and in ulps of the coordinate; none at 2, 3 and 5 samples; the start c - 0.5 is exact;
//   (b) for the slivers tests/test_aa_reach.py hands over (the scenes of tests/supersampling.py, and slivers at the worst coordinates
//       of (a) on frames as wide as those need): the bin range box_to_bins gives add_bbox's box contains the bins of pixel c, the
//       cell test keeps (sliver, bin of c), and the tile kernel's rectangle test keeps (sliver, tile of c);
//   (c) the ratio overshoot / margin distance, margin distance = m / sqrt(cu^2 + cv^2) of the sliver's nearest edge function, stays
//       below 1 -- and below twice the worst this program measured when it was added (the figures of DESIGN.md section 3.2).
// make_edge_fn, make_bin_fns, add_bbox and box_to_bins are the library's own; the frame description, the folded cell test of
// k_bin_pairs and rect_may_hit are device code or need the runtime, and are restated below line for line.
// Restated code can drift from the device code it copies: whoever changes csrc/rt_binned.hip's BinItem constants, rect_may_hit or
// make_camera_frame changes them here too.  Not covered here at all: the coarse levels of the cell walk (A0, A1: 64 x 64 and 8 x 8
// bins) and the frame_may_see prefilter that band frames run in front of the set-up -- only the GPU tests
// (tests/test_gpu_supersampling.py: whole frames and bands of these slivers) reach those.
#include "../../cpp-raytracer-rasterizer_amd/csrc/rt_binned.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

using namespace mirt;

// ---- restated: aa_start / aa_step (csrc/rt_common.hpp) ----
static float chain_start(int c, int rs) { return rs > 1 ? (float)c - 0.5f : (float)c; }
static float chain_step(int rs) { return 1.0f / (float)(rs - 1); }

// ---- restated: make_camera_frame (capi/rt_frame.cpp), the rotation's inverse as its transpose ----
static BinFrameDesc camera_frame(const float *pos, const float *R, float focal, int W, int H, int aa)
{
    BinFrameDesc c;
    memset(&c, 0, sizeof c);
    const float hw = (float)W / 2.0f, hh = (float)H / 2.0f;
    for (int i = 0; i < 3; i++) {
        c.Pu[i] = -R[0 + i];
        c.Pv[i] = -R[3 + i];
        c.P0[i] = -(R[6 + i] * focal - R[0 + i] * hw - R[3 + i] * hh);
    }
    float dm = 0.0f;
    for (int i = 0; i < 3; i++)
        dm = fmaxf(dm, fabsf(R[0 + i]) * (hw + 1.0f) + fabsf(R[3 + i]) * (hh + 1.0f) + fabsf(R[6 + i]) * fabsf(focal));
    c.dmax = dm;
    for (int i = 0; i < 3; i++) {
        const double rwd = -(double)R[6 + i] / (double)focal;       // (R^-1)(2, i) = R(i, 2) = R[6 + i]
        c.rw[i] = (float)rwd;
        c.ru[i] = (float)(-(double)R[0 + i] + (double)hw * rwd);
        c.rv[i] = (float)(-(double)R[3 + i] + (double)hh * rwd);
    }
    memcpy(c.S, pos, 12);
    c.ulo = 0.0f; c.vlo = 0.0f; c.du = (float)BIN_TILE; c.dv = (float)BIN_TILE;
    c.pad_lo = aa > 1 ? -0.5f : 0.0f; c.pad_hi = aa > 1 ? -0.5f : -1.0f;
    c.nbu = (W + BIN_TILE - 1) / BIN_TILE; c.nbv = (H + BIN_TILE - 1) / BIN_TILE;
    c.j0 = 0; c.j1 = c.nbv;
    c.nshell = 1;
    return c;
}

// ---- restated: the folded cell test of k_bin_pairs at one bin (csrc/rt_binned.hip: BinItem's A2 / Bu / Bv, cell_may_hit with K = 1) ----
static float corner(float s, float lo, float hi) { return fmaxf(s * lo, s * hi); }
static bool bin_may_hit(const TriBinFns &t, const BinFrameDesc &fr, int i, int j, bool *in_box)
{
    const float T = 1.6940658945086007e-21f;
    const bool both = fabsf(t.nb) < T || !(t.nb == t.nb);
    const float sgn = t.nb < 0.0f ? -1.0f : 1.0f;
    const EdgeFn *fn[4] = { &t.n, &t.p, &t.q, &t.s };
    const float I = (float)i, J = (float)j, inf = __builtin_huge_valf();
    bool ok = true;
    for (int k = 0; k < 4; k++) {
        const float su = sgn * fn[k]->cu, sv = sgn * fn[k]->cv;
        const float base = sgn * fn[k]->c0 + fn[k]->m + su * fr.ulo + sv * fr.vlo;
        const float Bu = both ? 0.0f : su * fr.du, Bv = both ? 0.0f : sv * fr.dv;
        const float A2 = both ? inf : base + corner(su, fr.pad_lo, fr.du + fr.pad_hi) + corner(sv, fr.pad_lo, fr.dv + fr.pad_hi);
        ok = ok && (__builtin_fmaf(J, Bv, __builtin_fmaf(I, Bu, A2)) >= 0.0f);
    }
    float lou = -inf, hiu = inf, lov = -inf, hiv = inf;
    if (t.bstate == BOX_VALID) {
        box_to_bins(t.bu0, t.bu1, fr.ulo, fr.pad_lo, fr.pad_hi, bin_rcp(fr.du), &lou, &hiu);
        box_to_bins(t.bv0, t.bv1, fr.vlo, fr.pad_lo, fr.pad_hi, bin_rcp(fr.dv), &lov, &hiv);
    } else if (t.bstate == BOX_EMPTY) {
        lou = lov = inf; hiu = hiv = -inf;
    }
    *in_box = (I + 1.0f >= lou) && (I <= hiu) && (J + 1.0f >= lov) && (J <= hiv);
    return ok && *in_box;
}

// ---- restated: fn_range / rect_may_hit (csrc/rt_binned.hpp, device only), as k_rt_tile2 calls it: no box ----
static void fn_range(const EdgeFn &e, float u0, float u1, float v0, float v1, float *lo, float *hi)
{
    const float a0 = e.cu * u0, a1 = e.cu * u1, b0 = e.cv * v0, b1 = e.cv * v1;
    *hi = e.c0 + fmaxf(a0, a1) + fmaxf(b0, b1);
    *lo = e.c0 + fminf(a0, a1) + fminf(b0, b1);
}
static bool rect_may_hit(const TriBinFns &t, float u0, float u1, float v0, float v1)
{
    float nlo, nhi, plo, phi, qlo, qhi, slo, shi;
    fn_range(t.n, u0, u1, v0, v1, &nlo, &nhi);
    fn_range(t.p, u0, u1, v0, v1, &plo, &phi);
    fn_range(t.q, u0, u1, v0, v1, &qlo, &qhi);
    fn_range(t.s, u0, u1, v0, v1, &slo, &shi);
    const float T = 2.384185791015625e-07f;
    const bool pos = (nhi > -t.n.m) && (phi >= -t.p.m) && (qhi >= -t.q.m) && (shi >= -t.s.m) && (t.nb > -T);
    const bool neg = (nlo < t.n.m) && (plo <= t.p.m) && (qlo <= t.q.m) && (slo <= t.s.m) && (t.nb < T);
    return pos || neg;
}

// The worst ratio overshoot / margin distance this program printed per sample count at the commit that added it, over the directed
// slivers and the slivers at the worst coordinates alike (DESIGN.md section 3.2 quotes them); the assertion leaves a factor 2.
static const double MEASURED_WORST_RATIO[9] = { 0, 0, 0, 0, 0.0157, 0, 0.0313, 0.0313, 0.0469 };

int main(int argc, char **argv)
{
    int bad = 0;
    const int LIMIT = 23000;                      // the largest frame side frame_fits_binning (capi/pass_plan.hpp) accepts
    // ---- (a) the chain ----
    for (int rs = 2; rs <= 8; rs++) {
        double worst_px = 0.0, worst_ulp = 0.0;
        int at_px = -1, at_ulp = -1, at_last8 = -1;
        long over = 0;
        double worst_last8 = 0.0;
        for (int c = 0; c <= LIMIT; c++) {
            float x1 = chain_start(c, rs);
            if ((double)x1 != (double)c - 0.5) { if (bad++ < 10) printf("FAIL: start of %d at %d samples is not exact\n", c, rs); }
            for (int k = 0; k < rs - 1; k++) x1 += chain_step(rs);
            const double ov = (double)x1 - ((double)c + 0.5);
            if (ov <= 0.0) continue;
            over++;
            const float half = (float)c + 0.5f;
            const double ulps = ov / ((double)nextafterf(half, 1.0e9f) - (double)half);
            if (ov > worst_px) { worst_px = ov; at_px = c; }
            if (ulps > worst_ulp) { worst_ulp = ulps; at_ulp = c; }
            if (c % 8 == 7 && ov > worst_last8) { worst_last8 = ov; at_last8 = c; }
        }
        printf("chain samples=%d overshooting=%ld worst_px=%.9g at=%d worst_ulps=%.3g at_ulps=%d worst_last_of_8=%.9g at_last8=%d\n",
               rs, over, worst_px, at_px, worst_ulp, at_ulp, worst_last8, at_last8);
        const bool none = rs == 2 || rs == 3 || rs == 5;
        if (none != (over == 0)) { printf("FAIL: %d samples: %ld coordinates overshoot\n", rs, over); bad++; }
    }
    // ---- (b), (c) the slivers ----
    if (argc < 2) { printf("usage: aa_reach_test <slivers file>\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    double worst[2][9] = { { 0 } };
    long count[2][9] = { { 0 } }, pairs = 0;
    for (;;) {
        char kind[8];
        int rs, W, H, axis, c;
        float focal, pos[3], R[9], t15[15];
        double ov;
        if (fscanf(f, "%7s %d %d %d %f", kind, &rs, &W, &H, &focal) != 5) break;
        bool ok = true;
        for (int k = 0; k < 3; k++) ok = ok && fscanf(f, "%f", &pos[k]) == 1;
        for (int k = 0; k < 9; k++) ok = ok && fscanf(f, "%f", &R[k]) == 1;
        ok = ok && fscanf(f, "%d %d %lf", &axis, &c, &ov) == 3;
        memset(t15, 0, sizeof t15);
        for (int k = 0; k < 9; k++) ok = ok && fscanf(f, "%f", &t15[k]) == 1;
        if (!ok || rs < 2 || rs > 8) { printf("FAIL: malformed sliver record\n"); return 2; }
        const int wide = kind[0] == 'W';
        const BinFrameDesc fr = camera_frame(pos, R, focal, W, H, rs);
        const OriginRow row = make_origin_row(t15, V3(pos[0], pos[1], pos[2]));
        TriBinFns t = make_bin_fns(row, fr);
        add_bbox(t, t15, fr);
        // the bins and the tiles of pixel c along the sliver (it spans rows, or columns, 4 .. size - 4)
        const int span = axis == 0 ? H : W;
        for (int r = 5; r < span - 5; r++) {
            const int px = axis == 0 ? c : r, py = axis == 0 ? r : c;
            if (r != 5 && r % 8 != 0) continue;                    // once per bin (bins are 8 pixels, tile rows 8, tile columns 16)
            bool in_box;
            const bool kept = bin_may_hit(t, fr, px / BIN_TILE, py / BIN_TILE, &in_box);
            pairs++;
            if (t.bstate == BOX_EMPTY || !in_box) {
                if (bad++ < 10) printf("FAIL: %s sliver at %s %d, %d samples, %d x %d: box state %d, bin (%d, %d) outside its range\n", kind,
                                       axis ? "row" : "column", c, rs, W, H, t.bstate, px / BIN_TILE, py / BIN_TILE);
            } else if (!kept) {
                if (bad++ < 10) printf("FAIL: %s sliver at %s %d, %d samples, %d x %d: the cell test drops bin (%d, %d)\n", kind,
                                       axis ? "row" : "column", c, rs, W, H, px / BIN_TILE, py / BIN_TILE);
            }
            const int x0 = px / 16 * 16, y0 = py / 8 * 8;
            const int xe = x0 + 15 < W - 1 ? x0 + 15 : W - 1, ye = y0 + 7 < H - 1 ? y0 + 7 : H - 1;
            TriBinFns nobox = t;
            nobox.bstate = BOX_NONE;
            if (!rect_may_hit(nobox, (float)x0 - 0.5f, (float)xe + 0.5f, (float)y0 - 0.5f, (float)ye + 0.5f) && bad++ < 10)
                printf("FAIL: %s sliver at %s %d, %d samples, %d x %d: the tile kernel's rectangle test drops tile (%d, %d)\n", kind,
                       axis ? "row" : "column", c, rs, W, H, x0 / 16, y0 / 8);
        }
        // the nearest edge function: the one whose zero line passes closest to the middle of the sliver's edge
        const double mu = axis == 0 ? (double)c + 0.5 : 0.5 * W, mv = axis == 0 ? 0.5 * H : (double)c + 0.5;
        const EdgeFn *fn[3] = { &t.p, &t.q, &t.s };
        double best = 1.0e300, margin = 0.0;
        for (int k = 0; k < 3; k++) {
            const double g = std::sqrt((double)fn[k]->cu * fn[k]->cu + (double)fn[k]->cv * fn[k]->cv);
            const double dist = std::fabs((double)fn[k]->c0 + (double)fn[k]->cu * mu + (double)fn[k]->cv * mv) / g;
            if (dist < best) { best = dist; margin = (double)fn[k]->m / g; }
        }
        if (!(best < 1.0e-2)) { if (bad++ < 10) printf("FAIL: no edge function of the sliver at %d passes its edge (nearest %.3g pixels)\n", c, best); continue; }
        const double ratio = ov / margin;
        count[wide][rs]++;
        if (ratio > worst[wide][rs]) worst[wide][rs] = ratio;
        if (!(ratio < 1.0) && bad++ < 10)
            printf("FAIL: %s sliver at %s %d, %d samples, %d x %d: overshoot %.3g pixels is %.3g of the margin distance %.3g\n", kind,
                   axis ? "row" : "column", c, rs, W, H, ov, ratio, margin);
    }
    fclose(f);
    for (int rs = 2; rs <= 8; rs++) {
        if (!count[0][rs] && !count[1][rs]) continue;
        printf("ratio samples=%d directed=%.6g (%ld slivers) worst_coordinates=%.6g (%ld slivers)\n", rs, worst[0][rs], count[0][rs], worst[1][rs], count[1][rs]);
        const double w = worst[0][rs] > worst[1][rs] ? worst[0][rs] : worst[1][rs];
        if (!(w < 2.0 * MEASURED_WORST_RATIO[rs])) { printf("FAIL: %d samples: ratio %.6g is beyond twice the %.6g measured when this test was added\n", rs, w, MEASURED_WORST_RATIO[rs]); bad++; }
    }
    for (int rs = 4; rs <= 8; rs++)
        if (rs != 5 && (count[0][rs] < 4 || count[1][rs] < 4)) { printf("FAIL: too few slivers at %d samples\n", rs); bad++; }
    printf("%ld (sliver, bin) pairs\n", pairs);
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
