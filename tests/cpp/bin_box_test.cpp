// add_bbox (csrc/rt_binned.hpp) places a CONSERVATIVE box with the hardware's one-ulp reciprocal and reciprocal square root
// where it used IEEE divisions and square roots.  Checked here on the CPU (built with -ffp-contract=off like the library) against
// the exact-division code it replaced, kept below as the model, with host twins of the two approximations that return the exact
// value times 1 + 2^-22 or 1 - 2^-22 -- always up, always down, or drawn per call:
//   1. where the model has a box (BOX_VALID), the new code has a box that contains it, or none (BOX_NONE, "every bin");
//      where the model has none, the new code has none;
//   2. the new code says BOX_EMPTY ("no ray of the family can hit") only where the model says so.
// Triangles: soup-like ones, needles of aspect 1:1000 and beyond, slivers near the projection plane, triangles all behind it, and
// coordinates up to the 1e8 the host admits; each projected into a camera frame and into the six faces of a light's cube.
#include <cmath>
#include <cstdint>

static int twin_mode = 0;                         // 0: per call, 1: always up, 2: always down
static uint64_t twin_state = 0x2545F4914F6CDD1Dull;
static float twin_scale(double exact)
{
    twin_state ^= twin_state << 13; twin_state ^= twin_state >> 7; twin_state ^= twin_state << 17;
    const bool up = twin_mode == 1 || (twin_mode == 0 && (twin_state >> 33 & 1u));
    return (float)(exact * (up ? 1.0 + 2.384185791015625e-07 : 1.0 - 2.384185791015625e-07));
}
static float twin_rcp(float x) { return twin_scale(1.0 / (double)x); }
static float twin_rsq(float x) { return twin_scale(1.0 / std::sqrt((double)x)); }
#define MIRT_BIN_HOST_RCP(x) twin_rcp(x)
#define MIRT_BIN_HOST_RSQ(x) twin_rsq(x)

#include "../../cpp-raytracer-rasterizer_amd/csrc/rt_binned.hpp"

#include <cstdio>
#include <cstring>

using namespace mirt;

// ---- the model: add_bbox with IEEE divisions and square roots, as it stood before the approximations ----
static void model_add_bbox(TriBinFns &t, const float *t15, const BinFrameDesc &fr)
{
    float us[3], vs[3], pad = 0.0f;
    int front = 0, behind = 0;
    for (int j = 0; j < 3; j++) {
        const float gx = fr.S[0] - t15[3 * j], gy = fr.S[1] - t15[3 * j + 1], gz = fr.S[2] - t15[3 * j + 2];
        const float w = fr.rw[0] * gx + fr.rw[1] * gy + fr.rw[2] * gz;
        const float wm = fabsf(fr.rw[0] * gx) + fabsf(fr.rw[1] * gy) + fabsf(fr.rw[2] * gz);
        front += (w > 0.00390625f * wm);
        behind += (w < -0.00390625f * wm);
        const float un = fr.ru[0] * gx + fr.ru[1] * gy + fr.ru[2] * gz, vn = fr.rv[0] * gx + fr.rv[1] * gy + fr.rv[2] * gz;
        const float um = fabsf(fr.ru[0] * gx) + fabsf(fr.ru[1] * gy) + fabsf(fr.ru[2] * gz);
        const float vm = fabsf(fr.rv[0] * gx) + fabsf(fr.rv[1] * gy) + fabsf(fr.rv[2] * gz);
        us[j] = un / w; vs[j] = vn / w;
        const float iw = 1.0f / fabsf(w);
        pad = fmaxf(pad, 4.76837158203125e-07f * ((um + fabsf(us[j]) * wm) * iw + (vm + fabsf(vs[j]) * wm) * iw) +
                             2.384185791015625e-07f * (fabsf(us[j]) + fabsf(vs[j])));
    }
    if (front != 3 && behind != 3) return;
    const float u0 = fminf(fminf(us[0], us[1]), us[2]), u1 = fmaxf(fmaxf(us[0], us[1]), us[2]);
    const float v0 = fminf(fminf(vs[0], vs[1]), vs[2]), v1 = fmaxf(fmaxf(vs[0], vs[1]), vs[2]);
    const float ext = fmaxf(u1 - u0, v1 - v0);
    const float ax = us[1] - us[0], ay = vs[1] - vs[0], bx = us[2] - us[0], by = vs[2] - vs[0], cx = us[2] - us[1], cy = vs[2] - vs[1];
    const float area2 = fabsf(ax * by - ay * bx);
    const float per = sqrtf(ax * ax + ay * ay) + sqrtf(bx * bx + by * by) + sqrtf(cx * cx + cy * cy);
    const float dp = t.p.m / sqrtf(t.p.cu * t.p.cu + t.p.cv * t.p.cv);
    const float dq = t.q.m / sqrtf(t.q.cu * t.q.cu + t.q.cv * t.q.cv);
    const float ds = t.s.m / sqrtf(t.s.cu * t.s.cu + t.s.cv * t.s.cv);
    const float d = fmaxf(fmaxf(dp, dq), ds) + pad;
    if (behind == 3) {
        const float area_lo = area2 - 2.0f * pad * per - 4.76837158203125e-07f * (fabsf(ax * by) + fabsf(ay * bx));
        if (d < 0.5f * (area_lo / per)) t.bstate = BOX_EMPTY;
        return;
    }
    const float l01 = sqrtf(ax * ax + ay * ay), l02 = sqrtf(bx * bx + by * by), l12 = sqrtf(cx * cx + cy * cy);
    const float e01x = ax / l01, e01y = ay / l01, e02x = bx / l02, e02y = by / l02, e12x = cx / l12, e12y = cy / l12;
    const float dd = 1.25f * d;
    const float k0 = dd / fabsf(e01x * e02y - e01y * e02x), k1 = dd / fabsf(e01x * e12y - e01y * e12x), k2 = dd / fabsf(e02x * e12y - e02y * e12x);
    const float px0 = us[0] - k0 * (e01x + e02x), py0 = vs[0] - k0 * (e01y + e02y);
    const float px1 = us[1] - k1 * (e12x - e01x), py1 = vs[1] - k1 * (e12y - e01y);
    const float px2 = us[2] + k2 * (e02x + e12x), py2 = vs[2] + k2 * (e02y + e12y);
    const float slack = 2.0f * pad + 1.0e-6f * ext;
    const float bu0 = fminf(fminf(px0, px1), px2) - slack, bu1 = fmaxf(fmaxf(px0, px1), px2) + slack;
    const float bv0 = fminf(fminf(py0, py1), py2) - slack, bv1 = fmaxf(fmaxf(py0, py1), py2) + slack;
    if (!(bu0 > -1.0e30f && bu1 < 1.0e30f && bv0 > -1.0e30f && bv1 < 1.0e30f)) return;
    t.bu0 = fminf(bu0, u0 - slack); t.bu1 = fmaxf(bu1, u1 + slack); t.bv0 = fminf(bv0, v0 - slack); t.bv1 = fmaxf(bv1, v1 + slack);
    t.bstate = BOX_VALID;
}

// ---- frames: what capi/rt_frame.cpp and capi/binned.cpp build (a camera of yaw `yaw` at `pos`; face `face` of a light's cube) ----
static BinFrameDesc camera_frame(const float *pos, double yaw, int W, int H)
{
    BinFrameDesc c;
    memset(&c, 0, sizeof c);
    const double cs = std::cos(yaw), sn = std::sin(yaw), f = H / 2.0, hw = W / 2.0, hh = H / 2.0;
    // rotation about y, column-major; its inverse is its transpose
    const double R[9] = { cs, 0, -sn, 0, 1, 0, sn, 0, cs };
    for (int i = 0; i < 3; i++) {
        c.Pu[i] = (float)-R[0 + i]; c.Pv[i] = (float)-R[3 + i];
        c.P0[i] = (float)-(R[6 + i] * f - R[0 + i] * hw - R[3 + i] * hh);
        const double rwd = -R[6 + i] / f;                       // (R^-1)(2, i) = R(i, 2) = R[6 + i]
        c.rw[i] = (float)rwd;
        c.ru[i] = (float)(-R[0 + i] + hw * rwd);
        c.rv[i] = (float)(-R[3 + i] + hh * rwd);
    }
    float dm = 0.0f;
    for (int i = 0; i < 3; i++)
        dm = fmaxf(dm, fabsf((float)R[0 + i]) * ((float)hw + 1.0f) + fabsf((float)R[3 + i]) * ((float)hh + 1.0f) + fabsf((float)R[6 + i]) * (float)f);
    c.dmax = dm;
    memcpy(c.S, pos, 12);
    c.du = c.dv = (float)BIN_TILE;
    c.pad_lo = 0.0f; c.pad_hi = -1.0f;
    c.nbu = (W + BIN_TILE - 1) / BIN_TILE; c.nbv = (H + BIN_TILE - 1) / BIN_TILE; c.j0 = 0; c.j1 = c.nbv;
    c.nshell = 1;
    return c;
}

static BinFrameDesc cube_frame(const float *pos, int face, int cube_bins)
{
    BinFrameDesc d;
    memset(&d, 0, sizeof d);
    const int ax = face >> 1;
    d.P0[ax] = (face & 1) ? -1.0f : 1.0f;
    d.Pu[(ax + 1) % 3] = 1.0f; d.Pv[(ax + 2) % 3] = 1.0f;
    d.rw[ax] = d.P0[ax]; d.ru[(ax + 1) % 3] = 1.0f; d.rv[(ax + 2) % 3] = 1.0f;
    memcpy(d.S, pos, 12);
    d.dmax = 2.0f;
    d.ulo = d.vlo = -1.0f; d.du = d.dv = 2.0f / (float)cube_bins;
    d.pad_lo = -3.814697265625e-06f; d.pad_hi = 3.814697265625e-06f;
    d.nbu = d.nbv = cube_bins; d.j0 = 0; d.j1 = cube_bins; d.tab = 1; d.nshell = 1;
    return d;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}
static double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }
static double sym() { return 2.0 * uni() - 1.0; }

// a triangle of the given kind around a point in front of, beside or behind the origin `S` of the family
static void make_triangle(int kind, const float *S, float *t15)
{
    memset(t15, 0, 15 * sizeof(float));
    double c[3], a[3], b[3];
    const double reach = kind == 5 ? 1.0e8 : (kind == 4 ? 50.0 : 3.0);
    for (int k = 0; k < 3; k++) c[k] = S[k] + reach * sym();
    if (kind == 3) c[2] = S[2] - 2.0 - 3.0 * uni();                            // all behind the camera's plane (it looks along +z)
    const double size = kind == 5 ? 1.0e8 * uni() : (kind == 0 ? 0.05 : 0.02 + uni());
    for (int k = 0; k < 3; k++) { a[k] = size * sym(); b[k] = size * sym(); }
    if (kind == 1) {                                                           // needle: the third vertex 1e-3 .. 1e-5 of the length beside the long edge
        const double thin = std::pow(10.0, -3.0 - 2.0 * uni()), along = uni();
        double o[3] = { sym(), sym(), sym() };
        for (int k = 0; k < 3; k++) b[k] = along * a[k] + thin * size * o[k];
    }
    if (kind == 2) {                                                           // sliver near the projection plane: z within 1e-3 .. 1e-7 of the origin's
        const double off = std::pow(10.0, -3.0 - 4.0 * uni()) * sym();
        c[2] = S[2] + off; a[2] *= 1.0e-3 * uni(); b[2] *= 1.0e-3 * uni();
    }
    for (int k = 0; k < 3; k++) { t15[k] = (float)c[k]; t15[3 + k] = (float)(c[k] + a[k]); t15[6 + k] = (float)(c[k] + b[k]); }
}

int main()
{
    const float cam[3] = { 0.0f, 0.0f, -2.0f }, light[3] = { 0.0f, -0.5f, -0.7f }, far_light[3] = { 3.0e7f, -2.0e7f, 1.0e7f };
    BinFrameDesc frames[16];
    int nframes = 0;
    frames[nframes++] = camera_frame(cam, 0.0, 1920, 1080);
    frames[nframes++] = camera_frame(cam, 0.7, 203, 117);
    for (int f = 0; f < 6; f++) frames[nframes++] = cube_frame(light, f, 64);
    for (int f = 0; f < 6; f++) frames[nframes++] = cube_frame(far_light, f, 256);
    long tested = 0, boxed = 0, lost_box = 0, empty_model = 0, empty_new = 0, bad = 0;
    long valid_kind[6] = { 0 }, lost_kind[6] = { 0 };
    double widest = 0.0;
    float t15[15];
    for (int mode = 0; mode < 3; mode++) {
        twin_mode = mode;
        const long n = mode == 0 ? 200000 : 50000;
        for (long it = 0; it < n; it++) {
            const int kind = (int)(it % 6);
            const int fi = (int)(rnd() % (uint64_t)nframes);
            const BinFrameDesc &fr = frames[fi];
            make_triangle(kind, fr.S, t15);
            // (every triangle against its own frame and against the two neighbours in the list: four views of it in all modes)
            for (int df = 0; df < 3; df++) {
                const BinFrameDesc &f2 = frames[(fi + df) % nframes];
                const OriginRow row = make_origin_row(t15, V3(f2.S[0], f2.S[1], f2.S[2]));
                TriBinFns m = make_bin_fns(row, f2), g = m;
                model_add_bbox(m, t15, f2);
                add_bbox(g, t15, f2);
                tested++;
                empty_model += m.bstate == BOX_EMPTY; empty_new += g.bstate == BOX_EMPTY;
                bool ok = true;
                if (g.bstate == BOX_EMPTY) ok = m.bstate == BOX_EMPTY;
                else if (m.bstate == BOX_NONE) ok = g.bstate == BOX_NONE;
                else if (m.bstate == BOX_VALID) {
                    valid_kind[kind]++;
                    if (g.bstate == BOX_NONE) { lost_box++; lost_kind[kind]++; }
                    else {
                        boxed++;
                        ok = g.bu0 <= m.bu0 && g.bu1 >= m.bu1 && g.bv0 <= m.bv0 && g.bv1 >= m.bv1;
                        const double wm = (double)(m.bu1 - m.bu0) + (double)(m.bv1 - m.bv0), wg = (double)(g.bu1 - g.bu0) + (double)(g.bv1 - g.bv0);
                        if (wm > 0.0 && wg / wm - 1.0 > widest) widest = wg / wm - 1.0;
                    }
                }
                if (!ok && bad++ < 10)
                    printf("FAIL mode %d kind %d frame %d: model state %d box [%.9g %.9g] x [%.9g %.9g], new state %d box [%.9g %.9g] x [%.9g %.9g]\n", mode, kind,
                           (int)((fi + df) % nframes), m.bstate, m.bu0, m.bu1, m.bv0, m.bv1, g.bstate, g.bu0, g.bu1, g.bv0, g.bv1);
            }
        }
    }
    printf("%ld views: %ld boxes contain the model's (widest by %.3g of the model's half perimeter), %ld gave their box up, BOX_EMPTY %ld of the model's %ld, %ld failures\n",
           tested, boxed, widest, lost_box, empty_new, empty_model, bad);
    // the generator must reach what it is meant to reach
    if (boxed < tested / 10 || empty_new < tested / 100 || empty_new > empty_model) { printf("FAIL: the cases do not cover both outcomes\n"); return 1; }
    // A box is given up only for a corner whose sine is below ~2^-18 = 4e-6 once 2^-19 of the cross product's terms is off.  The
    // sharpest needles drawn have 1e-5 of their length as their width and the projection can foreshorten that; soup triangles,
    // slivers and far triangles reach such corners by chance only.  So: needles may lose one box in ten, every other kind one in fifty.
    for (int k = 0; k < 6; k++) {
        printf("kind %d: %ld of the model's %ld boxes given up\n", k, lost_kind[k], valid_kind[k]);
        if (valid_kind[k] < 1000 || lost_kind[k] * (k == 1 ? 10 : 50) > valid_kind[k]) { printf("FAIL: too many boxes given up (or too few cases) for kind %d\n", k); bad++; }
    }
    // ---- box_to_bins: the range with a reciprocal and 2^-18 + 2^-20 contains the range a division and 2^-18 give ----
    long ranges = 0;
    for (int mode = 0; mode < 3; mode++) {
        twin_mode = mode;
        for (long it = 0; it < 100000; it++) {
            const float steps[5] = { 8.0f, 2.0f / 64.0f, 2.0f / 128.0f, 2.0f / 256.0f, (float)(0.01 + 10.0 * uni()) };
            const float step = steps[rnd() % 5u], org = (rnd() & 1u) ? -1.0f : 0.0f, pad_lo = (rnd() & 1u) ? 0.0f : -3.814697265625e-06f, pad_hi = (rnd() & 1u) ? -1.0f : 3.814697265625e-06f;
            const double mag = std::pow(10.0, -3.0 + 9.0 * uni());
            const float b0 = (float)(mag * sym()), b1 = b0 + (float)(mag * uni());
            float lo, hi;
            box_to_bins(b0, b1, org, pad_lo, pad_hi, bin_rcp(step), &lo, &hi);
            float mlo = (b0 - org - pad_hi) / step, mhi = (b1 - org - pad_lo) / step;
            mlo -= 3.814697265625e-06f * (1.0f + fabsf(mlo)); mhi += 3.814697265625e-06f * (1.0f + fabsf(mhi));
            ranges++;
            if (!(lo <= mlo && hi >= mhi) && bad++ < 10) printf("FAIL box_to_bins mode %d: [%.9g %.9g] step %.9g: model [%.9g %.9g], new [%.9g %.9g]\n", mode, b0, b1, step, mlo, mhi, lo, hi);
        }
    }
    printf("%ld bin ranges contain the division's\n", ranges);
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
