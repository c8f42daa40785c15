// along.hpp -- ray queries along ONE direction (mirt_intersect_along*, mirt_occluded_along*): the rays {origins[i], dir} share their
// direction and differ in their start.  What the structure is, the predicate that files a triangle into it (host and device: the
// one text, MIRT_HD), what a ray reads of it, and the parameter blocks of the kernels (along.hip).  DESIGN.md section 5.1 has the
// argument in full; its steps stand beside the code they justify.
//
// The family.  With negD = -dir fixed, the reference's three dot products (raytracer.cpp:232-234) are, in exact arithmetic,
//     pu  = be2 . negD  = (S - v0) . (e2 x negD)         qv  = e1b . negD = (S - v0) . (negD x e1)         den = e1e2 . negD
// -- pu and qv affine in the start S and unchanged when S moves along dir, den a constant of the triangle.  The projection of S
// along dir onto the coordinate plane across dir's dominant axis k, (p, q) = (S[k1] - c1 S[k], S[k2] - c2 S[k]) with c = dir[k1|k2] /
// dir[k], therefore plays the part (u, v) plays in a cube face: a grid of B x B cells over the projected
// bounding box of the SCENE, every cell's list ordered in depth shells along dir.  Nothing depends on the call's origins.
#pragma once

#include "../query/rt_query.hpp"

#include <math.h>

namespace mirt {

// ---- the structure's descriptor: a function of (dir, the scene's bounding box, B, shells) alone ----------------------------------
struct AlongDesc {
    float nd[3];                 // d' = negD * 2^k, largest component in [0.5, 1) (rt_query.hpp: fan_dir_of): what the triangles are filed for
    float dhat[3];               // dir / |dir| rounded to float: a ray's depth is S . dhat
    int k, k1, k2;               // dir's dominant axis and the two across
    float c1, c2;                // dir[k1] / dir[k], dir[k2] / dir[k], rounded: |c| <= 1
    float p0, q0, ip, iq;        // cell of (p, q): ((p - p0) * ip, (q - q0) * iq), inside the grid while both lie in [0, B)
    int B, shells;
    float shell_d0, shell_iw;    // bin_shell_of's parameters: the shell of depth x
    float smax;                  // a ray takes its cell while every |component| of its start is <= smax = ALONG_START_EXTENTS x the scene's extent
    float sigma;                 // what a row's depth bound is lowered by
    double pad;                  // cells: how far a ray's computed cell coordinate may lie from the exact one
    double wp, wq;               // 1 / ip, 1 / iq in double: a cell's width (off by 2^-53 of itself, nothing beside pad)
};

constexpr float ALONG_START_EXTENTS = 8.0f;      // smax in units of the scene's extent R = the largest |coordinate| of its bounding box
constexpr int ALONG_SHELLS = 8;
constexpr int ALONG_BINS_MIN = 8, ALONG_BINS_MAX = 256;
constexpr double ALONG_PAD_MAX = 0.25;           // a grid whose cells a float cannot tell apart this well is not built
// The every-ray list may hold this share of the scene (and always ALONG_EVERY_FLOOR rows: a small scene seen edge-on is mostly
// edge-on); beyond it the call takes the brute-force kernels.
constexpr int ALONG_EVERY_SHARE = 8, ALONG_EVERY_FLOOR = 64;

// Cells per grid side for n triangles: the smallest power of two with B x B >= n / 2, within [ALONG_BINS_MIN, ALONG_BINS_MAX].
inline int along_bins_for(int n)
{
    int B = ALONG_BINS_MIN;
    while (B < ALONG_BINS_MAX && (long long)B * B * 2 < (long long)n) B *= 2;
    return B;
}
inline int along_every_cap(int n) { return n / ALONG_EVERY_SHARE > ALONG_EVERY_FLOOR ? n / ALONG_EVERY_SHARE : ALONG_EVERY_FLOOR; }
inline uint32_t along_keys(int B, int shells) { return ((uint32_t)(B * B) + 1u) * (uint32_t)shells; }   // cell B * B: the every-ray list

MIRT_HD float along_sel(v3 a, int k) { return k == 0 ? a.x : (k == 1 ? a.y : a.z); }
MIRT_HD double along_sel(double x, double y, double z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

// The descriptor for `dir` over the box [lo3, hi3]; false when no structure is built for them: dir outside the fans' window
// (rt_query.hpp: largest component in [2^-32, 2^19), all finite), a box that is not finite, or cells finer than `pad` resolves.
inline bool along_make_desc(const float *dir, const float *lo3, const float *hi3, int B, int shells, AlongDesc *out)
{
    AlongDesc a;
    memset(&a, 0, sizeof a);
    const FanDir fd = fan_dir_of(V3(-dir[0], -dir[1], -dir[2]));
    if (!fd.formed) return false;
    a.nd[0] = fd.d.x; a.nd[1] = fd.d.y; a.nd[2] = fd.d.z;
    const float ax = fabsf(a.nd[0]), ay = fabsf(a.nd[1]), az = fabsf(a.nd[2]);
    a.k = ax >= ay && ax >= az ? 0 : (ay >= az ? 1 : 2);
    a.k1 = (a.k + 1) % 3; a.k2 = (a.k + 2) % 3;
    a.c1 = a.nd[a.k1] / a.nd[a.k]; a.c2 = a.nd[a.k2] / a.nd[a.k];
    double R = 0.0;
    for (int c = 0; c < 3; c++) {
        if (!(fabsf(lo3[c]) < MIRT_QUERY_START_MAX && fabsf(hi3[c]) < MIRT_QUERY_START_MAX && lo3[c] <= hi3[c])) return false;
        R = fmax(R, fmax(fabs((double)lo3[c]), fabs((double)hi3[c])));
    }
    R = fmax(R, 1e-30);
    a.smax = (float)(ALONG_START_EXTENTS * R);
    a.sigma = (float)(ldexp(1.0, -16) * (R + (double)a.smax));
    const double len = sqrt((double)a.nd[0] * a.nd[0] + (double)a.nd[1] * a.nd[1] + (double)a.nd[2] * a.nd[2]);
    for (int c = 0; c < 3; c++) a.dhat[c] = (float)(-(double)a.nd[c] / len);
    double pl = INFINITY, ph = -INFINITY, ql = INFINITY, qh = -INFINITY, dl = INFINITY, dh = -INFINITY;
    for (int corner = 0; corner < 8; corner++) {
        double x[3];
        for (int c = 0; c < 3; c++) x[c] = (corner >> c & 1) ? (double)hi3[c] : (double)lo3[c];
        const double p = x[a.k1] - (double)a.c1 * x[a.k], q = x[a.k2] - (double)a.c2 * x[a.k];
        const double d = x[0] * a.dhat[0] + x[1] * a.dhat[1] + x[2] * a.dhat[2];
        pl = fmin(pl, p); ph = fmax(ph, p); ql = fmin(ql, q); qh = fmax(qh, q); dl = fmin(dl, d); dh = fmax(dh, d);
    }
    // one cell of margin on every side: a triangle's region reaches a little beyond its projection, and one that leaves the grid
    // goes on the every-ray list
    const double wp = fmax(ph - pl, ldexp(R, -10)) / (double)(B - 2), wq = fmax(qh - ql, ldexp(R, -10)) / (double)(B - 2);
    a.p0 = (float)(pl - wp); a.q0 = (float)(ql - wq);
    a.ip = (float)(1.0 / wp); a.iq = (float)(1.0 / wq);
    a.B = B; a.shells = shells;
    a.shell_d0 = (float)(dl - 4.0 * (double)a.sigma);
    a.shell_iw = dh > dl ? (float)((double)shells / (dh - dl + 8.0 * (double)a.sigma)) : 0.0f;
    // |computed cell coordinate - exact one| (along_cell_of): the rounding of c * S[k] and of the subtraction, 3.01 ulp of smax; of
    // p - p0, one ulp of 2 smax + |p0|; of the product with ip, one ulp of a coordinate below B.  2^-20 covers them three times over.
    const double padp = ldexp(1.0, -20) * ((double)a.ip * ((double)a.smax + fabs((double)a.p0)) + B);
    const double padq = ldexp(1.0, -20) * ((double)a.iq * ((double)a.smax + fabs((double)a.q0)) + B);
    a.pad = fmax(padp, padq);
    a.wp = 1.0 / (double)a.ip; a.wq = 1.0 / (double)a.iq;
    if (!(a.pad <= ALONG_PAD_MAX) || !(a.ip > 0.0f && a.ip < INFINITY && a.iq > 0.0f && a.iq < INFINITY)) return false;
    *out = a;
    return true;
}

// ---- what a ray reads of the descriptor ---------------------------------------------------------------------------------------------
// Whether the start may take its cell: finite and within smax (false for NaN; an infinity is beyond every smax).  The margins of
// along_tri_setup are sized for exactly these starts.
MIRT_HD bool along_start_in_reach(const AlongDesc &a, v3 S)
{
    return fabsf(S.x) <= a.smax && fabsf(S.y) <= a.smax && fabsf(S.z) <= a.smax;
}
// The start's cell, j * B + i, or -1 when its projection falls outside the grid.  Four roundings, in this order on host and device.
MIRT_HD int along_cell_of(const AlongDesc &a, v3 S)
{
    const float sk = along_sel(S, a.k);
    const float p = along_sel(S, a.k1) - a.c1 * sk, q = along_sel(S, a.k2) - a.c2 * sk;
    const float gi = (p - a.p0) * a.ip, gj = (q - a.q0) * a.iq;
    const bool in = gi >= 0.0f && gi < (float)a.B && gj >= 0.0f && gj < (float)a.B;
    return in ? (int)gj * a.B + (int)gi : -1;
}
// The start's depth along dir, (x + y) + z.
MIRT_HD float along_depth_of(const AlongDesc &a, v3 S) { return S.x * a.dhat[0] + S.y * a.dhat[1] + S.z * a.dhat[2]; }

// ---- the binning predicate ---------------------------------------------------------------------------------------------------------
//
// Per triangle, from the row the reference's own operations leave (v0, e1, e2, e1e2 as FLOATS: QueryRow) and d' = a.nd, in double
// -- a product of two floats is exact there and every sum is off by 2^-53 of itself, nothing beside the margins below --:
//     Nu = e2 x d', Nv = d' x e1, den = e1e2 . d'          pu(S) = (S - v0) . Nu, qv(S) = (S - v0) . Nv.
// What the reference computes in float differs from these by at most (u = 2^-24; Mb >= every |component| of b = S - v0 rounded, E1,
// E2, X, D the largest |component| of e1, e2, e1e2, d'):
//     |pu_f - pu| <= 36.1 u Mb E2 D   (b: 1 rounding; a cross component: two products and a difference, so 6.01 u Mb E2 on a value
//                                      below 2 Mb E2; the dot in (x + y) + z order: three roundings on each of three terms)
//     |qv_f - qv| <= 36.1 u Mb E1 D                        |den_f - den| <= 9.01 u X D
// taken as m_u = 2^-18 Mb E2 D, m_v = 2^-18 Mb E1 D, m_d = 2^-20 X D (64 u and 16 u).  The dots the kernels compute are those of
// negD itself, 2^-k times the dots of d' bit for bit unless a result is subnormal (rt_query.hpp); a0 = 2^-80 stands for that and for
// the quotients u, v that underflow to -0.
//
// Conditioning.  |den| >= 64 m_d: then den_f has den's sign s and is not zero, and the accept test u >= 0, v >= 0, u + v <= 1
// (:239) implies          s pu >= -(m_u + a0)        s qv >= -(m_v + a0)        s (pu + qv) <= |den| (1 + 2^-22) + m_u + m_v + 2 m_d + a0
// (fl(u + v) <= 1 gives u + v <= 1 + 2^-24, each quotient is within 2^-24 of itself: (pu_f + qv_f) / den_f <= 1 + 2^-22).
// In the cell coordinates S = (p + c1 z) e_k1 + (q + c2 z) e_k2 + z e_k an affine N . (S - v0) reads N[k1] (p - pv) + N[k2] (q - qv)
// + gamma (z - v0[k]), gamma = N[k1] c1 + N[k2] c2 + N[k]: zero for the exact c, a few 2^-24 |N| for the rounded one, so |gamma| Mb
// joins each threshold (tu, tv, tw below).  The three half-planes' normals sum to zero, so with det = au bv - av bu bounded away
// from zero (no corner too sharp: 2^-30 of the normals' lengths) they enclose a triangle, whose corners are the images of (-tu, -tv),
// (-tu, tw + tu), (tw + tv, -tv) under the inverse of (gu, gv).  Its box, grown by 2^-20 of its own size for the division, goes to
// cells, each refined by along_cell_may_hit.
// Anything else -- |den| within 64 m_d (edge-on: the signs of t, u, v are noise in the reference), a corner too sharp, a value that
// is not finite, a box that leaves the grid -- is ALONG_EVERY: on the list every ray tests, never skipped by depth.
//
// Depth.  An accepted test has u, v >= 0 and u + v <= 1 + 2^-24 in float, so pos = v0 + u e1 + v e2 (:241) lies within 2^-20 of the
// triangle's size of the triangle, and the distance (:242) is at least |(pos - S) . h| / |h| for ANY vector h, in particular for
// dhat: dist >= (min over corners of corner . dhat) - S . dhat - slack.  sigma = 2^-16 (R + smax) covers the slack -- pos, the
// float depth of S, |dhat| - 1, the length's roundings, each a few 2^-22 of R + smax -- several times, and `near` is lowered by two of it.
enum { ALONG_CELLS = 0, ALONG_EVERY = 1 };
struct AlongTri {
    int kind;
    double au, bu, av, bv;       // the normals of s pu and s qv in (p, q)
    double tu, tv, tw;           // gu >= -tu, gv >= -tv, gu + gv <= tw
    double pv, qv;               // v0's projection
    int i0, i1, j0, j1;          // the cell box, inclusive
    float near;                  // depth bound: a row is skipped when near > (the start's depth) + (the ray's distance bound)
};

MIRT_HD double along_max3(double a, double b, double c) { return fmax(fmax(fabs(a), fabs(b)), fabs(c)); }

MIRT_HD AlongTri along_tri_setup(const AlongDesc &a, v3 v0, v3 e1, v3 e2, v3 x)
{
    AlongTri t;
    t.kind = ALONG_EVERY;
    t.au = t.bu = t.av = t.bv = t.tu = t.tv = t.tw = t.pv = t.qv = 0.0;
    t.i0 = t.j0 = 0; t.i1 = t.j1 = -1;
    t.near = -INFINITY;
    const double nx = a.nd[0], ny = a.nd[1], nz = a.nd[2];
    const double V0 = along_max3(v0.x, v0.y, v0.z), E1 = along_max3(e1.x, e1.y, e1.z), E2 = along_max3(e2.x, e2.y, e2.z),
                 X = along_max3(x.x, x.y, x.z), D = along_max3(nx, ny, nz);
    if (!(V0 < 1e30 && E1 < 1e30 && E2 < 1e30 && X < 1e30)) return t;                // (false for NaN)
    const double ux = (double)e2.y * nz - (double)e2.z * ny, uy = (double)e2.z * nx - (double)e2.x * nz, uz = (double)e2.x * ny - (double)e2.y * nx;
    const double vx = ny * (double)e1.z - nz * (double)e1.y, vy = nz * (double)e1.x - nx * (double)e1.z, vz = nx * (double)e1.y - ny * (double)e1.x;
    const double den = (double)x.x * nx + (double)x.y * ny + (double)x.z * nz;
    const double Mb = ((double)a.smax + V0) * (1.0 + 1e-6);
    const double m_u = ldexp(Mb * E2 * D, -18), m_v = ldexp(Mb * E1 * D, -18), m_d = ldexp(X * D, -20), a0 = ldexp(1.0, -80);
    if (!(fabs(den) >= 64.0 * m_d) || den == 0.0) return t;
    const double s = den > 0.0 ? 1.0 : -1.0;
    const double c1 = a.c1, c2 = a.c2;
    const double gam_u = along_sel(ux, uy, uz, a.k1) * c1 + along_sel(ux, uy, uz, a.k2) * c2 + along_sel(ux, uy, uz, a.k);
    const double gam_v = along_sel(vx, vy, vz, a.k1) * c1 + along_sel(vx, vy, vz, a.k2) * c2 + along_sel(vx, vy, vz, a.k);
    t.au = s * along_sel(ux, uy, uz, a.k1); t.bu = s * along_sel(ux, uy, uz, a.k2);
    t.av = s * along_sel(vx, vy, vz, a.k1); t.bv = s * along_sel(vx, vy, vz, a.k2);
    t.tu = m_u + a0 + fabs(gam_u) * Mb;
    t.tv = m_v + a0 + fabs(gam_v) * Mb;
    t.tw = fabs(den) * (1.0 + ldexp(1.0, -22)) + m_u + m_v + 2.0 * m_d + a0 + (fabs(gam_u) + fabs(gam_v)) * Mb;
    const double aw = t.au + t.av, bw = t.bu + t.bv;
    const double lu = fabs(t.au) + fabs(t.bu), lv = fabs(t.av) + fabs(t.bv), lw = fabs(aw) + fabs(bw);
    const double det = t.au * t.bv - t.av * t.bu;
    if (!(fabs(det) >= ldexp(fmax(fmax(lu * lv, lu * lw), lv * lw), -30)) || det == 0.0) return t;
    // the region's corners, local to v0's projection
    const double gu[3] = { -t.tu, -t.tu, t.tw + t.tv }, gv[3] = { -t.tv, t.tw + t.tu, -t.tv };
    double xl = INFINITY, xh = -INFINITY, yl = INFINITY, yh = -INFINITY;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double px = (t.bv * gu[c] - t.bu * gv[c]) / det, py = (-t.av * gu[c] + t.au * gv[c]) / det;
        xl = fmin(xl, px); xh = fmax(xh, px); yl = fmin(yl, py); yh = fmax(yh, py);
    }
    const double grow = ldexp(fmax(fmax(fabs(xl), fabs(xh)), fmax(fabs(yl), fabs(yh))), -20);
    t.pv = (double)along_sel(v0, a.k1) - c1 * (double)along_sel(v0, a.k);
    t.qv = (double)along_sel(v0, a.k2) - c2 * (double)along_sel(v0, a.k);
    // every start the region holds computes a cell coordinate within pad of [gl, gh]: inside the grid, or the triangle is for everyone
    const double gil = (t.pv + xl - grow - (double)a.p0) * (double)a.ip - a.pad, gih = (t.pv + xh + grow - (double)a.p0) * (double)a.ip + a.pad;
    const double gjl = (t.qv + yl - grow - (double)a.q0) * (double)a.iq - a.pad, gjh = (t.qv + yh + grow - (double)a.q0) * (double)a.iq + a.pad;
    if (!(gil >= 0.0 && gih < (double)a.B && gjl >= 0.0 && gjh < (double)a.B)) return t;      // (false for NaN)
    t.i0 = (int)gil; t.i1 = (int)gih; t.j0 = (int)gjl; t.j1 = (int)gjh;
    const double hx = a.dhat[0], hy = a.dhat[1], hz = a.dhat[2];
    const double d0 = (double)v0.x * hx + (double)v0.y * hy + (double)v0.z * hz;
    const double d1 = d0 + ((double)e1.x * hx + (double)e1.y * hy + (double)e1.z * hz), d2 = d0 + ((double)e2.x * hx + (double)e2.y * hy + (double)e2.z * hz);
    t.near = (float)(fmin(d0, fmin(d1, d2)) - 2.0 * (double)a.sigma);
    t.kind = ALONG_CELLS;
    return t;
}

// Whether a start whose computed cell is (i, j) can lie in the triangle's region: the corner test of the three edge functions over
// the cell grown by pad (rt_binned.hpp: rect_may_hit is the model) -- the largest s pu and s qv and the smallest s (pu + qv) over the
// rectangle against their thresholds.
MIRT_HD bool along_cell_may_hit(const AlongDesc &a, const AlongTri &t, int i, int j)
{
    const double x0 = (double)a.p0 + ((double)i - a.pad) * a.wp - t.pv, x1 = (double)a.p0 + ((double)(i + 1) + a.pad) * a.wp - t.pv;
    const double y0 = (double)a.q0 + ((double)j - a.pad) * a.wq - t.qv, y1 = (double)a.q0 + ((double)(j + 1) + a.pad) * a.wq - t.qv;
    const double aw = t.au + t.av, bw = t.bu + t.bv;
    const double gu_max = t.au * (t.au > 0.0 ? x1 : x0) + t.bu * (t.bu > 0.0 ? y1 : y0);
    const double gv_max = t.av * (t.av > 0.0 ? x1 : x0) + t.bv * (t.bv > 0.0 ? y1 : y0);
    const double gw_min = aw * (aw > 0.0 ? x0 : x1) + bw * (bw > 0.0 ? y0 : y1);
    return gu_max >= -t.tu && gv_max >= -t.tv && gw_min <= t.tw;
}

// ---- the tables, and the kernels' parameter blocks -------------------------------------------------------------------------------------
// Row e of the structure: the triangle's QueryRow (the 41-operation test needs nothing else) and beside it the triangle's index and
// depth bound.
struct AlongAux { uint32_t tri; float near; };

struct AlongView {
    AlongDesc d;
    const uint32_t *off;         // along_keys + 1: first row of every (cell, shell) key; the every-ray list is cell B * B, shell 0
    const QueryRow *rows;        // never NULL: a lane with no row left still loads row 0
    const AlongAux *aux;
};

// The build: one lane per triangle files it (k_along_pairs), bucket_sort_pairs orders the pairs, k_along_rows expands them.
struct AlongPairs {
    AlongDesc d;
    const QueryRow *qrows;
    int n;
    uint32_t *counters;          // [0] pairs, [1] triangles on the every-ray list
    uint32_t *keys, *vals;
    uint32_t cap;
    uint32_t *bucket_cnt;        // nbuckets counts for bucket_sort_pairs (../csrc/bin_sort.hpp)
    uint32_t nbuckets;
    int bucket_shift;
    float *near;                 // n: the triangles' depth bounds, for k_along_rows
};
struct AlongRows {
    const uint32_t *entries;     // the triangles in key order
    const uint32_t *total;       // their number
    const QueryRow *qrows;
    const float *near;
    QueryRow *rows;
    AlongAux *aux;
};

// A call: the scene's rows (q.rays is not read: the starts are `origins`, the direction is `dir` as the caller gave it), the
// structure, and for occlusion the limits and bytes.
struct AlongFrame {
    QueryFrame q;
    AlongView v;
    const float *origins;        // nrays x 3
    float dir[3];
    const float *limit;          // k_along_occluded: nrays limits or NULL
    uint8_t *occluded;           // k_along_occluded: nrays bytes
    unsigned long long *stats;   // QSTAT_WORDS counters (the STATS instantiations): rays, rows offered, rows tested, rays that swept
};
// The rays written out for the brute-force kernels: ray i = { origins[3 i ..], dir }.
struct AlongExpand {
    const float *origins;
    float dir[3];
    int nrays;
    float *rays;                 // nrays x RAY_WORDS
};

__attribute__((global)) void k_along_pairs(const AlongPairs);
__attribute__((global)) void k_along_rows(const AlongRows);
__attribute__((global)) void k_along_expand(const AlongExpand);
template <bool STATS> __attribute__((global)) void k_along_closest(const AlongFrame);
template <bool STATS> __attribute__((global)) void k_along_occluded(const AlongFrame);

}  // namespace mirt
