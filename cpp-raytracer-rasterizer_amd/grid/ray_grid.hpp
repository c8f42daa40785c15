// ray_grid.hpp -- arbitrary rays through a cell grid (mirt_set_ray_grid: mirt_intersect*, mirt_occluded* on rays that share neither
// origin nor direction).  What the structure is, the predicate that files a triangle into it and the walk that says which keys a ray
// reads (host and device: the one text, MIRT_HD), and the parameter blocks of the kernels (ray_grid.hip).  DESIGN.md section 5.1 has
// the argument in full; its steps stand beside the code they justify.
//
// The reference accepts a triangle on computed u, v, t (raytracer.cpp:237-239), so a (ray, triangle) pair is one of two kinds.  With
// d' = negD scaled into [0.5, 1) (rt_query.hpp: fan_dir_of), den^ = e1e2 . d' as the reference rounds it and tau a threshold of the
// triangle:
//   well-conditioned, |den^| >= tau:  an accepted pair's line passes within rho of a point of the triangle, ahead of the start --
//       the triangle is found in a CELL the ray passes through (G x G x G cells, every triangle filed in the cells its box grown by
//       rho touches);
//   ill-conditioned, |den^| < tau:    the signs of u, v, t are rounding noise and the reference may accept a triangle the ray never
//       comes near -- but only when the ray's direction lies within kappa of the triangle's plane and its start within h of it: the
//       triangle is found in the PLANE INDEX, keyed by the plane's dominant axis k, its slopes (alpha, beta) and its offset delta
//       (x_k = alpha x_k1 + beta x_k2 + delta).
// Triangles whose thresholds are too wide for either (needles, zero areas, anything not finite) go on the EVERY-RAY list.
// All geometry of the filing and of the walk is computed in double from the float operands: a product of two floats is exact there,
// and what is left (2^-50 of a bin) is covered by GRID_PAD.
#pragma once

#include "../query/rt_query.hpp"

#include <math.h>

namespace mirt {

constexpr int GRID_CELLS_MIN = 4, GRID_CELLS_MAX = 128;
constexpr int GRID_PLANE_BINS = 64;              // (alpha, beta) bins per side and class; first choice, not swept
constexpr int GRID_OFFSET_BINS = 64;             // delta bins; first choice, not swept
constexpr double GRID_RHO_CELLS = 0.25;          // rho in cells: a whole cell multiplies a soup triangle's pairs by about five; not swept
constexpr double GRID_START_EXTENTS = 2.0;       // smax in units of the scene's extent R = the largest |coordinate| of its bounding box
constexpr double GRID_PLANE_SPAN = 1.25;         // the (alpha, beta) bins cover [-1.25, 1.25]: |alpha|, |beta| <= 1 and a reach of 0.125
constexpr double GRID_PLANE_REACH_MAX = 0.125;   // a triangle whose reach 5 kappa in (alpha, beta) is wider is for every ray
constexpr int GRID_PLANE_KEYS_MAX = 512;         // ... or whose neighbourhood holds more plane-index keys than this
constexpr int GRID_CELL_KEYS_MAX = 32768;        // ... or whose grown box touches more cells than this
constexpr double GRID_DIR_MIN = 0.2;             // a class is walked when the larger of |d'_k1|, |d'_k2| reaches this (else |n . d'| >= 0.1)
constexpr double GRID_PAD = 9.313225746154785e-10;      // 2^-30 of a bin, on both sides: the doubles' own rounding is 2^-40 of a bin at most
constexpr double GRID_FLOAT_PAD_MAX = 0.125;     // a grid whose cells a FLOAT could not tell apart this well is not built (the frame path's rule)
constexpr int GRID_EVERY_SHARE = 8, GRID_EVERY_FLOOR = 64;      // the along grids' rule for giving up

// Cells per side for n triangles: the smallest power of two with G^3 >= 2 n, within [GRID_CELLS_MIN, GRID_CELLS_MAX].  Not swept.
inline int grid_cells_for(int n)
{
    int G = GRID_CELLS_MIN;
    while (G < GRID_CELLS_MAX && (long long)G * G * G < 2ll * (long long)n) G *= 2;
    return G;
}
inline int grid_every_cap(int n) { return n / GRID_EVERY_SHARE > GRID_EVERY_FLOOR ? n / GRID_EVERY_SHARE : GRID_EVERY_FLOOR; }

// ---- the structure's descriptor: a function of (the scene's bounding box, G) alone -------------------------------------------------
// Key space: cells (x * G + y) * G + z from 0, the plane index ((k * PB + alpha bin) * PB + beta bin) * DB + delta bin from
// key_plane (delta minor: the delta range of an (alpha, beta) bin is one contiguous run), then the one key of the every-ray list.
struct GridDesc {
    int G, PB, DB;
    double lo[3];                // the grid's corner: cell coordinate of x along axis c is (x - lo[c]) * inv
    double w, inv;               // the cells' width (cubes) and 1 / w
    double rho;                  // GRID_RHO_CELLS * w
    double grow;                 // what a triangle's box is grown by: rho and the slack of the accepted point
    double smax;                 // a ray takes the walk while every |component| of its start is <= smax
    double Mb;                   // >= every |component| of b = start - v0 for such a start
    double d_lo, d_inv;          // delta bin of x: (x - d_lo) * d_inv, clamped
    double pw, pinv;             // width of an (alpha, beta) bin and its inverse
    double pad;                  // GRID_PAD: what every bin coordinate is moved by before its floor, in the filing and in the walk
    uint32_t key_plane, key_every, nkeys;
};

MIRT_HD double grid_sel(double x, double y, double z, int k) { return k == 0 ? x : (k == 1 ? y : z); }
MIRT_HD double grid_max3(double a, double b, double c) { return fmax(fmax(fabs(a), fabs(b)), fabs(c)); }
// floor(x) as an int clamped into [lo, hi] (x finite)
MIRT_HD int grid_bin(double x, int lo, int hi)
{
    const double f = floor(x);
    return f < (double)lo ? lo : (f > (double)hi ? hi : (int)f);
}

// The descriptor over the box [lo3, hi3]; false when no structure is built: a box that is not finite or smaller than 2^-60, or cells
// finer than a float resolves at the distance of the box and of the starts.
inline bool grid_make_desc(const float *lo3, const float *hi3, int G, GridDesc *out)
{
    GridDesc d;
    memset(&d, 0, sizeof d);
    double R = 0.0, ext = 0.0;
    for (int c = 0; c < 3; c++) {
        if (!(fabsf(lo3[c]) < MIRT_QUERY_START_MAX && fabsf(hi3[c]) < MIRT_QUERY_START_MAX && lo3[c] <= hi3[c])) return false;
        R = fmax(R, fmax(fabs((double)lo3[c]), fabs((double)hi3[c])));
        ext = fmax(ext, (double)hi3[c] - (double)lo3[c]);
    }
    if (!(R >= ldexp(1.0, -60))) return false;
    d.G = G; d.PB = GRID_PLANE_BINS; d.DB = GRID_OFFSET_BINS;
    d.smax = GRID_START_EXTENTS * R;
    d.Mb = (d.smax + R) * (1.0 + 1e-6);
    // G - 1 cells span the box and the accepted point's slack: half a cell is left on every side, for rho (a quarter) and the pads
    const double slack = ldexp(d.Mb, -20);
    d.w = (fmax(ext, ldexp(R, -10)) + 2.0 * slack) / (double)(G - 1);
    d.inv = 1.0 / d.w;
    d.rho = GRID_RHO_CELLS * d.w;
    d.grow = d.rho * (1.0 + ldexp(1.0, -10)) + slack;
    double far = 0.0;
    for (int c = 0; c < 3; c++) {
        d.lo[c] = 0.5 * ((double)lo3[c] + (double)hi3[c]) - 0.5 * (double)G * d.w;
        far = fmax(far, fabs(d.lo[c]));
    }
    // (the walk computes in double and needs none of this: the rule keeps the grid to the scenes the other structures bin)
    const double float_pad = ldexp(1.0, -20) * (d.inv * (d.smax + far) + (double)G);
    if (!(float_pad <= GRID_FLOAT_PAD_MAX)) return false;
    // |delta| = |v0_k - alpha v0_k1 - beta v0_k2| <= 3 R; beyond the ends the bins are clamped on both sides
    d.d_lo = -3.5 * R;
    d.d_inv = (double)d.DB / (7.0 * R);
    d.pw = 2.0 * GRID_PLANE_SPAN / (double)d.PB;
    d.pinv = 1.0 / d.pw;
    d.pad = GRID_PAD;
    d.key_plane = (uint32_t)G * (uint32_t)G * (uint32_t)G;
    d.key_every = d.key_plane + 3u * (uint32_t)(d.PB * d.PB) * (uint32_t)d.DB;
    d.nkeys = d.key_every + 1u;
    *out = d;
    return true;
}
inline uint32_t grid_keys(int G) { return (uint32_t)G * (uint32_t)G * (uint32_t)G + 3u * (uint32_t)(GRID_PLANE_BINS * GRID_PLANE_BINS) * (uint32_t)GRID_OFFSET_BINS + 1u; }

// ---- the filing predicate -----------------------------------------------------------------------------------------------------------
//
// Per triangle, from the row the reference's own operations leave (v0, e1, e2, X = e1e2 as FLOATS: QueryRow).  u = 2^-24; Mb bounds
// |b| = |start - v0| per component, E1, E2, X are the largest |component| of e1, e2, e1e2, and |d'| <= 1.  N = e1 x e2 exactly;
// |X - N| <= 6.01 u E1 E2 per component.  The reference's float dots differ from the exact ones of its own rounded b by at most
//     |den^ - X . d'| <= 9.01 u X          |T^ - X . b| <= 9.01 u X Mb          |U^ - U| <= 36.1 u Mb E2          |V^ - V| <= 36.1 u Mb E1
// (along.hpp derives the same bounds), a0 = 2^-80 standing for results that are subnormal under negD's own scale.
//
// Well-conditioned.  Cramer: b (N . d') = U e1 + V e2 + T d' exactly.  With the real quotients t* = T^ / den^, u* = U^ / den^, v* = V^ / den^
//     (S' - t* d') - (v0 + u* e1 + v* e2) = (b (den^ - N . d') - (U^ - U) e1 - (V^ - V) e2 - (T^ - T) d') / den^,       S' = v0 + b,
// per component at most u Mb (18.02 X + 108.3 E1 E2) / |den^|; Err = u Mb (32 X + 128 E1 E2) + a0 (...) is taken.  An accepted pair has
// t*, u*, v* >= -2^-149 and u* + v* <= 1 + 2^-22, so the point S' - t* d' of the ray, ahead of the start, lies within Err / |den^| of
// the triangle's box grown by 2^-22 (E1 + E2): with |den^| >= tau = Err / rho it lies in the box grown by `grow`, in a cell the
// triangle is filed in -- and the walk visits every cell the exact ray passes through.
//
// Ill-conditioned, |den^| < tau.  Acceptance forces |U^|, |V^| <= |den^| (1 + 2^-22), so
//     |X . d'| < tau + m_d            |U| < eu = tau (1 + 2^-22) + m_u            |V| < ev = tau (1 + 2^-22) + m_v,
// and the component of Cramer's identity along d's largest (>= 0.5) gives |N . b| <= 2 ((tau + m_d + m_x) Mb + eu E1 + ev E2), m_x =
// 2^-19 E1 E2 covering X - N.  With n = X / X_k = e_k - alpha e_k1 - beta e_k2 (k the dominant axis of X) and delta0 = n . v0:
//     |n . d'| < kappa = (tau + m_d) / |X_k|             |n . S - delta0| < h = H / |X_k|.
// A ray in the triangle's plane has alpha d_k1 + beta d_k2 = d_k, a line in (alpha, beta); with the larger of |d_k1|, |d_k2| at least
// GRID_DIR_MIN that line passes within 5 kappa of (alpha0, beta0) along the coordinate it is solved for -- at q, in a bin the ray
// visits -- and delta(q) = S_k - alpha S_k1 - beta S_k2 differs from delta0 by at most h + 5 kappa smax.  The triangle is filed in
// every bin its square of half-width 5 kappa and that delta interval touch.  (When both |d_k1|, |d_k2| < GRID_DIR_MIN, |d_k| >= 0.5
// and |n . d'| >= 0.5 - 0.4 > kappa: no triangle of class k is ill-conditioned for the ray, and the class is not walked.)
// Cells, refined.  The ray's point lies within rho + slack of a point of the triangle's PLANE too (the accepted point v0 + u* e1 + v* e2
// lies in the plane through v0 of normal N; X differs from N by m_x), so it lies in no cell of the grown box whose centre c has
// |X . (c - v0)| > |X|_1 (w / 2 + pad w + grow) + 2^-19 E1 E2 (E1 + E2): such a cell is not filed (grid_cell_near_plane).
enum { GRID_FILED = 0, GRID_EVERY = 1 };
struct GridTri {
    int kind;
    int c0[3], c1[3];            // the cells of the grown box, inclusive
    int k;                       // the dominant axis of the normal
    int a0, a1, b0, b1, o0, o1;  // the plane index's bins, inclusive
    double nx, ny, nz, n0, nthr; // the plane slab of the cells: |n . c - n0| <= nthr for a cell's centre c
};
// The thresholds of a triangle: kappa and h of the text above (infinite or NaN when it has none: not finite, X all zero).
struct GridThresholds { double tau, kappa, h; };
MIRT_HD GridThresholds grid_tri_thresholds(const GridDesc &d, v3 v0, v3 e1, v3 e2, v3 x)
{
    GridThresholds q;
    q.tau = q.kappa = q.h = INFINITY;
    const double V0 = grid_max3(v0.x, v0.y, v0.z), E1 = grid_max3(e1.x, e1.y, e1.z), E2 = grid_max3(e2.x, e2.y, e2.z), X = grid_max3(x.x, x.y, x.z);
    if (!(V0 < 1e30 && E1 < 1e30 && E2 < 1e30 && X < 1e30) || !(X > 0.0)) return q;          // (false for NaN)
    const double Mb = d.Mb, a0 = ldexp(1.0, -80);
    const double err = ldexp(Mb * (32.0 * X + 128.0 * E1 * E2), -24) + a0 * (Mb + 1.0 + E1 + E2);
    const double m_d = ldexp(X, -20) + a0, m_x = ldexp(E1 * E2, -19), m_u = ldexp(Mb * E2, -18) + a0, m_v = ldexp(Mb * E1, -18) + a0;
    q.tau = err / d.rho;
    q.kappa = (q.tau + m_d) / X;
    const double eu = q.tau * (1.0 + ldexp(1.0, -22)) + m_u, ev = q.tau * (1.0 + ldexp(1.0, -22)) + m_v;
    q.h = (2.0 * ((q.tau + m_d + m_x) * Mb + eu * E1 + ev * E2) + m_x * Mb + ldexp(X * Mb, -22)) / X;
    return q;
}

// The bins of a triangle whose direction and start thresholds are kappa and h (grid_tri_setup passes grid_tri_thresholds'; the tests
// also file a structure without margins, to see it miss).
MIRT_HD GridTri grid_tri_file(const GridDesc &d, v3 v0, v3 e1, v3 e2, v3 x, double kappa, double h)
{
    GridTri t;
    t.kind = GRID_EVERY;
    t.k = 0;
    t.a0 = t.b0 = t.o0 = 0; t.a1 = t.b1 = t.o1 = -1;
    t.c0[0] = t.c0[1] = t.c0[2] = 0; t.c1[0] = t.c1[1] = t.c1[2] = -1;
    t.nx = t.ny = t.nz = t.n0 = t.nthr = 0.0;
    const double pad = d.pad, reach = 5.0 * kappa;
    if (!(reach <= GRID_PLANE_REACH_MAX) || !(h < INFINITY)) return t;                       // (false for NaN)
    const double ax = fabs((double)x.x), ay = fabs((double)x.y), az = fabs((double)x.z);
    const int k = ax >= ay && ax >= az ? 0 : (ay >= az ? 1 : 2), k1 = (k + 1) % 3, k2 = (k + 2) % 3;
    const double xk = grid_sel(x.x, x.y, x.z, k);
    const double alpha = -grid_sel(x.x, x.y, x.z, k1) / xk, beta = -grid_sel(x.x, x.y, x.z, k2) / xk;
    const double delta = grid_sel(v0.x, v0.y, v0.z, k) - alpha * grid_sel(v0.x, v0.y, v0.z, k1) - beta * grid_sel(v0.x, v0.y, v0.z, k2);
    const double hp = h + reach * d.smax;
    t.k = k;
    t.a0 = grid_bin((alpha - reach + GRID_PLANE_SPAN) * d.pinv - pad, 0, d.PB - 1);
    t.a1 = grid_bin((alpha + reach + GRID_PLANE_SPAN) * d.pinv + pad, 0, d.PB - 1);
    t.b0 = grid_bin((beta - reach + GRID_PLANE_SPAN) * d.pinv - pad, 0, d.PB - 1);
    t.b1 = grid_bin((beta + reach + GRID_PLANE_SPAN) * d.pinv + pad, 0, d.PB - 1);
    t.o0 = grid_bin((delta - hp - d.d_lo) * d.d_inv - pad, 0, d.DB - 1);
    t.o1 = grid_bin((delta + hp - d.d_lo) * d.d_inv + pad, 0, d.DB - 1);
    if ((t.a1 - t.a0 + 1) * (t.b1 - t.b0 + 1) * (t.o1 - t.o0 + 1) > GRID_PLANE_KEYS_MAX) return t;
    // the cells of the box of v0, v0 + e1, v0 + e2 (the accepted point is v0 + u e1 + v e2 of these very floats), grown
    const double grow = d.grow;
    long long cells = 1;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double p = grid_sel(v0.x, v0.y, v0.z, c), q1 = p + grid_sel(e1.x, e1.y, e1.z, c), q2 = p + grid_sel(e2.x, e2.y, e2.z, c);
        const double bl = fmin(p, fmin(q1, q2)) - grow, bh = fmax(p, fmax(q1, q2)) + grow;
        t.c0[c] = grid_bin((bl - d.lo[c]) * d.inv - pad, 0, d.G - 1);
        t.c1[c] = grid_bin((bh - d.lo[c]) * d.inv + pad, 0, d.G - 1);
        cells *= (long long)(t.c1[c] - t.c0[c] + 1);
    }
    if (cells > GRID_CELL_KEYS_MAX) return t;
    const double E1 = grid_max3(e1.x, e1.y, e1.z), E2 = grid_max3(e2.x, e2.y, e2.z);
    t.nx = x.x; t.ny = x.y; t.nz = x.z;
    t.n0 = t.nx * (double)v0.x + t.ny * (double)v0.y + t.nz * (double)v0.z;
    t.nthr = ((ax + ay + az) * ((0.5 + pad) * d.w + grow) + ldexp(E1 * E2 * (E1 + E2), -19)) * (1.0 + ldexp(1.0, -30));
    t.kind = GRID_FILED;
    return t;
}
MIRT_HD GridTri grid_tri_setup(const GridDesc &d, v3 v0, v3 e1, v3 e2, v3 x)
{
    const GridThresholds q = grid_tri_thresholds(d, v0, e1, e2, x);
    return grid_tri_file(d, v0, e1, e2, x, q.kappa, q.h);
}

// Whether cell (cx, cy, cz) of the grown box lies within the triangle's plane slab.
MIRT_HD bool grid_cell_near_plane(const GridDesc &d, const GridTri &t, int cx, int cy, int cz)
{
    const double x = d.lo[0] + ((double)cx + 0.5) * d.w, y = d.lo[1] + ((double)cy + 0.5) * d.w, z = d.lo[2] + ((double)cz + 0.5) * d.w;
    return fabs(t.nx * x + t.ny * y + t.nz * z - t.n0) <= t.nthr;
}

// How many keys the triangle is filed under, and each of them to f(key) -- the one enumeration of the count pass, the write pass
// and the tests.
MIRT_HD uint32_t grid_tri_cell_keys(const GridDesc &d, const GridTri &t)
{
    uint32_t n = 0u;
    for (int cx = t.c0[0]; cx <= t.c1[0]; cx++)
        for (int cy = t.c0[1]; cy <= t.c1[1]; cy++)
            for (int cz = t.c0[2]; cz <= t.c1[2]; cz++) n += grid_cell_near_plane(d, t, cx, cy, cz) ? 1u : 0u;
    return n;
}
MIRT_HD uint32_t grid_tri_plane_keys(const GridTri &t) { return (uint32_t)((t.a1 - t.a0 + 1) * (t.b1 - t.b0 + 1) * (t.o1 - t.o0 + 1)); }
template <class F>
MIRT_HD void grid_tri_keys(const GridDesc &d, const GridTri &t, F &&f)
{
    if (t.kind == GRID_EVERY) { f(d.key_every); return; }
    for (int cx = t.c0[0]; cx <= t.c1[0]; cx++)
        for (int cy = t.c0[1]; cy <= t.c1[1]; cy++)
            for (int cz = t.c0[2]; cz <= t.c1[2]; cz++)
                if (grid_cell_near_plane(d, t, cx, cy, cz)) f((uint32_t)((cx * d.G + cy) * d.G + cz));
    for (int a = t.a0; a <= t.a1; a++)
        for (int b = t.b0; b <= t.b1; b++)
            for (int o = t.o0; o <= t.o1; o++) f(d.key_plane + (uint32_t)(((t.k * d.PB + a) * d.PB + b) * d.DB + o));
}

// ---- the walk: which runs of keys a ray reads, in order -------------------------------------------------------------------------------
//
// A ray is fit for the walk when its direction is inside the fans' window (fan_dir_of: finite, not zero, largest component in
// [2^-32, 2^19)) and every component of its start is finite and within smax; any other ray sweeps all n rows.
MIRT_HD bool grid_ray_fit(const GridDesc &d, v3 S, v3 dir)
{
    const FanDir fd = fan_dir_of(V3(-dir.x, -dir.y, -dir.z));
    return fd.formed && fabs((double)S.x) <= d.smax && fabs((double)S.y) <= d.smax && fabs((double)S.z) <= d.smax;      // (false for NaN)
}

// Cells, slab by slab along the direction's dominant axis `ax` (|slope| <= 1 across it, the cells are cubes: within one slab the ray
// moves at most one cell along each other axis, so the cells of its piece are a block of at most 3 x 3 with the pads -- computed
// afresh per slab from the start, no incremental state).  The first slab is the start's (t* >= -2^-149: the accepted point is not
// behind it by more than the pad), clipped to the grid.  Before a later slab is entered, every slab before it has been walked: a
// triangle not offered yet has its ray point S' - t* d' -- which lies in a cell the triangle is filed in AND the ray visits -- at
// or beyond the entry face.  Its accepted point, the float one distance3 measures to, lies within Err / |den^| <= rho of that per
// component, plus the slack: not nearer than |face - S_ax| - grow along ax.  So its float distance exceeds `reach` = the record's
// distance (the limit) times 1 + 2^-20 whenever reach < |face - S_ax| - grow, and the cells end there.
// Then the plane index, class by class: for each bin of the parameter coordinate the bins the line's segment touches in the
// solved coordinate (at most 3) and the delta bins between the segment's ends, one run of keys each.  Then the every-ray list.
struct GridWalk {
    double sx, sy, sz, dx, dy, dz;   // the start; the direction of travel, scaled (-d')
    int phase;                       // 0 cells, 1..3 plane class phase - 1, 4 every-ray list, 5 through
    int i, iend, step;               // slab / parameter bin, where it ends (exclusive), +-1
    int j, j1, k0, k1, k;            // cells: block cursor; planes: solved-bin cursor j..j1, delta bins k0..k1
    int ax;                          // cells: the dominant axis
    int solved_alpha;                // planes: the line is solved for alpha over bins of beta (else the other way round)
    double p0, p1, p2;               // cells: the slopes across ax and the start's cell coordinate along it; planes: s(x) = (p0 - x p1) * p2
};

MIRT_HD void grid_walk_slab(const GridDesc &d, GridWalk &w)
{
    const int a1 = (w.ax + 1) % 3, a2 = (w.ax + 2) % 3;
    const double c1 = w.p0, c2 = w.p1, ga = w.p2;
    // the ray's piece inside the slab, in cell coordinates along ax: from the entry face (or the start) to the exit face
    const double f0 = (double)w.i, f1 = (double)(w.i + 1);
    const double ua = w.step > 0 ? fmax(f0, ga) : fmin(f1, ga), ub = w.step > 0 ? f1 : f0;
    const double g1 = (grid_sel(w.sx, w.sy, w.sz, a1) - d.lo[a1]) * d.inv, g2 = (grid_sel(w.sx, w.sy, w.sz, a2) - d.lo[a2]) * d.inv;
    const double y0 = g1 + (ua - ga) * c1, y1 = g1 + (ub - ga) * c1, z0 = g2 + (ua - ga) * c2, z1 = g2 + (ub - ga) * c2;
    const double yl = floor(fmin(y0, y1) - d.pad), yh = floor(fmax(y0, y1) + d.pad);
    const double zl = floor(fmin(z0, z1) - d.pad), zh = floor(fmax(z0, z1) + d.pad);
    const double top = (double)(d.G - 1);
    const bool none = yl > top || yh < 0.0 || zl > top || zh < 0.0;
    w.j = none ? 0 : (int)fmax(yl, 0.0);
    w.j1 = none ? -1 : (int)fmin(yh, top);
    w.k0 = none ? 0 : (int)fmax(zl, 0.0);
    w.k1 = none ? -1 : (int)fmin(zh, top);
    w.k = w.k0;
}

// The parameter bin w.i of plane class w.phase - 1: the solved coordinate's bins j..j1 and the delta bins k0..k1 (none: j > j1).
MIRT_HD void grid_walk_plane_bin(const GridDesc &d, GridWalk &w)
{
    const int kk = w.phase - 1, k1 = (kk + 1) % 3, k2 = (kk + 2) % 3;
    const double x0 = -GRID_PLANE_SPAN + (double)w.i * d.pw, x1 = -GRID_PLANE_SPAN + (double)(w.i + 1) * d.pw;
    const double s0 = (w.p0 - x0 * w.p1) * w.p2, s1 = (w.p0 - x1 * w.p1) * w.p2;
    const double sl = floor((fmin(s0, s1) + GRID_PLANE_SPAN) * d.pinv - d.pad), sh = floor((fmax(s0, s1) + GRID_PLANE_SPAN) * d.pinv + d.pad);
    const double top = (double)(d.PB - 1);
    const bool none = sl > top || sh < 0.0;
    w.j = none ? 0 : (int)fmax(sl, 0.0);
    w.j1 = none ? -1 : (int)fmin(sh, top);
    const double Sk = grid_sel(w.sx, w.sy, w.sz, kk), S1 = grid_sel(w.sx, w.sy, w.sz, k1), S2 = grid_sel(w.sx, w.sy, w.sz, k2);
    const double e0 = w.solved_alpha ? Sk - s0 * S1 - x0 * S2 : Sk - x0 * S1 - s0 * S2;
    const double e1 = w.solved_alpha ? Sk - s1 * S1 - x1 * S2 : Sk - x1 * S1 - s1 * S2;
    w.k0 = grid_bin((fmin(e0, e1) - d.d_lo) * d.d_inv - d.pad, 0, d.DB - 1);
    w.k1 = grid_bin((fmax(e0, e1) - d.d_lo) * d.d_inv + d.pad, 0, d.DB - 1);
}

// Enters plane class `cls` (0..2), or the every-ray list for cls == 3.
MIRT_HD void grid_walk_class(const GridDesc &d, GridWalk &w, int cls)
{
    for (; cls < 3; cls++) {
        const int k1 = (cls + 1) % 3, k2 = (cls + 2) % 3;
        const double dk = grid_sel(w.dx, w.dy, w.dz, cls), d1 = grid_sel(w.dx, w.dy, w.dz, k1), d2 = grid_sel(w.dx, w.dy, w.dz, k2);
        if (!(fmax(fabs(d1), fabs(d2)) >= GRID_DIR_MIN)) continue;
        w.phase = 1 + cls;
        w.solved_alpha = fabs(d1) >= fabs(d2) ? 1 : 0;
        w.p0 = dk;
        w.p1 = w.solved_alpha ? d2 : d1;
        w.p2 = 1.0 / (w.solved_alpha ? d1 : d2);
        w.i = -1; w.iend = d.PB; w.step = 1;
        w.j = 0; w.j1 = -1;
        return;
    }
    w.phase = 4;
}

MIRT_HD GridWalk grid_walk_begin(const GridDesc &d, v3 S, v3 dir, bool fit)
{
    GridWalk w;
    w.sx = S.x; w.sy = S.y; w.sz = S.z;
    const FanDir fd = fan_dir_of(V3(-dir.x, -dir.y, -dir.z));
    w.dx = -(double)fd.d.x; w.dy = -(double)fd.d.y; w.dz = -(double)fd.d.z;
    w.phase = 5;
    w.i = w.iend = 0; w.step = 1;
    w.j = w.k0 = w.k = 0; w.j1 = w.k1 = -1;
    w.ax = 0; w.solved_alpha = 0;
    w.p0 = w.p1 = w.p2 = 0.0;
    if (!fit) return w;
    const double ax = fabs(w.dx), ay = fabs(w.dy), az = fabs(w.dz);
    w.ax = ax >= ay && ax >= az ? 0 : (ay >= az ? 1 : 2);
    w.step = grid_sel(w.dx, w.dy, w.dz, w.ax) > 0.0 ? 1 : -1;
    const double ga = (grid_sel(w.sx, w.sy, w.sz, w.ax) - d.lo[w.ax]) * d.inv;
    const double da = grid_sel(w.dx, w.dy, w.dz, w.ax);
    w.p0 = grid_sel(w.dx, w.dy, w.dz, (w.ax + 1) % 3) / da;
    w.p1 = grid_sel(w.dx, w.dy, w.dz, (w.ax + 2) % 3) / da;
    w.p2 = ga;
    const double fi = floor(w.step > 0 ? ga - d.pad : ga + d.pad);
    const double top = (double)(d.G - 1);
    w.phase = 0;
    if (w.step > 0) { w.i = fi < 0.0 ? 0 : (fi > top ? d.G : (int)fi); w.iend = d.G; }
    else { w.i = fi > top ? d.G - 1 : (fi < 0.0 ? -1 : (int)fi); w.iend = -1; }
    if (w.i == w.iend) grid_walk_class(d, w, 0);
    else grid_walk_slab(d, w);
    return w;
}

// One step of the walk: GRID_STEP_RUN with the next run of keys [*kf, *kl] the ray reads, GRID_STEP_MOVED when the step only moved
// the state on (to the next slab, parameter bin or class: straight-line work, so that the lanes of a wave step together whatever
// part of the walk each is in), GRID_STEP_DONE when the ray is through.  reach: see above (+inf walks everything).
enum { GRID_STEP_DONE = 0, GRID_STEP_RUN = 1, GRID_STEP_MOVED = 2 };
MIRT_HD int grid_walk_step(const GridDesc &d, GridWalk &w, double reach, uint32_t *kf, uint32_t *kl)
{
    if (w.phase == 0) {
        if (w.j <= w.j1) {
            const int a1 = (w.ax + 1) % 3, a2 = (w.ax + 2) % 3;
            const int st0 = d.G * d.G, st1 = d.G;
            const int sa = w.ax == 0 ? st0 : (w.ax == 1 ? st1 : 1), s1 = a1 == 0 ? st0 : (a1 == 1 ? st1 : 1), s2 = a2 == 0 ? st0 : (a2 == 1 ? st1 : 1);
            *kf = *kl = (uint32_t)(w.i * sa + w.j * s1 + w.k * s2);
            if (++w.k > w.k1) { w.k = w.k0; w.j++; }
            return GRID_STEP_RUN;
        }
        w.i += w.step;
        bool more = w.i != w.iend;
        if (more) {
            const double face = d.lo[w.ax] + (double)(w.step > 0 ? w.i : w.i + 1) * d.w;
            more = !(reach < fabs(face - grid_sel(w.sx, w.sy, w.sz, w.ax)) - d.grow);
        }
        if (more) grid_walk_slab(d, w);
        else grid_walk_class(d, w, 0);
        return GRID_STEP_MOVED;
    }
    if (w.phase <= 3) {
        if (w.j <= w.j1) {
            const int a = w.solved_alpha ? w.j : w.i, b = w.solved_alpha ? w.i : w.j;
            const uint32_t base = d.key_plane + (uint32_t)((((w.phase - 1) * d.PB + a) * d.PB + b) * d.DB);
            *kf = base + (uint32_t)w.k0;
            *kl = base + (uint32_t)w.k1;
            w.j++;
            return GRID_STEP_RUN;
        }
        if (++w.i < w.iend) grid_walk_plane_bin(d, w);
        else grid_walk_class(d, w, w.phase);
        return GRID_STEP_MOVED;
    }
    if (w.phase == 4) {
        *kf = *kl = d.key_every;
        w.phase = 5;
        return GRID_STEP_RUN;
    }
    return GRID_STEP_DONE;
}
// The next run of keys; false when the ray is through (the host's loop over grid_walk_step).
inline bool grid_walk_next(const GridDesc &d, GridWalk &w, double reach, uint32_t *kf, uint32_t *kl)
{
    for (;;) {
        const int r = grid_walk_step(d, w, reach, kf, kl);
        if (r != GRID_STEP_MOVED) return r == GRID_STEP_RUN;
    }
}

// ---- the tables, and the kernels' parameter blocks ------------------------------------------------------------------------------------
struct GridView {
    GridDesc d;
    const uint32_t *off;         // nkeys + 1: first row of every key
    const QueryRow *rows;        // the rows in key order; never NULL: a lane with no row left still loads row 0
    const uint32_t *tri;         // the triangle of each row
};

// The build: one lane per triangle files it (k_grid_pairs), bucket_sort_pairs orders the pairs, k_grid_rows expands them.
struct GridPairs {
    GridDesc d;
    const QueryRow *qrows;
    int n;
    uint32_t *counters;          // [0] pairs, [1] triangles on the every-ray list, [2] pairs of the plane index, [4..5] the pairs as 64 bits
    uint32_t *keys, *vals;
    uint32_t cap;
    uint32_t *bucket_cnt;        // nbuckets counts for bucket_sort_pairs (../csrc/bin_sort.hpp)
    uint32_t nbuckets;
    int bucket_shift;
};
struct GridRows {
    const uint32_t *entries;     // the triangles in key order
    const uint32_t *total;       // their number
    const QueryRow *qrows;
    QueryRow *rows;
};

// The counters of the STATS instantiations.
enum { GSTAT_RAYS = 0, GSTAT_ROWS_CELLS = 1, GSTAT_ROWS_PLANES = 2, GSTAT_ROWS_EVERY = 3, GSTAT_TESTS = 4, GSTAT_SWEPT = 5, GSTAT_WORDS = 6 };

// A call: the scene's rows, the caller's rays and records (q), the structure, and for occlusion the limits and bytes.
struct GridFrame {
    QueryFrame q;
    GridView v;
    const float *limit;          // k_grid_occluded: nrays limits or NULL
    uint8_t *occluded;           // k_grid_occluded: nrays bytes
    unsigned long long *stats;   // GSTAT_WORDS counters (the STATS instantiations)
};

__attribute__((global)) void k_grid_pairs(const GridPairs);
__attribute__((global)) void k_grid_rows(const GridRows);
template <bool STATS> __attribute__((global)) void k_grid_closest(const GridFrame);
template <bool STATS> __attribute__((global)) void k_grid_occluded(const GridFrame);

}  // namespace mirt
