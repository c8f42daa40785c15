// shadowed.hpp -- covers_whole: whether ONE triangle U hides the whole of a triangle T from a light position S, so that every
// shadow ray DirectLight casts from a hit point on T (raytracer.cpp:294-315) is known to end occluded before it is cast.  Decided
// once per (triangle, position) when the shared light cube is built (rt_trace.hip: k_shadowed_table); the trace kernel then gives
// such a pixel D = (0, 0, 0) without a ray.  DESIGN.md section 3.2 has the proof; tests/cpp/covers_whole_test.cpp runs the
// reference's arithmetic against every verdict.
#pragma once

#include "rt_common.hpp"

namespace mirt {

// The margins every inequality of sure_hit (rt_common.hpp) must hold by, relative to the sums of the absolute products of its dot
// product -- not to the result, so that cancellation does not eat them.  Two sums, because the roundings are of two kinds:
//  * normalize and the three dots err relative to the direction's own components: below 2^-21 of sum |row_c| |S_c - v_c|.
//    COVER_MARGIN_DIR = 2^-10 is 2048 times that bound;
//  * the hit point v0 + u*e1 + v*e2 and lightPos - pos err relative to the COORDINATES (|S_c| + max |v_c|, which on a scene placed far
//    from the origin are much larger than their differences): below 2^-19 of sum |row_c| (|S_c| + max |v_c|) with room for a few ulp
//    more per coordinate, a few 2^-24 of it in practice.  COVER_MARGIN_POS = 2^-12 is 128 times the bound, a thousand times the practice.
constexpr double COVER_MARGIN_DIR = 0.0009765625, COVER_MARGIN_POS = 0.000244140625;
// ... and the sums themselves must not be tiny (relative to the largest coordinate magnitude, which bounds the length the direction is
// divided by): with the margins, what the kernel compares is then >= 1e-34, a normal number, and a single product that is denormal or
// flushed beside a large one errs by 2^-126 at most.
constexpr double COVER_FLOOR = 1.0e-30;

MIRT_HD bool cover_in_range(v3 a) { return fabsf(a.x) < MIRT_SAFE_MAG && fabsf(a.y) < MIRT_SAFE_MAG && fabsf(a.z) < MIRT_SAFE_MAG; }   // false for NaN

// U: the occluder's origin row for light position S with origin_far(U, S) in r2.w (as k_select_faces files it and the cube's rows
// carry it); t0, t1, t2: the vertices of T.  True only when the reference is certain to accept U for the shadow ray of EVERY hit
// point it can compute on T, at a distance below 0.99 r: anything not provable -- NaN, Inf, an unsafe row, U edge-on, T degenerate or
// touching S, U == T or sharing a vertex or an edge with it -- is false, which costs time only.
MIRT_HD bool covers_whole(const OriginRow &U, v3 t0, v3 t1, v3 t2, v3 S)
{
    if (!origin_row_safe(U) || !cover_in_range(t0) || !cover_in_range(t1) || !cover_in_range(t2) || !cover_in_range(S)) return false;
    // the distance test (:313) for every r on T: no point of U is farther from S than `far`, no hit point on T closer than `near`,
    // each with its own slack (origin_far, origin_near), and rounding is monotone: fl(0.99f * r) >= fl(0.99f * near) > far
    const float far = U.r2.w, near = origin_near(t0, t1, t2, S);
    if (!(far > 0.0f && far < 0.99f * near)) return false;                   // (false for NaN, and for a word that is no distance)
    const v3 n = cross3(sub3(t1, t0), sub3(t2, t0));
    if (!(n.x != 0.0f || n.y != 0.0f || n.z != 0.0f)) return false;            // T has no area
    // sure_hit's inequalities are linear and homogeneous in the direction: holding, with the margin, for the directions from T's
    // three vertices to S they hold for every direction of T's cone.  In double: the rows' floats are the very coefficients the
    // kernel's dots use, and the products and sums below are then exact to 2^-50.
    const double Q[3] = { (double)fabsf(S.x) + (double)fmaxf(fmaxf(fabsf(t0.x), fabsf(t1.x)), fabsf(t2.x)),
                          (double)fabsf(S.y) + (double)fmaxf(fmaxf(fabsf(t0.y), fabsf(t1.y)), fabsf(t2.y)),
                          (double)fabsf(S.z) + (double)fmaxf(fmaxf(fabsf(t0.z), fabsf(t1.z)), fabsf(t2.z)) };
    const double Md = fabs((double)U.r0.x) * Q[0] + fabs((double)U.r0.y) * Q[1] + fabs((double)U.r0.z) * Q[2];
    const double Mu = fabs((double)U.r1.x) * Q[0] + fabs((double)U.r1.y) * Q[1] + fabs((double)U.r1.z) * Q[2];
    const double Mv = fabs((double)U.r2.x) * Q[0] + fabs((double)U.r2.y) * Q[1] + fabs((double)U.r2.z) * Q[2];
    const double floor_ = COVER_FLOOR * fmax(fmax(Q[0], Q[1]), Q[2]);
    if (!(Md > floor_ && Mu > floor_ && Mv > floor_)) return false;
    const v3 tv[3] = { t0, t1, t2 };
    double s = 0.0;
    for (int i = 0; i < 3; i++) {
        const double wx = (double)S.x - (double)tv[i].x, wy = (double)S.y - (double)tv[i].y, wz = (double)S.z - (double)tv[i].z;
        const double den = (double)U.r0.x * wx + (double)U.r0.y * wy + (double)U.r0.z * wz;
        const double pu = (double)U.r1.x * wx + (double)U.r1.y * wy + (double)U.r1.z * wz;
        const double qv = (double)U.r2.x * wx + (double)U.r2.y * wy + (double)U.r2.z * wz;
        // the margins: COVER_MARGIN_DIR of the absolute products with this direction, COVER_MARGIN_POS of those with the coordinates' magnitudes
        const double ax = fabs(wx), ay = fabs(wy), az = fabs(wz);
        const double md = COVER_MARGIN_DIR * (fabs((double)U.r0.x) * ax + fabs((double)U.r0.y) * ay + fabs((double)U.r0.z) * az) + COVER_MARGIN_POS * Md;
        const double mu = COVER_MARGIN_DIR * (fabs((double)U.r1.x) * ax + fabs((double)U.r1.y) * ay + fabs((double)U.r1.z) * az) + COVER_MARGIN_POS * Mu;
        const double mv = COVER_MARGIN_DIR * (fabs((double)U.r2.x) * ax + fabs((double)U.r2.y) * ay + fabs((double)U.r2.z) * az) + COVER_MARGIN_POS * Mv;
        if (i == 0) s = den < 0.0 ? -1.0 : 1.0;                               // e1e2d's sign: the same from all three vertices, or false
        const double D = s * den, a = s * pu, b = s * qv;
        if (!(D >= md && a >= mu && b >= mv && D - (a + b) >= md + mu + mv)) return false;
    }
    if (!(fabsf(U.r0.w) <= 3.402823466e+38f)) return false;                   // (e1e2b is outside origin_row_safe's range check: Inf and NaN here)
    return s * (double)U.r0.w > 0.0;                                          // t = e1e2b / e1e2d > 0: S is off U's plane, on the side the rays leave from
}

}  // namespace mirt
