// rt_query.hpp -- parameter blocks and declarations of the ray-query kernels (rt_query.hip): ClosestIntersection
// (raytracer.cpp:202-257) and DirectLight (:265-327) for rays and hit records the CALLER supplies, one call per ray / per record,
// instead of the pinhole camera's rays the frame kernels generate themselves.
#pragma once

#include "../csrc/rt_common.hpp"
#include "../csrc/rt_binned.hpp"
#include "light_passes.hpp"
#include "light_mask.hpp"

#include <string.h>

namespace mirt {

// What ClosestIntersection computes per triangle before it looks at the ray (:216-217, :225): 12 floats,
//   a = { v0.x, v0.y, v0.z, e1.x }   b = { e1.y, e1.z, e2.x, e2.y }   c = { e2.z, e1e2.x, e1e2.y, e1e2.z }
// e1 = v1 - v0, e2 = v2 - v0, e1e2 = cross(e1, e2): the same operations on the same operands as the reference runs per call, so
// building them once changes no bit.  48 bytes, read as three 16-byte LDS broadcasts per test like an OriginRow.
struct QueryRow { float4 a, b, c; };
static_assert(sizeof(QueryRow) == 48, "query row must be 48 bytes");

// Words of the scene-wide maxima k_query_rows leaves beside the rows: the largest |component| of v0, e1, e2 and e1e2 as float
// BITS (non-negative floats order like unsigned integers; a NaN component is larger than every finite one).
enum { QMAX_V0 = 0, QMAX_E1 = 1, QMAX_E2 = 2, QMAX_E1E2 = 3, QMAX_WORDS = 4 };

// Bounds of a ray the pre-reject filter may run on (the frame path's, rt_frame.cpp: operands_safe): every component of `start`
// below 1e8 and of `dir` below 1e6 in magnitude; anything else, NaN included, takes the exact-only path.
#define MIRT_QUERY_START_MAX 1.0e8f
#define MIRT_QUERY_DIR_MAX 1.0e6f

// struct Intersection (raytracer.cpp:91-96) as five 32-bit words: position, distance, triangleIndex.
constexpr int HIT_WORDS = 5;
constexpr int RAY_WORDS = 6;                      // start, dir

struct QueryFrame {
    const QueryRow *rows;       // n rows
    int n;
    const uint32_t *scene_max;  // QMAX_WORDS words
    int scene_finite;           // every vertex coordinate below 1e8 in magnitude (host side, mirt_scene_upload)
    const float *rays;          // nrays x RAY_WORDS
    int nrays;
    uint32_t *hits;             // nrays x HIT_WORDS, in/out
};

// DirectLight for `nhits` records: f carries the scene, the light positions / colours, the light origin tables (k_prep_origin)
// and their `unsafe` flag; nothing of f that describes a view or an output plane is read.
// A call of more than MIRT_MAX_LIGHTS positions runs as several passes (light_passes.hpp; the CARRY instantiations of the kernels):
// f holds the pass's own f.nlights <= MIRT_MAX_LIGHTS positions, `first` says where they stand in the call's list, and the
// accumulators travel from pass to pass in `carry`.  The kernels of a call of one pass read none of the three.
// The MASK instantiations (mirt_shadow_mask*) write the shadow decisions of the pass's positions into `mask` (light_mask.hpp)
// and nothing else: they read a record's position only, `first` in every call, and neither rgb nor carry; k_query_relight
// (mirt_direct_light_masked*) reads `mask` and writes rgb.
struct QueryLightFrame {
    RtFrame f;
    const uint32_t *hits;       // nhits x HIT_WORDS: position and index are read
    int nhits;
    float *rgb;                 // nhits x 3
    int first;                  // global index of the pass's position 0
    float *carry;               // LIGHT_CARRY_WORDS planes of nhits floats: result, result2
    int pass_flags;             // LIGHT_PASS_FIRST | LIGHT_PASS_LAST
    uint32_t *mask;             // light_mask_words(positions of the call) planes of nhits words
    unsigned long long *stats;  // QSTAT_WORDS counters of the sweep's MASK + STATS instantiation (the binned kernels': QueryBinnedFrame)
};

// DirectLight for `nhits` records with every shadow ray walking its light-cube bin (k_query_direct_light_binned): q.f.light_tab
// is the CUBE's origin table (k_select_faces: one row per (light position, triangle)), which the records the bins do not cover
// sweep instead; the rest is what the trace kernel of a binned frame reads of a light cube (capi.hpp: LightCache).
enum { QSTAT_SHADOW_RAYS = 0, QSTAT_CANDIDATES = 1, QSTAT_TESTS = 2, QSTAT_FALLBACK = 3, QSTAT_WORDS = 4 };
// What a walk kernel reads of a light cube (capi.hpp: LightCache; made by cube_view, query.cpp).  light_rows is never NULL: a lane
// with no row left still loads row 0.
struct CubeView {
    const uint32_t *light_off;          // positions * 6 * B * B * shells + 1: first row of every (bin, shell) key
    const LightRow *light_rows;         // the candidates' origin rows in key order, `far` in r2.w (k_expand_light_rows)
    const uint32_t *light_tri;          // the triangle of each row
    const BinFrameDesc *light_frames;   // 6 per position: shell_d0 / shell_iw of the position's depth shells
    int cube_bins, shells;
};
struct QueryBinnedFrame {
    QueryLightFrame q;
    CubeView cube;
    unsigned long long *stats;          // QSTAT_WORDS counters (the STATS instantiation only)
};

// DirectLight with the shadow ray of every (record, position) replaced by its bit of q.mask (k_query_relight): all npos <=
// MIRT_MAX_LIGHT_POSITIONS positions in one launch.  lights: npos rows of six floats, lpos then lcol as RtFrame holds them for a
// pass; of q.f only tris15, n and samples are read, and of q hits, nhits, mask and rgb.
struct QueryRelightFrame {
    QueryLightFrame q;
    const float *lights;        // npos x 6
    int npos;
};

// ---- origin fans: ClosestIntersection for many directions from ONE origin (mirt_intersect_from*) ---------------------------
//
// The cube around the origin is a ray family of directions whose largest component is 1 (rt_binned.hpp: negD ~ s e_k + u e_k1 +
// v e_k2, dmax = 2); a caller's direction has any length.  fan_dir_of scales negD by a power of two so that its largest component
// lies in [0.5, 1): d' = negD * 2^k.  The bin is chosen from d'; every test runs on negD itself.
//
// Why the bin of d' holds every triangle the reference accepts for negD (DESIGN.md section 5.1 has the full argument).  The row
// operands of the three dots are below 2^57 (scene_finite and the origin below 1e8: 8e16), so with the largest |negD| component in
// [2^(FAN_EXP_MIN - 1), 2^FAN_EXP_MAX) no product or sum overflows (below 2^78), and multiplying by 2^k commutes with every rounding
// whose result is normal: the dots of negD are 2^-k times the dots of d', bit for bit, and the quotients t, u, v -- hence the
// verdict -- are the same.  Subnormal results: a sum of two floats that lands in the subnormal range is exact; a product that
// does is off by at most 2^-150 of its own scale, so the dots of negD, scaled by 2^k, are the dots of d' up to the ordinary
// rounding of a dot product plus at most 3 * 2^-150 * (1 + 2^k) <= 2^-116 -- both inside the margin the edge functions of
// section 3.2 carry (2^-17 M dmax + 2^-20).  The absolute thresholds of the accept test in units of d': u >= 0 lets a < 0 pass
// only when |a| / D underflows, |a'| < 2^-150 D' < 2^-91, likewise v and t: tighter than the 2^-22 the margins were sized for.
// The upper end keeps negD inside the filter's own range (MIRT_QUERY_DIR_MAX = 1e6 > 2^19), so maybe_hit needs no override on
// a lane that takes a bin.  Outside the window -- zero, NaN, infinite, tiny or huge -- a ray takes no bin and sweeps the table.
constexpr int FAN_EXP_MIN = -31;                  // largest |component| = f * 2^e with f in [0.5, 1): e in [FAN_EXP_MIN, FAN_EXP_MAX],
constexpr int FAN_EXP_MAX = 19;                   // i.e. 2^-32 <= largest |component| < 2^19

struct FanDir { int formed; v3 d; };
MIRT_HD uint32_t fan_bits(float x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __float_as_uint(x);
#else
    uint32_t u; memcpy(&u, &x, 4); return u;
#endif
}
// formed: every component finite and the largest inside the window; d = nd * 2^k then, each component the correctly rounded
// product (exact unless a component more than 2^107 below the largest drops into the subnormal range under k < 0: that moves
// (u, v) of the bin by less than 2^-125, the bins' pad is 2^-18).  Signs and zero components are kept.  Not formed: d = nd.
// (The largest component is found on the integer bits: a NaN or infinity orders above every finite value and has exponent
// field 255, outside the window like zero and the subnormals with field 0.)
MIRT_HD FanDir fan_dir_of(v3 nd)
{
    const uint32_t bx = fan_bits(nd.x) & 0x7fffffffu, by = fan_bits(nd.y) & 0x7fffffffu, bz = fan_bits(nd.z) & 0x7fffffffu;
    const uint32_t bm = bx > by ? (bx > bz ? bx : bz) : (by > bz ? by : bz);
    const int E = (int)(bm >> 23);                // largest |component| in [2^(E - 127), 2^(E - 126)): e = E - 126
    FanDir r;
    r.formed = (int)(E >= FAN_EXP_MIN + 126) & (int)(E <= FAN_EXP_MAX + 126);
    const uint32_t sb = (uint32_t)(253 - (r.formed ? E : 126)) << 23;          // 2^(126 - E) = 2^k; 1.0 when not formed
#ifdef __HIP_DEVICE_COMPILE__
    const float s = __uint_as_float(sb);
#else
    float s; memcpy(&s, &sb, 4);
#endif
    r.d = r.formed ? V3(nd.x * s, nd.y * s, nd.z * s) : nd;
    return r;
}

// One origin, nrays directions, the in/out records.  tab: the origin's table, one row per triangle (the cube's own, written by
// k_select_faces, or the query's, written by k_prep_origin); the cube is read by the binned walk (rt_query.hip: fan_walk) only.
struct QueryFanFrame {
    const float *tris15;
    int n;
    const OriginRow *tab;
    const uint32_t *unsafe;             // k_query_fan: != 0 runs every test through the exact path
    float origin[3];
    const float *dirs;                  // nrays x 3, used as given
    int nrays;
    uint32_t *hits;                     // nrays x HIT_WORDS, in/out
    CubeView cube;                      // the cube around the origin: one position
    unsigned long long *stats;          // QSTAT_WORDS counters (the STATS instantiation only): rays, rows offered, rows tested, rays that swept
};

// ---- origin fans from MANY origins in one call (mirt_intersect_fans*) ---------------------------------------------------------
//
// One pass of the call: the cube `f.cube` holds the origins [first, first + count) of the call's list as its positions 0 .. count - 1
// (capi.hpp: LightCache for a many-position list, as DirectLight's), and ray i belongs to the pass when origin_of[i] lies in that
// range.  k_query_fans_binned hands the walk of k_query_fan_binned (rt_query.hip: fan_walk) per lane what that kernel has per launch:
// the position k = origin_of[i] - first, S = origins[3 (1 + k) ..] (the cube's own list: slot 0 is the camera's place), the bin base
// k * 6 B B and the sweep table f.tab + k * n; the shell descriptor is cube.light_frames[6 k].  f.origin and f.unsafe are not read.
struct QueryFansFrame {
    QueryFanFrame f;
    const float *origins;               // (1 + count) x 3: the cube's origin list
    const int32_t *origin_of;           // nrays indices into the CALL's origins; NULL: every ray takes origin 0
    int first, count;                   // the pass's range of the call's origins
};

// The rays of such a call written out for k_query_closest*: ray i = { origins[3 origin_of[i] ..], dirs[3 i ..] }, RAY_WORDS words
// each; an index outside [0, norigins) gives a ray no triangle accepts (k_query_fans_expand).
struct QueryFansExpand {
    const float *origins;               // norigins x 3
    int norigins;
    const int32_t *origin_of;           // nrays, or NULL: origin 0
    const float *dirs;                  // nrays x 3
    int nrays;
    float *rays;                        // nrays x RAY_WORDS
};

// ---- occlusion queries (mirt_occluded*): one byte per ray, 1 when some accepted triangle has distance < limit ---------------------
//
// q.hits is not read: the answer of ray i goes to occluded[i], 0 or 1, for every i in [0, nrays).
struct QueryOccludedFrame {
    QueryFrame q;
    const float *limit;                 // nrays limits, used as given; NULL: every limit is +inf
    uint8_t *occluded;                  // nrays bytes
};
// One pass of the many-origin form through the cube (k_query_occluded_fans_binned): QueryFansFrame's fields as k_query_fans_binned
// reads them, f.f.hits apart.  norigins is the CALL's origin count: the pass with first == 0 writes the 0 of every ray whose index
// lies outside [0, norigins), which belongs to no pass.
struct QueryOccludedFansFrame {
    QueryFansFrame f;
    int norigins;
    const float *limit;                 // nrays, or NULL: +inf
    uint8_t *occluded;                  // nrays bytes; a pass writes its own rays' only
};

// Rays (hits) per workgroup of the lane-per-ray kernels: 256 lanes x P.
constexpr int QUERY_P = 2;
constexpr int QUERY_BLOCK_RAYS = 256 * QUERY_P;

__attribute__((global)) void k_query_rows(const float *, int, QueryRow *, uint32_t *);
template <int P> __attribute__((global)) void k_query_closest(const QueryFrame);
__attribute__((global)) void k_query_closest_wave(const QueryFrame);
template <int P, bool CARRY = false, bool MASK = false, bool STATS = false> __attribute__((global)) void k_query_direct_light(const QueryLightFrame);
constexpr int QUERY_BIN_P = 1;                    // records per lane of the binned DirectLight kernel: lists differ per lane
template <int P, bool STATS = false, bool CARRY = false, bool MASK = false> __attribute__((global)) void k_query_direct_light_binned(const QueryBinnedFrame);
__attribute__((global)) void k_query_relight(const QueryRelightFrame);
template <int P> __attribute__((global)) void k_query_fan(const QueryFanFrame);
template <bool STATS> __attribute__((global)) void k_query_fan_binned(const QueryFanFrame);
template <bool STATS> __attribute__((global)) void k_query_fans_binned(const QueryFansFrame);
__attribute__((global)) void k_query_fans_expand(const QueryFansExpand);
template <int P> __attribute__((global)) void k_query_occluded(const QueryOccludedFrame);
__attribute__((global)) void k_query_occluded_wave(const QueryOccludedFrame);
template <bool STATS> __attribute__((global)) void k_query_occluded_fans_binned(const QueryOccludedFansFrame);

}  // namespace mirt
