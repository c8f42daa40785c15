// rt_query.hpp -- parameter blocks and declarations of the ray-query kernels (rt_query.hip): ClosestIntersection
// (raytracer.cpp:202-257) and DirectLight (:265-327) for rays and hit records the CALLER supplies, one call per ray / per record,
// instead of the pinhole camera's rays the frame kernels generate themselves.
#pragma once

#include "../csrc/rt_common.hpp"
#include "../csrc/rt_binned.hpp"

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
struct QueryLightFrame {
    RtFrame f;
    const uint32_t *hits;       // nhits x HIT_WORDS: position and index are read
    int nhits;
    float *rgb;                 // nhits x 3
};

// DirectLight for `nhits` records with every shadow ray walking its light-cube bin (k_query_direct_light_binned): q.f.light_tab
// is the CUBE's origin table (k_select_faces: one row per (light position, triangle)), which the records the bins do not cover
// sweep instead; the rest is what the trace kernel of a binned frame reads of a light cube (capi.hpp: LightCache).
enum { QSTAT_SHADOW_RAYS = 0, QSTAT_CANDIDATES = 1, QSTAT_TESTS = 2, QSTAT_FALLBACK = 3, QSTAT_WORDS = 4 };
struct QueryBinnedFrame {
    QueryLightFrame q;
    const uint32_t *light_off;          // nlights * 6 * B * B * shells + 1: first row of every (bin, shell) key
    const LightRow *light_rows;         // the candidates' origin rows in key order, `far` in r2.w (k_expand_light_rows)
    const uint32_t *light_tri;          // the triangle of each row
    const BinFrameDesc *light_frames;   // 6 per light position: shell_d0 / shell_iw of the position's depth shells
    int cube_bins, shells;
    unsigned long long *stats;          // QSTAT_WORDS counters (the STATS instantiation only)
};

// Rays (hits) per workgroup of the lane-per-ray kernels: 256 lanes x P.
constexpr int QUERY_P = 2;
constexpr int QUERY_BLOCK_RAYS = 256 * QUERY_P;

__attribute__((global)) void k_query_rows(const float *, int, QueryRow *, uint32_t *);
template <int P> __attribute__((global)) void k_query_closest(const QueryFrame);
__attribute__((global)) void k_query_closest_wave(const QueryFrame);
template <int P> __attribute__((global)) void k_query_direct_light(const QueryLightFrame);
constexpr int QUERY_BIN_P = 1;                    // records per lane of the binned DirectLight kernel: lists differ per lane
template <int P, bool STATS = false> __attribute__((global)) void k_query_direct_light_binned(const QueryBinnedFrame);

}  // namespace mirt
