// count_device.hpp -- what every kernel of the hit counts does around its integer (device code; count_hits.hip and count_walk.hpp): what
// a ray reads of the call's `after` record and limit, and a row of the scene tested and counted.  Every (ray, triangle) test is
// k_query_closest's own (../query/rt_query_device.hpp: ray_dots, the conservative filter maybe_hit with the per-ray exact-only
// override, exact_hit_row) on the caller's start and negD = -dir; an accepted distance goes through count_rule.hpp's predicate.
#pragma once

#include "count_hits.hpp"
#include "../query/rt_query_device.hpp"

namespace mirt {

// What ray `ray` counts behind and below: the caller's `after` record (distance and index) and limit, +inf for no limit array; `open`
// is false for a lane without a ray and for a ray nothing can count for (count_open) -- such a lane reads no row.
struct CountRay {
    bool has_after, open;
    float a, L;
    int k;
};
__device__ __forceinline__ CountRay count_ray_of(const CountOut &o, long long ray, bool ok)
{
    CountRay c;
    c.has_after = o.after != nullptr;
    c.a = -1.0f;
    c.k = 0;
    if (ok && o.after) {
        const uint32_t *r = o.after + (size_t)HIT_WORDS * ray;
        c.a = __uint_as_float(r[3]);
        c.k = (int)r[4];
    }
    c.L = occlusion_limit(o.limit, ray, ok);
    c.open = ok && count_open(c.has_after, c.a, c.L);
    return c;
}

// An accepted distance of triangle `tri`: 1 when it counts.
__device__ __forceinline__ int count_hit(const CountRay &c, float dist, int tri) { return (int)count_admits(dist, tri, c.has_after, c.a, c.k, c.L); }

// Row `tri` of a sweep for a lane that is `on`: the filter with the exact-only override in front of the exact test.
__device__ __forceinline__ int count_row(const CountRay &c, const RowVecs &r, int tri, v3 S, v3 nd, bool on, bool exact_only)
{
    float e1e2b;
    const TestDots td = ray_dots(r, S, nd, &e1e2b);
    int hit = 0;
    if (on && (maybe_hit(td) || exact_only)) {
        v3 hp;
        float dist;
        if (exact_hit_row(td, e1e2b, r, S, &hp, &dist)) hit = count_hit(c, dist, tri);
    }
    return hit;
}

__device__ __forceinline__ int wave_sum32(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

}  // namespace mirt
