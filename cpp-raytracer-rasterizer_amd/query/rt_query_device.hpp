// rt_query_device.hpp -- device helpers of the ray-query kernels (rt_query.hip) that kernels outside that file use as well
// (../lights/aa_many_lights.hip): the filter range of a direction, the LDS staging of a row chunk, the record's words, the
// sequential record rule, and the row walk of a cube's list.  Their text is the one rt_query.hip has always compiled.
#pragma once

#include "rt_query.hpp"

namespace mirt {

// The ray's part of the filter's range: every |dir| component below MIRT_QUERY_DIR_MAX (false for NaN).  A ray outside it has
// its filter verdicts overridden, per ray.
__device__ __forceinline__ bool dir_in_filter_range(v3 d)
{
    return fabsf(d.x) < MIRT_QUERY_DIR_MAX && fabsf(d.y) < MIRT_QUERY_DIR_MAX && fabsf(d.z) < MIRT_QUERY_DIR_MAX;
}

// A chunk of `cnt` 48-byte rows (QueryRow, OriginRow: three float4 each) into LDS, by the whole workgroup of 256 between two barriers.
template <class Row>
__device__ __forceinline__ void stage_rows(float4 *s_rows, const Row *rows, int cnt)
{
    static_assert(sizeof(Row) == 48, "rows are staged as three float4");
    __syncthreads();
    const float4 *src = reinterpret_cast<const float4 *>(rows);
    for (int k = threadIdx.x; k < cnt * 3; k += 256) s_rows[k] = src[k];
    __syncthreads();
}

// struct Intersection (raytracer.cpp:91-96) to its HIT_WORDS words: position, distance (as bits), triangleIndex.
__device__ __forceinline__ void store_record(uint32_t *h, v3 pos, uint32_t dist_bits, uint32_t tri)
{
    h[0] = __float_as_uint(pos.x); h[1] = __float_as_uint(pos.y); h[2] = __float_as_uint(pos.z);
    h[3] = dist_bits;
    h[4] = tri;
}

// The in/out `closestIntersection` of a ray while one lane sees the triangles in index order: the reference's own sequential
// update, `if (record.distance >= distance)` (:243), started from the incoming record -- which is what the packed min-t key
// encodes (rt_common.hpp) and needs no key here: ties go to the later index, an incoming record loses every tie, a negative or
// NaN incoming distance is never replaced and +inf by any hit.  The state -- distance, index (-1: still the incoming record),
// position, whether anything replaced the record -- stays in the kernels' own registers.
template <class Flag>
__device__ __forceinline__ void closest_offer(float &best_d, int &best_i, v3 &pos, Flag &replaced, float dist, int tri, v3 hp)
{
    if (best_d >= dist) { best_d = dist; best_i = tri; pos = hp; replaced = Flag(1); }   // :243-247
}

// The step of a cube walk: on to row e + 1 where the lane continues (`cont`), else to the list's end and row 0 -- loaded and
// ignored, so that every step is straight-line code for every lane (CubeView: the row table is never NULL).
__device__ __forceinline__ void walk_row(const float4 *rows4, uint32_t e, float4 &c0, float4 &c1, float4 &c2)
{
    const float4 *src = rows4 + (size_t)e * 3;
    c0 = src[0]; c1 = src[1]; c2 = src[2];
}
__device__ __forceinline__ void walk_step(const float4 *rows4, uint32_t &e, uint32_t end, int cont, float4 &c0, float4 &c1, float4 &c2)
{
    e = cont ? e + 1u : end;
    walk_row(rows4, cont ? e : 0u, c0, c1, c2);
}

// First row and end of the list a ray from position k walks: the bin of direction d (fan_dir_of's d') among the bins from bin_base
// on, its shells up to the one distance x falls into.  Returns the list's key, the index of its first shell in light_off.
__device__ __forceinline__ uint32_t fan_list(const CubeView &cv, uint32_t k, uint32_t bin_base, v3 d, float x, uint32_t *e, uint32_t *end)
{
    const BinFrameDesc *lf = cv.light_frames + 6 * (size_t)k;
    const uint32_t key = cube_bin_of(d, bin_base, cv.cube_bins) * (uint32_t)cv.shells;
    *e = cv.light_off[key];
    *end = cv.light_off[key + bin_shell_of(x, lf->shell_d0, lf->shell_iw, cv.shells) + 1u];
    return key;
}

// The origin of lane `ray` in one pass of a many-origin call (rt_query.hip: k_query_fans_binned's paragraph): whether the ray is the pass's at all, and the
// position k, origin S, first bin and sweep table of a ray that is -- position 0's for one that is not.  idx is the ray's index as
// the caller gave it.
struct FansLane { bool mine; uint32_t idx, k, bin_base; v3 S; const OriginRow *tab; };
__device__ __forceinline__ FansLane fans_lane(const QueryFansFrame &qf, long long ray, bool ok)
{
    const QueryFanFrame &q = qf.f;
    const uint32_t face_bins = (uint32_t)(q.cube.cube_bins * q.cube.cube_bins) * 6u;
    FansLane l;
    l.idx = qf.origin_of ? (uint32_t)qf.origin_of[ok ? ray : 0] : 0u;
    const uint32_t rel = l.idx - (uint32_t)qf.first;               // (modulo 2^32: a negative or huge index lands beyond count)
    l.mine = ok && rel < (uint32_t)qf.count;
    l.k = l.mine ? rel : 0u;
    l.bin_base = l.k * face_bins;
    l.S = ld3(qf.origins + 3 * (size_t)(1u + l.k));
    l.tab = q.tab + (size_t)l.k * q.n;
    return l;
}

// ---- the row test of the caller's own rays, shared by rt_query.hip and ../along/along.hip ------------------------------------------

// Whether the rows of the scene are inside the filter's range for every start below MIRT_QUERY_START_MAX (rt_query.hip's header
// comment); wave-uniform: four scalar loads and a handful of scalar-unit operations.
__device__ __forceinline__ bool scene_rows_in_range(const QueryFrame &q)
{
    const float V = __uint_as_float(q.scene_max[QMAX_V0]), E1 = __uint_as_float(q.scene_max[QMAX_E1]),
                E2 = __uint_as_float(q.scene_max[QMAX_E2]), X = __uint_as_float(q.scene_max[QMAX_E1E2]);
    const float B = MIRT_QUERY_START_MAX + V;
    // (comparisons are false for NaN: a NaN anywhere in the scene sends every ray down the exact path)
    return q.scene_finite && 2.0f * B * E1 < MIRT_SAFE_MAG && 2.0f * B * E2 < MIRT_SAFE_MAG && X < MIRT_SAFE_MAG;
}

// A ray whose operands are not provably inside the filter's range: it takes the exact path for every triangle.
__device__ __forceinline__ bool ray_exact_only(bool scene_ok, v3 start, v3 dir)
{
    const bool in_range = fabsf(start.x) < MIRT_QUERY_START_MAX && fabsf(start.y) < MIRT_QUERY_START_MAX && fabsf(start.z) < MIRT_QUERY_START_MAX &&
                          dir_in_filter_range(dir);
    return !(scene_ok && in_range);
}

// The incoming distance of ray `ray` -- a lane without a ray carries a record nothing can replace.
__device__ __forceinline__ float incoming_distance(const uint32_t *hits, long long ray, bool ok)
{
    return ok ? __uint_as_float(hits[(size_t)HIT_WORDS * ray + 3]) : -1.0f;
}

// The limit of an occlusion ray: a lane without a ray carries one nothing is below; a missing limit array stands for +inf.
__device__ __forceinline__ float occlusion_limit(const float *limit, long long ray, bool ok)
{
    return !ok ? -1.0f : (limit ? limit[ray] : __uint_as_float(0x7f800000u));
}

struct RowVecs { v3 v0, e1, e2, e1e2; };
__device__ __forceinline__ RowVecs unpack_row(const float4 &a, const float4 &b, const float4 &c)
{
    RowVecs r;
    r.v0 = V3(a.x, a.y, a.z); r.e1 = V3(a.w, b.x, b.y); r.e2 = V3(b.z, b.w, c.x); r.e1e2 = V3(c.y, c.z, c.w);
    return r;
}

// One ray against one row: b, be2, e1b, e1e2b (:218, :226-227, :231), then the three dots against negD (:232-234).
__device__ __forceinline__ TestDots ray_dots(const RowVecs &r, v3 start, v3 nd, float *e1e2b)
{
    const v3 b = sub3(start, r.v0);
    const v3 be2 = cross3(b, r.e2), e1b = cross3(r.e1, b);
    *e1e2b = r.e1e2.x * b.x + r.e1e2.y * b.y + r.e1e2.z * b.z;
    TestDots d;
    d.den = r.e1e2.x * nd.x + r.e1e2.y * nd.y + r.e1e2.z * nd.z;
    d.pu = be2.x * nd.x + be2.y * nd.y + be2.z * nd.z;
    d.qv = e1b.x * nd.x + e1b.y * nd.y + e1b.z * nd.z;
    return d;
}

// The accept test, hit point and distance as the reference computes them (:237-242), from the row alone.
__device__ __forceinline__ bool exact_hit_row(const TestDots &d, float e1e2b, const RowVecs &r, v3 start, v3 *pos, float *dist)
{
    const float t = e1e2b / d.den, u = d.pu / d.den, v = d.qv / d.den;
    if (u + v <= 1.0f && u >= 0.0f && v >= 0.0f && t >= 0.0f) {
        const v3 p = add3(add3(r.v0, scale3(r.e1, u)), scale3(r.e2, v));
        *pos = p;
        *dist = distance3(start, p);
        return true;
    }
    return false;
}

// ---- the counters of a STATS kernel ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// The QSTAT_WORDS counters of a STATS kernel: summed over the wave, one atomic per wave and non-zero word.
__device__ __forceinline__ void flush_query_stats(unsigned long long *stats, unsigned long long rays, unsigned long long cand,
                                                  unsigned long long tests, unsigned long long fallback)
{
    const unsigned long long sums[QSTAT_WORDS] = { wave_sum64(rays), wave_sum64(cand), wave_sum64(tests), wave_sum64(fallback) };
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int w = 0; w < QSTAT_WORDS; w++)
            if (sums[w]) atomicAdd(stats + w, sums[w]);
}

}  // namespace mirt
