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

}  // namespace mirt
