// alongs.hip -- hand-written gfx950 kernels of the ray queries along several directions in one call (mirt_intersect_alongs*,
// mirt_occluded_alongs*; alongs.hpp has the parameter blocks, along.hpp the structure and the predicate, DESIGN.md section 5.1 the
// argument).
//
// The build of a GROUP of directions (once per scene version and list of directions): k_alongs_pairs files every triangle for every
// slot -- k_along_pairs' body (along_file.hpp) with the slot's descriptor and the slot's first key --, bucket_sort_pairs (../csrc/bin_sort.hpp)
// orders the one pair list, k_alongs_rows writes the rows in key order.
// The walks: along_walk.hpp's two bodies, the ones k_along_closest / k_along_occluded run; a lane's descriptor, first key and
// direction are those of the slot its ray's index names, read out of LDS, where every workgroup stages the group's tables once.
// Built with -ffp-contract=off like every kernel of the library.
#include "alongs.hpp"
#include "along_file.hpp"
#include "along_lanes.hpp"

namespace mirt {

// ---- the build ---------------------------------------------------------------------------------------------------------------------

// One lane per (triangle, slot): along_file.hpp's filing body -- the one k_along_pairs runs, its counting scheme unchanged -- with the
// slot's descriptor, keys from the slot's first and slot * n + triangle as the value.  The slot is the grid's y, so the descriptor is
// the same for every lane of a workgroup: it is copied out of the device table before anything is stored, which leaves the loads
// scalar.  The triangles on the every-ray list are counted per slot (counters[1 + slot]): each slot's list has its own cap.
__global__ __launch_bounds__(256) void k_alongs_pairs(const AlongsPairs b)
{
    extern __shared__ uint32_t s_hist[];
    const uint32_t slot = blockIdx.y;
    const AlongDesc d = b.descs[slot];
    const AlongFiling o = { b.counters, b.counters + 1u + slot, b.keys, b.vals, b.cap, b.bucket_cnt, b.nbuckets, b.bucket_shift };
    along_file_triangles(d, o, s_hist, b.qrows, b.n, slot * b.keys_per_slot, slot * (uint32_t)b.n, b.near + (size_t)slot * (size_t)b.n);
}

// Row e of the group's tables: the scene's row of the e-th pair's triangle in key order, its index and the depth bound it has for
// the pair's slot beside it.
__global__ __launch_bounds__(256) void k_alongs_rows(const AlongsRows x)
{
    const uint32_t total = *x.total;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const uint32_t val = x.entries[e], tri = val % x.n;
        const float4 *src = reinterpret_cast<const float4 *>(x.qrows + tri);
        float4 *dst = reinterpret_cast<float4 *>(x.rows + e);
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
        AlongAux a;
        a.tri = tri; a.near = x.near[val];
        x.aux[e] = a;
    }
}

// The rays of a call written out for k_query_closest* / k_query_occluded* (BRUTE, and every call with a direction no structure is
// built for).  An index outside [0, ndirs) reads no direction and becomes the ray no triangle accepts, as in k_query_fans_expand:
// a NaN start makes every u, v and t of the accept test NaN, so its record stays unwritten and its byte is 0.
__global__ __launch_bounds__(256) void k_alongs_expand(const AlongsExpand x)
{
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    if (ray >= x.nrays) return;
    const uint32_t idx = x.dir_of ? (uint32_t)x.dir_of[ray] : 0u;
    const bool valid = idx < (uint32_t)x.ndirs;
    const float qnan = __uint_as_float(0x7fc00000u);
    const v3 S = valid ? ld3(x.origins + 3 * (size_t)ray) : V3(qnan, qnan, qnan);
    const v3 d = valid ? ld3(x.dirs + 3 * (size_t)idx) : V3(0.0f, 0.0f, 0.0f);
    float *r = x.rays + (size_t)RAY_WORDS * ray;
    st3(r, S);
    st3(r + 3, d);
}

// ---- the walks ---------------------------------------------------------------------------------------------------------------------
//
// A lane's descriptor, first key and direction: alongs_lane (along_lanes.hpp), staged through LDS once per workgroup.
template <bool STATS>
__global__ __launch_bounds__(256) void k_alongs_closest(const AlongsFrame f)
{
    __shared__ __attribute__((aligned(8))) uint32_t s_desc[MIRT_MAX_LIGHTS * ALONGS_DESC_WORDS];
    __shared__ float s_dir[MIRT_MAX_LIGHTS * 3];
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const AlongsLane a = alongs_lane(f, s_desc, s_dir, ray, ray < f.q.nrays);
    const AlongTables t = { f.off, f.rows, f.aux };
    along_closest_walk<STATS>(f.q, t, a.l, ray, a.mine, f.stats);
}

template __global__ void k_alongs_closest<false>(const AlongsFrame);
template __global__ void k_alongs_closest<true>(const AlongsFrame);

template <bool STATS>
__global__ __launch_bounds__(256) void k_alongs_occluded(const AlongsFrame f)
{
    __shared__ __attribute__((aligned(8))) uint32_t s_desc[MIRT_MAX_LIGHTS * ALONGS_DESC_WORDS];
    __shared__ float s_dir[MIRT_MAX_LIGHTS * 3];
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const AlongsLane a = alongs_lane(f, s_desc, s_dir, ray, ray < f.q.nrays);
    const AlongTables t = { f.off, f.rows, f.aux };
    along_occluded_walk<STATS>(f.q, t, a.l, ray, a.mine, a.zero, f.limit, f.occluded, f.stats);
}

template __global__ void k_alongs_occluded<false>(const AlongsFrame);
template __global__ void k_alongs_occluded<true>(const AlongsFrame);

}  // namespace mirt
