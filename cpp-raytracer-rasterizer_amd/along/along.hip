// along.hip -- hand-written gfx950 kernels of the ray queries along one direction (mirt_intersect_along*, mirt_occluded_along*;
// along.hpp has the structure and the predicate, DESIGN.md section 5.1 the argument).
//
// The build (once per scene version and direction): k_along_pairs files every triangle -- a (cell, shell) key per cell its region
// may reach, or the one key of the every-ray list --, bucket_sort_pairs (../csrc/bin_sort.hpp) orders the pairs, k_along_rows
// writes the 48-byte QueryRow of each pair in key order with the triangle's index and depth bound alongside.
// The walks: one lane per ray over its cell's list, front to back in depth shells, then the every-ray list -- the bodies of
// along_walk.hpp, which the kernels of several directions in one call (alongs.hip) run too.
// Built with -ffp-contract=off like every kernel of the library.
#include "along_file.hpp"
#include "along_lanes.hpp"

namespace mirt {

// ---- the build ---------------------------------------------------------------------------------------------------------------------

// One lane per triangle: along_file.hpp's filing body with the call's descriptor, keys from 0 and the triangle's index as the value.
__global__ __launch_bounds__(256) void k_along_pairs(const AlongPairs b)
{
    extern __shared__ uint32_t s_hist[];
    const AlongFiling o = { b.counters, b.counters + 1, b.keys, b.vals, b.cap, b.bucket_cnt, b.nbuckets, b.bucket_shift };
    along_file_triangles(b.d, o, s_hist, b.qrows, b.n, 0u, 0u, b.near);
}

// Row e of the structure: the scene's row of the e-th triangle in key order, its index and depth bound beside it.
__global__ __launch_bounds__(256) void k_along_rows(const AlongRows x)
{
    const uint32_t total = *x.total;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const uint32_t tri = x.entries[e];
        const float4 *src = reinterpret_cast<const float4 *>(x.qrows + tri);
        float4 *dst = reinterpret_cast<float4 *>(x.rows + e);
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
        AlongAux a;
        a.tri = tri; a.near = x.near[tri];
        x.aux[e] = a;
    }
}

// The rays of a call written out for k_query_closest* / k_query_occluded* (BRUTE, and every call the structure is not built for).
__global__ __launch_bounds__(256) void k_along_expand(const AlongExpand x)
{
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    if (ray >= x.nrays) return;
    float *r = x.rays + (size_t)RAY_WORDS * ray;
    st3(r, ld3(x.origins + 3 * (size_t)ray));
    st3(r + 3, V3(x.dir[0], x.dir[1], x.dir[2]));
}


// ---- the walks ---------------------------------------------------------------------------------------------------------------------
//
// One direction: the descriptor, the tables and dir are the kernel's arguments, the same for every lane; the direction's keys start
// at 0.  A lane beyond the call's rays reads ray 0's start and is not `mine` (along_walk.hpp); along_lane: along_lanes.hpp.
template <bool STATS>
__global__ __launch_bounds__(256) void k_along_closest(const AlongFrame f)
{
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = ray < f.q.nrays;
    const AlongTables t = { f.v.off, f.v.rows, f.v.aux };
    along_closest_walk<STATS>(f.q, t, along_lane(f, ray, ok), ray, ok, f.stats);
}

template __global__ void k_along_closest<false>(const AlongFrame);
template __global__ void k_along_closest<true>(const AlongFrame);

template <bool STATS>
__global__ __launch_bounds__(256) void k_along_occluded(const AlongFrame f)
{
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = ray < f.q.nrays;
    const AlongTables t = { f.v.off, f.v.rows, f.v.aux };
    along_occluded_walk<STATS>(f.q, t, along_lane(f, ray, ok), ray, ok, false, f.limit, f.occluded, f.stats);
}

template __global__ void k_along_occluded<false>(const AlongFrame);
template __global__ void k_along_occluded<true>(const AlongFrame);

}  // namespace mirt
