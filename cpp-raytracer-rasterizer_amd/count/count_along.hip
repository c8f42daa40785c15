// count_along.hip -- hand-written gfx950 kernels of mirt_count_hits_along* and mirt_count_hits_alongs*: the hit counts of the rays
// {origins[i], dir} or {origins[i], dirs[dir_of[i]]} through the grid across the direction that mirt_intersect_along* /
// mirt_occluded_along* and mirt_intersect_alongs* / mirt_occluded_alongs* walk (../along/along.hpp; the same tables: a grid one family
// builds serves the other).  The walk and the argument that it offers a row at most once: count_walk.hpp.  The kernels take their
// descriptors as along.hip's and alongs.hip's take them (../along/along_lanes.hpp).
// Built with -ffp-contract=off like every kernel of the library.
#include "count_walk.hpp"

namespace mirt {

// ---- k_along_count: one direction, its descriptor in the kernel's arguments (k_along_occluded's shape) ------------------------------
template <bool STATS>
__global__ __launch_bounds__(256) void k_along_count(const AlongCountFrame f)
{
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = ray < f.a.q.nrays;
    const AlongTables t = { f.a.v.off, f.a.v.rows, f.a.v.aux };
    along_count_walk<STATS>(f.a.q, t, along_lane(f.a, ray, ok), ray, ok, false, f.out, f.a.stats);
}

template __global__ void k_along_count<false>(const AlongCountFrame);
template __global__ void k_along_count<true>(const AlongCountFrame);

// ---- k_alongs_count: a group of directions, each lane's descriptor out of LDS by its ray's index (k_alongs_occluded's shape) -------
template <bool STATS>
__global__ __launch_bounds__(256) void k_alongs_count(const AlongsCountFrame f)
{
    __shared__ __attribute__((aligned(8))) uint32_t s_desc[MIRT_MAX_LIGHTS * ALONGS_DESC_WORDS];
    __shared__ float s_dir[MIRT_MAX_LIGHTS * 3];
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const AlongsLane a = alongs_lane(f.a, s_desc, s_dir, ray, ray < f.a.q.nrays);
    const AlongTables t = { f.a.off, f.a.rows, f.a.aux };
    along_count_walk<STATS>(f.a.q, t, a.l, ray, a.mine, a.zero, f.out, f.a.stats);
}

template __global__ void k_alongs_count<false>(const AlongsCountFrame);
template __global__ void k_alongs_count<true>(const AlongsCountFrame);

}  // namespace mirt
