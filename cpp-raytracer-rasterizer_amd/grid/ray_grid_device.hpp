// ray_grid_device.hpp -- device helpers of the arbitrary-ray grid's walk kernels (ray_grid.hip) that kernels outside that file use as
// well (../order/ordered_hits.hip): a lane's ray and whether it fits the walk, the step to a lane's next run of rows, and the flush of
// a STATS kernel's counters.  Their text is the one ray_grid.hip has always compiled.
#pragma once

#include "ray_grid.hpp"
#include "../query/rt_query_device.hpp"

namespace mirt {

// A lane's ray.  `fit`: grid_ray_fit and inside the filter's range (ray_exact_only false: the scene's rows and a start below 1e8; the
// window keeps negD inside it) -- the thresholds of grid_tri_setup hold for exactly these.  Any other live lane sweeps all n rows
// of the scene in index order after the wave's walk, with k_query_closest's loop body.
struct GridLane {
    v3 S, nd;
    bool exact_only, fit;
};
__device__ __forceinline__ GridLane grid_lane(const GridFrame &f, long long ray, bool ok)
{
    const float *r = f.q.rays + (size_t)RAY_WORDS * (ok ? ray : 0);
    const v3 S = ld3(r), dir = ld3(r + 3);
    GridLane l;
    l.S = S;
    l.nd = V3(-dir.x, -dir.y, -dir.z);
    l.exact_only = ray_exact_only(scene_rows_in_range(f.q), S, dir);
    l.fit = grid_ray_fit(f.v.d, S, dir) && !l.exact_only;
    return l;
}

// One step of the walk for a lane whose run of rows is used up: its next run [e, end) -- which may be empty --, or the state moved on,
// or the lane through (live = false); `src` says which part of the structure a run comes from.  Straight-line per lane: the lanes of a
// wave that need a step take it together, whatever part of the walk each is in.
__device__ __forceinline__ void grid_step_rows(const GridView &v, GridWalk &w, double reach, bool &live, uint32_t &e, uint32_t &end, int &src)
{
    if (live && !(e < end)) {
        uint32_t kf = 0u, kl = 0u;
        const int r = grid_walk_step(v.d, w, reach, &kf, &kl);
        if (r == GRID_STEP_DONE) live = false;
        if (r == GRID_STEP_RUN) {
            e = v.off[kf];
            end = v.off[kl + 1u];
            src = kf >= v.d.key_every ? 2 : (kf >= v.d.key_plane ? 1 : 0);
        }
    }
}

__device__ __forceinline__ void flush_grid_stats(unsigned long long *stats, const unsigned long long (&c)[GSTAT_WORDS])
{
#pragma unroll
    for (int w = 0; w < GSTAT_WORDS; w++) {
        const unsigned long long s = wave_sum64(c[w]);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(stats + w, s);
    }
}

}  // namespace mirt
