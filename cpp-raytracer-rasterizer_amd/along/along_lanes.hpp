// along_lanes.hpp -- where a lane of the walks along a direction takes its descriptor, first key and direction from (device code): the
// kernel's arguments for one direction (along.hip: k_along_closest / k_along_occluded), the slot its ray's index names out of LDS for
// a group of directions (alongs.hip: k_alongs_closest / k_alongs_occluded).  The ordered walks (../order/ordered_along.hip) take
// their lanes from here too.
#pragma once

#include "alongs.hpp"
#include "along_walk.hpp"

namespace mirt {

// One direction: the descriptor, the tables and dir are the kernel's arguments, the same for every lane; the direction's keys start
// at 0.  A lane beyond the call's rays reads ray 0's start and is not `mine` (along_walk.hpp).
__device__ __forceinline__ AlongLane along_lane(const AlongFrame &f, long long ray, bool ok)
{
    return along_walk_of(f.v.d, 0u, V3(f.dir[0], f.dir[1], f.dir[2]), scene_rows_in_range(f.q), ld3(f.origins + 3 * (size_t)(ok ? ray : 0)));
}

// The group's descriptors and directions staged once per workgroup: at most MIRT_MAX_LIGHTS of each, 3.9 KiB of LDS.  A lane then
// takes the slot its ray's index names -- lanes of a wave may hold different directions; their lists differ per lane anyway -- and
// copies what the walk reads of the slot's descriptor into its own registers (along_walk_of).  A lane that is not `mine` reads slot
// 0, which every pass has, so that every load stays inside the tables.
constexpr int ALONGS_DESC_WORDS = (int)(sizeof(AlongDesc) / sizeof(uint32_t));
static_assert(sizeof(AlongDesc) % sizeof(uint32_t) == 0 && alignof(AlongDesc) <= 8, "AlongDesc is staged word by word");

struct AlongsLane { AlongLane l; bool mine, zero; };
__device__ __forceinline__ AlongsLane alongs_lane(const AlongsFrame &f, uint32_t *s_desc, float *s_dir, long long ray, bool ok)
{
    const int count = min(f.count, MIRT_MAX_LIGHTS);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(f.descs);
    for (int w = threadIdx.x; w < count * ALONGS_DESC_WORDS; w += 256) s_desc[w] = src[w];
    for (int w = threadIdx.x; w < count * 3; w += 256) s_dir[w] = f.dirs[w];
    __syncthreads();
    const uint32_t idx = f.dir_of ? (uint32_t)f.dir_of[ok ? ray : 0] : 0u;
    const uint32_t rel = idx - (uint32_t)f.first;                  // (modulo 2^32: a negative or huge index lands beyond count)
    AlongsLane a;
    a.mine = ok && rel < (uint32_t)count;
    a.zero = ok && f.first == 0 && !(idx < (uint32_t)f.ndirs);
    const uint32_t slot = a.mine ? rel : 0u;
    const AlongDesc &d = reinterpret_cast<const AlongDesc *>(s_desc)[slot];
    const v3 dir = V3(s_dir[3 * slot], s_dir[3 * slot + 1], s_dir[3 * slot + 2]);
    a.l = along_walk_of(d, slot * f.keys_per_slot, dir, scene_rows_in_range(f.q), ld3(f.origins + 3 * (size_t)(ok ? ray : 0)));
    return a;
}

}  // namespace mirt
