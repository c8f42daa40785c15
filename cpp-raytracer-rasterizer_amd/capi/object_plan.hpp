// object_plan.hpp -- the decisions of the posed-scene calls (mirt_scene_set_objects, mirt_scene_pose, mirt_pose) that are pure
// arithmetic, free of library state: whether an object list is one (ranges inside their arrays, scene ranges pairwise disjoint),
// whether a list of objects to pose is one (indices inside the list, none twice), and the work items of a pose -- one per listed
// object and 256-row chunk of it -- with the lookup a workgroup of the pose kernel makes to find its own.  Host code without HIP
// types (the lookup alone is also compiled for the device, by scene/scene_kernels.hip); scene.cpp applies it to the uploaded scene,
// csrc/scene_host.cpp to the caller's arrays; tests/cpp/object_plan_test.cpp checks it on the CPU.
#pragma once

#include "../../include/mirt.h"

#include <stdint.h>

#include <algorithm>
#include <vector>

#ifdef __HIPCC__
#define MIRT_PLAN_HD __host__ __device__ inline
#else
#define MIRT_PLAN_HD inline
#endif

namespace mirt {

constexpr int POSE_CHUNK_ROWS = 256;             // rows of a work item: one workgroup's (scene_kernels.hpp: SCENE_BLOCK_ROWS)

// ---- an object list ----
// What is wrong with it, in the order the checks are made: every field of every object first, then the ranges, then the overlaps.
// a: the object; b: the other one of an overlapping pair.
enum ObjectFault { OBJECTS_OK = 0, OBJECT_NEGATIVE, OBJECT_LEAVES_REST, OBJECT_LEAVES_SCENE, OBJECTS_OVERLAP };
struct ObjectCheck { ObjectFault fault; int a, b; };

// Object k writes rest rows [rest_first, rest_first + count) of nrest to scene rows [scene_first, scene_first + count) of n.  An
// empty object is never work and overlaps nothing, wherever it starts within [0, n]; rest ranges may overlap as they like.  The
// sums are taken in long long: first + count of two ints passes INT_MAX.
inline ObjectCheck check_objects(const mirt_object *o, int nobjects, int nrest, int n)
{
    for (int k = 0; k < nobjects; k++)
        if (o[k].rest_first < 0 || o[k].scene_first < 0 || o[k].count < 0) return ObjectCheck{ OBJECT_NEGATIVE, k, k };
    for (int k = 0; k < nobjects; k++) {
        if ((long long)o[k].rest_first + o[k].count > nrest) return ObjectCheck{ OBJECT_LEAVES_REST, k, k };
        if ((long long)o[k].scene_first + o[k].count > n) return ObjectCheck{ OBJECT_LEAVES_SCENE, k, k };
    }
    // the objects that write anything, by where they start: two of them overlap exactly when two neighbours of this order do
    std::vector<int> order;
    for (int k = 0; k < nobjects; k++)
        if (o[k].count > 0) order.push_back(k);
    std::sort(order.begin(), order.end(), [o](int x, int y) { return o[x].scene_first != o[y].scene_first ? o[x].scene_first < o[y].scene_first : x < y; });
    for (size_t i = 1; i < order.size(); i++) {
        const mirt_object &p = o[order[i - 1]], &q = o[order[i]];
        if ((long long)p.scene_first + p.count > q.scene_first) return ObjectCheck{ OBJECTS_OVERLAP, std::min(order[i - 1], order[i]), std::max(order[i - 1], order[i]) };
    }
    return ObjectCheck{ OBJECTS_OK, -1, -1 };
}

// ---- the objects of one pose ----
// which[i]: an index into the declared list; NULL: objects 0 .. count - 1.  at: the entry of `which` that is wrong.
enum WhichFault { WHICH_OK = 0, WHICH_NO_OBJECTS, WHICH_TOO_MANY, WHICH_OUTSIDE, WHICH_TWICE };
struct WhichCheck { WhichFault fault; int at; };
inline WhichCheck check_which(const int32_t *which, int count, int nobjects)
{
    if (nobjects <= 0) return WhichCheck{ WHICH_NO_OBJECTS, -1 };
    if (!which) return WhichCheck{ count > nobjects ? WHICH_TOO_MANY : WHICH_OK, -1 };
    for (int i = 0; i < count; i++)
        if (which[i] < 0 || which[i] >= nobjects) return WhichCheck{ WHICH_OUTSIDE, i };
    std::vector<bool> seen((size_t)nobjects, false);
    for (int i = 0; i < count; i++) {
        if (seen[(size_t)which[i]]) return WhichCheck{ WHICH_TWICE, i };
        seen[(size_t)which[i]] = true;
    }
    return WhichCheck{ WHICH_OK, -1 };
}
inline int listed_object(const int32_t *which, int i) { return which ? which[i] : i; }

// ---- the work items of a pose ----
// What the pose kernel reads of listed object i (64 bytes: one scalar load) ...
struct PoseEntry {
    int32_t rest_first, scene_first, count;
    float rot[9], tr[3];                         // v -> rot * v + tr (rot: column-major)
    int32_t pad;
};
static_assert(sizeof(PoseEntry) == 64, "one 16-dword row per listed object");
constexpr int POSE_ENTRY_WORDS = sizeof(PoseEntry) / 4;
// ... and the table of a call, in 32-bit words: `count` entries, then count + 1 words of prefix -- prefix[i] = work items of the
// listed objects before i, prefix[count] = all of them, the launch's grid.
inline size_t pose_table_words(int count) { return (size_t)count * POSE_ENTRY_WORDS + (size_t)count + 1; }
MIRT_PLAN_HD const uint32_t *pose_prefix_of(const PoseEntry *table, int count) { return reinterpret_cast<const uint32_t *>(table + count); }
inline uint32_t pose_chunks_of(int rows) { return (uint32_t)(((long long)rows + POSE_CHUNK_ROWS - 1) / POSE_CHUNK_ROWS); }

// Fills the table for `count` listed objects (xforms12: {rot9, translate3} each) and returns the number of work items.  Disjoint scene
// ranges bound it by n / 256 + n, which 32 bits hold.
inline uint32_t fill_pose_table(const mirt_object *objects, const int32_t *which, int count, const float *xforms12, uint32_t *words)
{
    PoseEntry *e = reinterpret_cast<PoseEntry *>(words);
    uint32_t *prefix = words + (size_t)count * POSE_ENTRY_WORDS, total = 0;
    for (int i = 0; i < count; i++) {
        const mirt_object &o = objects[listed_object(which, i)];
        e[i].rest_first = o.rest_first; e[i].scene_first = o.scene_first; e[i].count = o.count;
        for (int k = 0; k < 9; k++) e[i].rot[k] = xforms12[12 * (size_t)i + k];
        for (int k = 0; k < 3; k++) e[i].tr[k] = xforms12[12 * (size_t)i + 9 + k];
        e[i].pad = 0;
        prefix[i] = total;
        total += pose_chunks_of(o.count);
    }
    prefix[count] = total;
    return total;
}

// The listed object work item `item` (< prefix[count]) belongs to: the LAST i with prefix[i] <= item -- an object without rows adds
// nothing to the prefix, so its entry equals its successor's, and the last of a run of equal entries is the one that has the item.
// The item is chunk item - prefix[i] of that object: rows [256 chunk, min(256 chunk + 256, count)).
MIRT_PLAN_HD int pose_find(const uint32_t *prefix, int count, uint32_t item)
{
    int lo = 0, hi = count;                      // prefix[lo] <= item < prefix[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (prefix[mid] <= item) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace mirt
