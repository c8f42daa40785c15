// along_plan.hpp -- the arithmetic of the ray queries along SEVERAL directions in one call (mirt_intersect_alongs*,
// mirt_occluded_alongs*; alongs.cpp, ../along/alongs.hip) that is free of library state and of device code: how many directions
// share one build chain, the ranges of the call's list its passes cover, and how a sort key is put together from a direction's
// place in its group and the key the single-direction grid gives (../along/along.hpp).  tests/cpp/alongs_plan_test.cpp checks it on
// the CPU.
#pragma once

#include "../along/along.hpp"
#include "cube_plan.hpp"

#include <algorithm>
#include <vector>

namespace mirt {

// ---- the group ----
// A group's directions take consecutive SLOTS.  Slot s owns the keys [s * K, (s + 1) * K), K = along_keys(B, shells): inside them
// the layout is the single grid's, (cell * shells + shell) with cell B * B the every-ray list, so one sort over one pair list
// orders every slot's lists and one offset table of slots * K + 1 entries bounds them.
//
// Slots per group: what one sort pass holds (BIN_MAX_KEYS, less the 64 keys every user of the sort leaves free), and never more
// than MIRT_MAX_LIGHTS -- the walk kernels stage that many descriptors.  32 up to B = 128, 15 at B = 256; 0 when not even one
// direction's keys fit.
inline int alongs_slots(int B, int shells)
{
    const uint32_t k = along_keys(B, shells);
    return (int)std::min<uint32_t>((uint32_t)MIRT_MAX_LIGHTS, (BIN_MAX_KEYS - 64u) / k);
}

// ---- the key ----
inline uint32_t alongs_key(uint32_t slot, uint32_t local, uint32_t keys_per_slot) { return slot * keys_per_slot + local; }
inline uint32_t alongs_key_slot(uint32_t key, uint32_t keys_per_slot) { return key / keys_per_slot; }
inline uint32_t alongs_key_local(uint32_t key, uint32_t keys_per_slot) { return key % keys_per_slot; }
// Keys of a group of `slots` directions (the offset table holds one entry more).
inline uint32_t alongs_group_keys(int slots, int B, int shells) { return (uint32_t)slots * along_keys(B, shells); }

// ---- the passes ----
// A call of more directions than a group holds runs in passes over consecutive ranges of its list: pass p covers the directions
// [first, first + count).  Every pass covers all rays; a ray whose direction lies outside the range leaves at once.
struct AlongsPass { int first, count; };
// The passes of a call of ndirs directions with `slots` slots a group; false when nothing can be planned (no slot, no direction).
inline bool alongs_pass_plan(int ndirs, int slots, std::vector<AlongsPass> *plan)
{
    plan->clear();
    if (ndirs <= 0 || slots <= 0) return false;
    for (int first = 0; first < ndirs; first += slots) plan->push_back(AlongsPass{ first, std::min(slots, ndirs - first) });
    return true;
}
// The kept group pass p reads and leaves: one of ALONGS_GROUPS, taken in turn, so that a repeated call of up to that many passes
// finds every group held.
constexpr int ALONGS_GROUPS = 8;
inline int alongs_group_of_pass(size_t pass) { return (int)(pass % (size_t)ALONGS_GROUPS); }

// What the passes of a call read, folded for mirt_query_stats::cube_source: 0 none yet, 1 some pass built, 2 every pass's group was held.
inline int alongs_fold_source(int so_far, bool built) { return built || so_far == 1 ? 1 : 2; }

}  // namespace mirt
