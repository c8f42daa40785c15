// ordered_along.hpp -- the parameter blocks and the kernels of mirt_intersect_ordered_along* / mirt_intersect_ordered_alongs*
// (ordered_along.hip; the rule: along_order.hpp; the host: ../capi/order_along.cpp): the walks of ../along/along_walk.hpp with the
// list of hit_list.hpp in place of the record.
#pragma once

#include "ordered_hits.hpp"
#include "../along/alongs.hpp"

namespace mirt {

// What the ordered walks add to a call along a direction: a.q.hits is the OUTPUT (nrays * max_hits records, ray-major), the `after`
// records or NULL, and the counts.  a.limit and a.occluded are not read.
struct AlongOrderFrame {
    AlongFrame a;
    const uint32_t *after;       // nrays records of HIT_WORDS words, or NULL: only distance and index are read
    int max_hits;                // 1 .. K of the instantiation
    int32_t *counts;             // nrays
};
// One pass of a call along several directions (alongs.hpp: AlongsFrame).  The pass with a.first == 0 writes the count 0 for a ray
// whose index lies outside [0, ndirs); no pass writes that ray's slots.
struct AlongsOrderFrame {
    AlongsFrame a;
    const uint32_t *after;
    int max_hits;
    int32_t *counts;
};

template <int K, bool STATS> __attribute__((global)) void k_along_order(const AlongOrderFrame);
template <int K, bool STATS> __attribute__((global)) void k_alongs_order(const AlongsOrderFrame);

}  // namespace mirt
