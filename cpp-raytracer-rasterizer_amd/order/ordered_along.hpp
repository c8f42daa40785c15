// ordered_along.hpp -- the parameter blocks and the kernels of mirt_intersect_ordered_along* / mirt_intersect_ordered_alongs*
// (ordered_along.hip; the rule: order_bound.hpp; the host: ../capi/order_along.cpp): the walks of ../along/along_walk.hpp with the
// list of hit_list.hpp in place of the record.
#pragma once

#include "ordered_hits.hpp"
#include "../along/alongs.hpp"

namespace mirt {

// A call along a direction with what the ordered call adds (order_out.hpp).  a.q.hits, a.limit and a.occluded are not read.
struct AlongOrderFrame {
    AlongFrame a;
    OrderOut out;
};
// One pass of a call along several directions (alongs.hpp: AlongsFrame).  The pass with a.first == 0 writes the count 0 for a ray
// whose index lies outside [0, ndirs); no pass writes that ray's slots.
struct AlongsOrderFrame {
    AlongsFrame a;
    OrderOut out;
};

template <int K, bool STATS> __attribute__((global)) void k_along_order(const AlongOrderFrame);
template <int K, bool STATS> __attribute__((global)) void k_alongs_order(const AlongsOrderFrame);

}  // namespace mirt
