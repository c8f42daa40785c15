// ordered_fans.hpp -- the parameter blocks and the kernels of mirt_intersect_ordered_from* / mirt_intersect_ordered_fans*
// (ordered_fans.hip; the rule: fan_order.hpp; the host: ../capi/order_fans.cpp): the fan walk of ../query/rt_query.hip with the list of
// hit_list.hpp in place of the record.
#pragma once

#include "hit_list.hpp"
#include "../query/rt_query.hpp"

namespace mirt {

// What the ordered walk adds to a fan from one origin: f.hits is the OUTPUT (nrays * max_hits records, ray-major), the `after` records
// or NULL, and the counts.
struct FanOrderFrame {
    QueryFanFrame f;
    const uint32_t *after;       // nrays records of HIT_WORDS words, or NULL: only distance and index are read
    int max_hits;                // 1 .. K of the instantiation
    int32_t *counts;             // nrays
};
// One pass of a call from several origins (rt_query.hpp: QueryFansFrame).  norigins is the CALL's origin count: the pass with
// f.first == 0 writes the count 0 for a ray whose index lies outside [0, norigins); no pass writes that ray's slots.
struct FansOrderFrame {
    QueryFansFrame f;
    int norigins;
    const uint32_t *after;
    int max_hits;
    int32_t *counts;
};

template <int K, bool STATS> __attribute__((global)) void k_fan_order(const FanOrderFrame);
template <int K, bool STATS> __attribute__((global)) void k_fans_order(const FansOrderFrame);

}  // namespace mirt
