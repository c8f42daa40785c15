// ordered_fans.hpp -- the parameter blocks and the kernels of mirt_intersect_ordered_from* / mirt_intersect_ordered_fans*
// (ordered_fans.hip; the rule: order_bound.hpp; the host: ../capi/order_fans.cpp): the fan walk of ../query/rt_query.hip with the list of
// hit_list.hpp in place of the record.
#pragma once

#include "hit_list.hpp"
#include "order_out.hpp"
#include "../query/rt_query.hpp"

namespace mirt {

// A fan from one origin with what the ordered call adds (order_out.hpp).  f.hits is not read.
struct FanOrderFrame {
    QueryFanFrame f;
    OrderOut out;
};
// One pass of a call from several origins (rt_query.hpp: QueryFansFrame).  norigins is the CALL's origin count: the pass with
// f.first == 0 writes the count 0 for a ray whose index lies outside [0, norigins); no pass writes that ray's slots.
struct FansOrderFrame {
    QueryFansFrame f;
    int norigins;
    OrderOut out;
};

template <int K, bool STATS> __attribute__((global)) void k_fan_order(const FanOrderFrame);
template <int K, bool STATS> __attribute__((global)) void k_fans_order(const FansOrderFrame);

}  // namespace mirt
