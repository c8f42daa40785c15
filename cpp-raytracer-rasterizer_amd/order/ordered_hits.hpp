// ordered_hits.hpp -- the parameter block and the kernels of mirt_intersect_ordered* (ordered_hits.hip; the list rule: hit_list.hpp;
// the host: ../capi/order.cpp).
#pragma once

#include "hit_list.hpp"
#include "order_out.hpp"
#include "../grid/ray_grid.hpp"

namespace mirt {

// A call: the scene's rows and the caller's rays (f.q; f.q.hits is not read), the grid's structure and counters for k_grid_order
// (f.v, f.stats; unused by the sweeps), and what the ordered call adds (out).
struct OrderFrame {
    GridFrame f;
    OrderOut out;
    const int32_t *dir_of;       // the sweeps of mirt_intersect_ordered_alongs*: the rays' indices into the call's ndirs directions; a ray
    int ndirs;                   // whose index names none keeps its slots and gets the count 0.  NULL: every ray is answered
};

template <int K> __attribute__((global)) void k_order_sweep(const OrderFrame);
template <int K> __attribute__((global)) void k_order_sweep_wave(const OrderFrame);
template <int K, bool STATS> __attribute__((global)) void k_grid_order(const OrderFrame);

}  // namespace mirt
