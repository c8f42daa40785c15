// fan_order.hpp -- what the bound of a K-entry list (hit_list.hpp) admits of a cube bin's list (../query/rt_query.hpp: CubeView), once:
// the lines k_fan_order / k_fans_order (ordered_fans.hip) decide by, and tests/cpp/fan_order_test.cpp checks against a plain sort.
// Plain C++ under any compiler; MIRT_HD under hipcc.
//
// The structure gives, per accepted (row, direction) pair of distance d: near <= d in float -- a cube row's `near` is a lower bound of
// the distance the reference computes for ANY direction from the origin, pos = v0 + u e1 + v e2 lies on the triangle -- and the row's
// shell is the shell of its `near`, by the one formula bin_shell_of, which is monotone: near <= b implies shell(near) <= shell(b).
// So for a list that holds K entries at or below the bound b, a row with near > b, or in a shell behind that of b, has d > b and
// could not enter.  Both rejects are strict: a row AT the bound is a tie the index decides, and is still tested.
//
// The bound is FLT_MAX until K entries are held (along_order_bound's reasoning: no eligible distance is above FLT_MAX, and the shell
// of a finite float is a defined conversion on host and device alike).  A cube whose shells have no width (shell_iw == 0: a position
// whose depth range is degenerate, pass_plan.hpp) gives (FLT_MAX - d0) * 0 = 0, shell 0 -- and every row of such a cube lies in
// shell 0 by the same product, so the list that ends behind shell 0 is the whole list.  With a width, (FLT_MAX - d0) * iw is far
// beyond the last shell, or +inf, and the clamp gives the last shell: the whole list as well.  The +inf of a list that is not full
// would give inf * 0 = NaN in the first case -- shell 0 too, but only by the NaN rule; FLT_MAX needs no such rule.
//
// The list's end is light_off[key + shell(b) + 1] and only moves in: b never grows.  No shell is skipped for lying in FRONT of an
// `after` record: a row has no upper depth bound (`far` belongs to the shadow rays' rows), so a row whose `near` is small may be hit
// at any distance behind it, and a ray that continues walks its first shells again.  A row offered twice gives an equal key, which the list drops (hit_list_offer): nothing depends on
// a bin's list naming a triangle only once.
#pragma once

#include "hit_list.hpp"

namespace mirt {

// The bound a walk uses: the list's, with FLT_MAX in place of the +inf of a list that is not full.
MIRT_HD float fan_order_bound(float list_bound) { return list_bound <= FLT_MAX ? list_bound : FLT_MAX; }

// Whether a row is still tested: the reject is strict, and a NaN on either side rejects nothing.
MIRT_HD bool fan_order_near_ok(float near, float bound) { return !(near > bound); }

// The number of shells of its bin the ray still walks, given the shell `shell_of_bound` the bound falls into: a row in a later
// shell has near > bound.
MIRT_HD uint32_t fan_order_shells(uint32_t shell_of_bound) { return shell_of_bound + 1u; }

}  // namespace mirt
