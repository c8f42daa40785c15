// along_order.hpp -- what the bound of a K-entry list (hit_list.hpp) admits of an along grid's cell (../along/along.hpp), once: the
// three lines k_along_order / k_alongs_order (ordered_along.hip) decide by, and tests/cpp/along_order_test.cpp checks against a
// plain sort.  Plain C++ under any compiler; MIRT_HD under hipcc.
//
// The structure gives, per accepted (row, start) pair of distance d: near <= rs + d in float, and the row's shell is no later than
// the shell of rs + d (tests/cpp/along_bins_test.cpp).  Float addition of a fixed rs is monotone: d <= b implies rs + d <= rs + b.
// So for a list that holds K entries at or below the bound b, a row with near > rs + b, or in a shell behind that of rs + b, has
// d > b and could not enter.  Both rejects are strict: a row AT the bound is a tie the index decides, and is still tested.
#pragma once

#include "hit_list.hpp"

namespace mirt {

// The bound a walk uses: the list's, with FLT_MAX in place of the +inf of a list that is not full.  No eligible distance is above
// FLT_MAX (hit_eligible), so nothing is lost; and the shell of the threshold stays a conversion of a finite float or of a float the
// shell's clamp covers on host and device alike -- (int)(+inf) is not defined in C++, and +inf times a zero shell width is NaN.
MIRT_HD float along_order_bound(float list_bound) { return list_bound <= FLT_MAX ? list_bound : FLT_MAX; }

// The threshold of a ray whose depth is rs: what a row's depth bound `near` is compared with and what the cell list's end follows.
MIRT_HD float along_order_threshold(float rs, float bound) { return rs + bound; }

// Whether a row is still tested: the reject is strict, and a NaN on either side rejects nothing.
MIRT_HD bool along_order_near_ok(float near, float thr) { return !(near > thr); }

// The number of shells of its cell the ray still walks, given the shell `shell_of_thr` the threshold falls into.
MIRT_HD uint32_t along_order_shells(uint32_t shell_of_thr) { return shell_of_thr + 1u; }

}  // namespace mirt
