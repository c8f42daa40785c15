// count_rule.hpp -- which hits of a ray a count holds (mirt_count_hits*): the ONE admission predicate, for the kernels (count_hits.hip,
// count_walk.hpp), the host (../capi/count.cpp) and tests/cpp/count_rule_test.cpp, and what a limit admits of a depth-ordered row
// list.  Plain C++ under any compiler; MIRT_HD under hipcc.
//
// The count of a ray is the number of triangles j ClosestIntersection's test accepts (raytracer.cpp:239) whose distance d_j (:241-242)
//   - a fresh record would take, FLT_MAX >= d_j (hit_eligible: never NaN or +inf),
//   - comes behind the `after` record (a, k) when there is one, d_j > a || (d_j == a && j < k) (hit_after, float and signed-int
//     comparisons as written: a NaN a admits nothing, -0.0f is 0.0f),
//   - lies below the limit L, d_j < L, strictly (the occlusion calls' `<`, :313; a NaN, 0 or negative L admits nothing).
// No limit is L = +inf: every eligible distance is finite, hence below it.
//
// A count has no list and no order, and -- unlike the closest hit, the any-hit byte and the K first hits -- it is NOT indifferent to a
// row that is offered twice: whatever offers rows to this predicate must offer each row of the scene at most once per ray (DESIGN.md
// section 5.1, "Counting hits", says which structures do).
#pragma once

#include "../order/order_bound.hpp"

namespace mirt {

// Whether triangle j at distance d counts for a ray that continues behind (a, k) (has_after) below the limit L.
MIRT_HD bool count_admits(float d, int j, bool has_after, float a, int k, float L)
{
    return hit_eligible(d) && (!has_after || hit_after(d, j, a, k)) && d < L;
}

// Whether a ray can count anything at all: a limit nothing is below (NaN, 0, negative) or a NaN `after` distance settles it before
// any row is read.
MIRT_HD bool count_open(bool has_after, float a, float L) { return L > 0.0f && (!has_after || a == a); }

// The depth threshold of a ray along a direction whose depth is rs (../along/along.hpp: Depth): along_occluded_walk's rs + L with
// FLT_MAX in place of a limit above it -- order_bound.hpp's treatment of a list that is not yet full, and for its reason: no
// admitted distance is above FLT_MAX, and the shell of the threshold stays the conversion of a finite float.  An admitted row has
// d < L and d <= FLT_MAX, so near <= rs + d <= rs + min(L, FLT_MAX) in float (the addition of a fixed rs is monotone): it passes the
// strict reject order_near_ok and lies in a shell no later than the threshold's.  `after` moves nothing: a row has no upper depth bound.
MIRT_HD float count_threshold(float rs, float L) { return along_order_threshold(rs, order_bound(L)); }

}  // namespace mirt
