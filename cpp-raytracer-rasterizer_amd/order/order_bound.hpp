// order_bound.hpp -- what the bound of a K-entry list (hit_list.hpp) admits of a depth-ordered row list, once: the lines the walks of
// ordered_along.hip (an along grid's cell, ../along/along.hpp) and ordered_fans.hip (a cube bin's list, ../query/rt_query.hpp:
// CubeView) decide by, and tests/cpp/along_order_test.cpp and tests/cpp/fan_order_test.cpp check against a plain sort.  Plain C++
// under any compiler; MIRT_HD under hipcc.
//
// The rule is one -- a row whose depth bound `near` lies strictly above a threshold, or whose shell lies behind the threshold's, is not
// tested --; why nothing is lost is argued per structure, and only the threshold differs: rs + bound along a direction, the bound
// itself from an origin.  Both rejects are strict: a row AT the bound is a tie the index decides, and is still tested.
//
// The along grid.  The structure gives, per accepted (row, start) pair of distance d: near <= rs + d in float, and the row's shell is
// no later than the shell of rs + d (tests/cpp/along_bins_test.cpp).  Float addition of a fixed rs is monotone: d <= b implies
// rs + d <= rs + b.  So for a list that holds K entries at or below the bound b, a row with near > rs + b, or in a shell behind that of
// rs + b, has d > b and could not enter.
//
// The cube bin.  The structure gives, per accepted (row, direction) pair of distance d: near <= d in float -- a cube row's `near` is a
// lower bound of the distance the reference computes for ANY direction from the origin, pos = v0 + u e1 + v e2 lies on the triangle --
// and the row's shell is the shell of its `near`, by the one formula bin_shell_of, which is monotone: near <= b implies shell(near) <=
// shell(b).  So for a list that holds K entries at or below the bound b, a row with near > b, or in a shell behind that of b, has
// d > b and could not enter.  The list's end is light_off[key + shell(b) + 1] and only moves in: b never grows.  No shell is skipped
// for lying in FRONT of an `after` record: a row has no upper depth bound (`far` belongs to the shadow rays' rows), so a row whose
// `near` is small may be hit at any distance behind it, and a ray that continues walks its first shells again.  A row offered twice
// gives an equal key, which the list drops (hit_list_offer): nothing depends on a bin's list naming a triangle only once.
//
// FLT_MAX for a list that is not full.  No eligible distance is above FLT_MAX (hit_eligible), so nothing is lost; and the shell of the
// threshold stays a conversion of a finite float or of a float the shell's clamp covers on host and device alike -- (int)(+inf) is not
// defined in C++, and +inf times a zero shell width is NaN.  A cube whose shells have no width (shell_iw == 0: a position whose depth
// range is degenerate, pass_plan.hpp) gives (FLT_MAX - d0) * 0 = 0, shell 0 -- and every row of such a cube lies in shell 0 by the same
// product, so the list that ends behind shell 0 is the whole list.  With a width, (FLT_MAX - d0) * iw is far beyond the last shell, or
// +inf, and the clamp gives the last shell: the whole list as well.  The +inf of a list that is not full would give inf * 0 = NaN in
// the first case -- shell 0 too, but only by the NaN rule; FLT_MAX needs no such rule.
#pragma once

#include "hit_list.hpp"

namespace mirt {

// The bound a walk uses: the list's, with FLT_MAX in place of the +inf of a list that is not full.
MIRT_HD float order_bound(float list_bound) { return list_bound <= FLT_MAX ? list_bound : FLT_MAX; }

// The threshold of a ray along a direction whose depth is rs: what a row's `near` is compared with and what the cell list's end
// follows.  (From an origin the threshold is the bound.)
MIRT_HD float along_order_threshold(float rs, float bound) { return rs + bound; }

// Whether a row is still tested: the reject is strict, and a NaN on either side rejects nothing.
MIRT_HD bool order_near_ok(float near, float thr) { return !(near > thr); }

// The number of shells of its list the ray still walks, given the shell `shell_of_thr` the threshold falls into.
MIRT_HD uint32_t order_shells(uint32_t shell_of_thr) { return shell_of_thr + 1u; }

}  // namespace mirt
