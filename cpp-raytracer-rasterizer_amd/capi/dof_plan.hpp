// dof_plan.hpp -- the one decision of the depth-of-field path that is pure arithmetic, free of library state: how many rows above
// and below a band the blur of that band can tap, which is how many render_with_dof (capi.hpp) renders around it.  Host code
// without HIP types; tests/cpp/dof_plan_test.cpp checks it on the CPU against every tap.
#pragma once

#include <algorithm>
#include <cmath>

namespace mirt {

// CalculateDOF's tap range [zlo, zhi) in both directions (raytracer.cpp:624,626), as csrc/dof_kernel.hip derives it.
inline int dof_tap_lo(int K) { return (int)std::ceil((float)K / -2.0f); }
inline int dof_tap_hi(int K) { return (int)std::ceil((float)K / 2.0f); }

// floor(a / b) for b > 0 (the language's division rounds towards zero)
inline int dof_floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// The blur addresses its taps by FLAT index, (y + z) * W + (x + z2): a tap column outside the row lands floor((x + z2) / W) rows
// further on.  For the interior pixels, x in [1, W - 2], the farthest tap rows are therefore
//     above:  y + zlo + floor((1 + zlo) / W)            below:  y + zhi - 1 + floor((W - 3 + zhi) / W)
// On a frame at least about K / 2 wide a column wraps by one row at most, which is the `+ 1` of the halo every frame has always
// had; a narrower frame wraps further and needs more.  The halo is the larger of the two, so that every frame the old halo served
// keeps it row for row (K = 2 and 3 included, where one row fewer would do) and renders what it always rendered.
inline int dof_halo_rows(int K, int W)
{
    const int zlo = dof_tap_lo(K), zhi = dof_tap_hi(K);
    const int one_wrap = std::max(-zlo, zhi - 1) + 1;
    if (W < 3) return one_wrap;                      // (no interior pixel: nothing is blurred)
    const int above = -(zlo + dof_floor_div(1 + zlo, W)), below = zhi - 1 + dof_floor_div(W - 3 + zhi, W);
    return std::max(one_wrap, std::max(above, below));
}

}  // namespace mirt
