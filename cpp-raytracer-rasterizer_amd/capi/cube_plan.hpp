// cube_plan.hpp -- the arithmetic that sizes a light cube and splits a list of positions over several cubes, free of library state:
// binned.cpp (light_cube_bins_for, light_keys_fit) and query.cpp (mirt_intersect_fans*) apply it to the uploaded scene, and
// tests/cpp/fans_plan_test.cpp checks it on the CPU.
#pragma once

#include "../csrc/bin_sort.hpp"
#include "../csrc/rt_binned.hpp"

#include <algorithm>
#include <vector>

namespace mirt {

// Most sort keys (bin * depth shells + shell) one binning pass may use: the two-level counting sort keeps one LDS counter per
// bucket of at most 1024 keys (bin_bucket_sort.hip).  The callers choose their grids and shell counts to stay below it.
constexpr uint32_t BIN_MAX_KEYS = BUCKET_SORT_MAX_BUCKETS * 1024u - 1u;

// Bins per face side of the cubes of `nlights` positions in a scene of n triangles; cube_override: MIRT_CUBE_BINS (64 | 128 | 256
// fixes the grid, anything else leaves it to the scene's size).  The rule's reasons: binned.cpp, light_cube_bins_for.
inline int cube_bins_rule(int n, int nlights, int cube_override, bool *fixed_grid)
{
    int fine_bins = n < 2000 ? CUBE_BINS_MIN : (n < 20000 ? 2 * CUBE_BINS_MIN : 4 * CUBE_BINS_MIN);
    const bool fixed = cube_override == 64 || cube_override == 128 || cube_override == 256;
    if (fixed_grid) *fixed_grid = fixed;
    if (fixed) fine_bins = cube_override;
    // (many light positions -- 16 soft-shadow samples of two lights -- at the finest grid are more keys than one sort pass holds)
    while (fine_bins > CUBE_BINS_MIN && 6ll * fine_bins * fine_bins * nlights * 4 > (long long)BIN_MAX_KEYS) fine_bins /= 2;
    return fine_bins;
}

inline bool cube_keys_fit(int nlights, int cube_bins)
{
    return 6ll * cube_bins * cube_bins * std::max(nlights, 1) + 64 <= (long long)BIN_MAX_KEYS;
}

// One pass of a many-origin fan call: origins [first, first + count) of the call's list in one cube on a grid of cube_bins.
struct FanPass { int first, count, cube_bins; };

// The passes of a call with `norigins` origins against a scene of n triangles: consecutive ranges that tile [0, norigins), each
// the longest a cube takes -- at most MIRT_MAX_LIGHTS positions, and no more than cube_keys_fit allows at the grid cube_bins_rule
// chooses for that many.  False (and an empty plan) when not even one position fits a cube: the call cannot be binned.
inline bool fan_pass_plan(int norigins, int n, int cube_override, std::vector<FanPass> *plan)
{
    plan->clear();
    for (int first = 0; first < norigins;) {
        int count = std::min(norigins - first, (int)MIRT_MAX_LIGHTS);
        while (count > 0 && !cube_keys_fit(count, cube_bins_rule(n, count, cube_override, nullptr))) count--;
        if (count == 0) { plan->clear(); return false; }
        plan->push_back({ first, count, cube_bins_rule(n, count, cube_override, nullptr) });
        first += count;
    }
    return true;
}

}  // namespace mirt
