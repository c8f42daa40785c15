// count_hits.hpp -- the parameter blocks and the kernels of mirt_count_hits* (count_hits.hip: the sweeps; count_along.hip: the walks
// through the grids of ../along/along.hpp; the rule: count_rule.hpp; the host: ../capi/count.cpp).
#pragma once

#include "count_rule.hpp"
#include "../along/alongs.hpp"

namespace mirt {

// What a count call adds to the rays it runs on: the block every frame below embeds and the host passes from entry point to launch.
struct CountOut {
    const uint32_t *after;       // nrays records of HIT_WORDS words, or NULL: only distance and index are read
    const float *limit;          // nrays limits, used as given, or NULL: +inf
    int32_t *counts;             // the OUTPUT: nrays
};

// A sweep: the scene's rows and the caller's rays (q.hits is not read).
struct CountFrame {
    QueryFrame q;
    CountOut out;
};
// A call along a direction (along.hpp: AlongFrame; a.q.hits, a.limit and a.occluded are not read) ...
struct AlongCountFrame {
    AlongFrame a;
    CountOut out;
};
// ... and one pass of a call along several (alongs.hpp: AlongsFrame).  The pass with a.first == 0 writes the count 0 of a ray whose
// index lies outside [0, ndirs), which belongs to no pass.
struct AlongsCountFrame {
    AlongsFrame a;
    CountOut out;
};

// Rays per lane of the lane-per-ray sweep, as k_query_closest's QUERY_P.
constexpr int COUNT_P = 2;
constexpr int COUNT_BLOCK_RAYS = 256 * COUNT_P;

__attribute__((global)) void k_count_wave(const CountFrame);
template <int P> __attribute__((global)) void k_count_lanes(const CountFrame);
template <bool STATS> __attribute__((global)) void k_along_count(const AlongCountFrame);
template <bool STATS> __attribute__((global)) void k_alongs_count(const AlongsCountFrame);

}  // namespace mirt
