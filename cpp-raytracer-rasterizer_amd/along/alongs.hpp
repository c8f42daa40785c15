// alongs.hpp -- ray queries along SEVERAL directions in one call (mirt_intersect_alongs*, mirt_occluded_alongs*): the rays
// {origins[i], dirs[dir_of[i]]}.  Each direction's part of the structure is exactly the single-direction grid of along.hpp -- the
// same along_make_desc, the same along_tri_setup / along_cell_may_hit, the same rows -- so nothing of the predicate or its proof
// changes; what is new is that a GROUP of directions shares one build chain: direction `slot` of the group files its pairs under
// the keys slot * along_keys + (cell * shells + shell) of ONE pair list, one sort orders them and one offset table bounds every
// slot's lists (../capi/along_plan.hpp has the arithmetic, DESIGN.md section 5.1 the argument).  The parameter blocks of alongs.hip.
#pragma once

#include "along.hpp"

namespace mirt {

// The build of a group: one lane per (triangle, slot) files the triangle for the slot's direction (k_alongs_pairs), the sort
// orders the pairs, k_alongs_rows expands them.  A pair's value is slot * n + triangle: the row of `near` it belongs to.
struct AlongsPairs {
    const AlongDesc *descs;      // the group's descriptors, one a slot (device)
    int slots;
    uint32_t keys_per_slot;      // along_keys(B, shells)
    const QueryRow *qrows;
    int n;
    uint32_t *counters;          // [0] pairs, [1 + slot] triangles on the slot's every-ray list
    uint32_t *keys, *vals;
    uint32_t cap;
    uint32_t *bucket_cnt;        // nbuckets counts for bucket_sort_pairs (../csrc/bin_sort.hpp)
    uint32_t nbuckets;
    int bucket_shift;
    float *near;                 // slots x n: the triangles' depth bounds per slot, for k_alongs_rows
};
struct AlongsRows {
    const uint32_t *entries;     // slot * n + triangle, in key order
    const uint32_t *total;       // their number
    const QueryRow *qrows;
    const float *near;
    uint32_t n;
    QueryRow *rows;
    AlongAux *aux;
};

// One pass of a call: the group's tables, its descriptors and directions (device tables, `count` entries each, staged per
// workgroup), and the range [first, first + count) of the call's list the group holds.  A lane whose index lies outside the range
// -- another pass's ray, or an index outside the call's list -- takes no list, sweeps nothing and leaves its record unwritten.
struct AlongsFrame {
    QueryFrame q;
    const AlongDesc *descs;
    const float *dirs;           // count x 3, as the caller gave them
    const uint32_t *off;         // count * keys_per_slot + 1
    const QueryRow *rows;        // never NULL
    const AlongAux *aux;
    uint32_t keys_per_slot;
    const float *origins;        // nrays x 3
    const int32_t *dir_of;       // nrays indices into the call's list, or NULL: every ray takes direction 0
    int first, count, ndirs;
    const float *limit;          // k_alongs_occluded: nrays limits or NULL
    uint8_t *occluded;           // k_alongs_occluded: nrays bytes; the pass with first == 0 writes 0 for indices outside [0, ndirs)
    unsigned long long *stats;   // QSTAT_WORDS counters (the STATS instantiations): the passes add up in the same words
};
// The rays written out for the brute-force kernels: ray i = { origins[3 i ..], dirs[3 dir_of[i] ..] }, or the ray no triangle accepts
// (NaN start, zero direction) for an index outside [0, ndirs).
struct AlongsExpand {
    const float *origins;
    const float *dirs;           // ndirs x 3 (device)
    const int32_t *dir_of;
    int ndirs, nrays;
    float *rays;                 // nrays x RAY_WORDS
};

__attribute__((global)) void k_alongs_pairs(const AlongsPairs);
__attribute__((global)) void k_alongs_rows(const AlongsRows);
__attribute__((global)) void k_alongs_expand(const AlongsExpand);
template <bool STATS> __attribute__((global)) void k_alongs_closest(const AlongsFrame);
template <bool STATS> __attribute__((global)) void k_alongs_occluded(const AlongsFrame);

}  // namespace mirt
