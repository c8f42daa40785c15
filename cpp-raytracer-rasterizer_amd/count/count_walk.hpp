// count_walk.hpp -- the walk of the hit counts along a direction (device code): k_along_count and k_alongs_count (count_along.hip)
// run this one body over the tables of ../along/along.hpp, with their lanes from ../along/along_lanes.hpp.
//
// The walk has the shape of along_occluded_walk (../along/along_walk.hpp) without `done`: one lane per ray over its cell's list, front
// to back in depth shells, then the every-ray list; every step straight-line code for every lane (a lane with no row left loads row 0
// and ignores it), only the exact stage in a divergent branch.  The list's end and the strict row reject are that walk's, under the
// threshold count_threshold(rs, L) (count_rule.hpp): the end never moves, because nothing ends a count early.
//
// Why the count is exact: every row is offered to a ray at most once.  A ray walks exactly two lists, its cell's and the every-ray
// list; along_file_triangles (../along/along_file.hpp) puts a triangle EITHER on the every-ray list once OR once into each cell of its
// box, so no row stands twice on one list nor on both of a ray's; a lane is either binned or swept, never both; and in a call of
// several passes a ray is `mine` in exactly one.  That every row the reference accepts for the ray is offered is the structure's own
// argument (along.hpp), which the closest-hit and occlusion walks rest on too.
#pragma once

#include "count_device.hpp"
#include "../along/along_lanes.hpp"

namespace mirt {

// `mine`: the lane has a ray of this launch (a ray inside the call, and of this pass's directions): any other lane takes no list and
// sweeps nothing; `zero`: the lane's count is written 0 though the ray is not of this launch (a ray whose index names no direction of
// the call).  `ray` must index the call's arrays whenever `mine` or `zero` is set.
template <bool STATS>
__device__ __forceinline__ void along_count_walk(const QueryFrame &q, const AlongTables &t, const AlongLane &l, long long ray, bool mine, bool zero,
                                                 const CountOut &o, unsigned long long *stats)
{
    const CountRay cr = count_ray_of(o, ray, mine);
    const bool binned = cr.open && l.in_reach, swept = cr.open && !l.in_reach;
    const float thr = count_threshold(l.rs, cr.L);
    uint32_t e = 0u, end = 0u, e2 = 0u, end2 = 0u;
    if (binned) { e2 = t.off[l.every]; end2 = t.off[l.every + 1u]; }
    if (binned && l.has_cell) { e = t.off[l.key]; end = along_list_end(t, l, thr); }
    int stage = 0;
    if (!(e < end)) { e = e2; end = end2; stage = 1; }
    unsigned long long n_cand = 0, n_tests = 0;
    int cnt = 0;
    float4 c0, c1, c2;
    AlongAux ax;
    along_row(t, e < end ? e : 0u, c0, c1, c2, ax);
    for (;;) {
        const int act = (int)(e < end);
        if (!__any(act)) break;
        const RowVecs r = unpack_row(c0, c1, c2);
        float e1e2b;
        const TestDots td = ray_dots(r, l.S, l.nd, &e1e2b);
        const int near_ok = act & (int)order_near_ok(ax.near, thr);    // every point of the row is beyond the limit: cannot pass `<`
        if (STATS) { n_cand += (unsigned)act; n_tests += (unsigned)near_ok; }
        if (near_ok & (int)maybe_hit(td)) {
            v3 hp;
            float dist;
            if (exact_hit_row(td, e1e2b, r, l.S, &hp, &dist)) cnt += count_hit(cr, dist, (int)ax.tri);
        }
        // on to the next row of the list, else to the every-ray list, else the lane is through
        const int cont = act & (int)(e + 1u < end);
        const int turn = (cont ^ 1) & (int)(stage == 0);
        e = cont ? e + 1u : (turn ? e2 : end);
        end = turn ? end2 : end;
        stage |= turn;
        along_row(t, e < end ? e : 0u, c0, c1, c2, ax);
    }
    if (__any(swept)) {
        // (rare) the lanes the structure does not cover: every row of the scene once, in index order
        if (STATS && swept) { n_cand += (unsigned)q.n; n_tests += (unsigned)q.n; }
        for (int j = 0; j < q.n; j++) {
            const float4 *src = reinterpret_cast<const float4 *>(q.rows + j);
            cnt += count_row(cr, unpack_row(src[0], src[1], src[2]), j, l.S, l.nd, swept, l.exact_only);
        }
    }
    if (mine || zero) o.counts[ray] = cnt;
    if (STATS) flush_query_stats(stats, mine ? 1u : 0u, n_cand, n_tests, swept ? 1u : 0u);
}

}  // namespace mirt
