// ordered_fans.hip -- hand-written gfx950 kernels of mirt_intersect_ordered_from* and mirt_intersect_ordered_fans*: the max_hits first
// triangles along each of the rays {origin, dirs[i]} or {origins[origin_of[i]], dirs[i]} in the reference's own order (hit_list.hpp),
// behind an optional `after` record, bit for bit -- through the cube around the origin that mirt_intersect_from* and
// mirt_intersect_fans* walk (../query/rt_query.hip; the same tables: a cube one family builds serves the other).
//
// The walk is fan_walk's: one lane per ray over the list of its direction's bin, front to back in depth shells of the rows' `near`
// bound, no LDS, state in plain registers, every step straight-line code (a lane with no row left loads row 0 and ignores it),
// verdicts as integers combined with `&`, only the exact stage in a divergent branch, the next row fetched by walk_row / walk_step.
// Every test is the fan's own (test_dots on the origin's row, maybe_hit, exact_hit on tris15 and the origin S, negD = -dir).  What
// differs is what an accepted distance does: it is offered to the K-entry list (hit_list_consider), and the bound that moves the
// list's end and skips a row by its `near` is the list's K-th distance -- FLT_MAX until K entries are held (order_bound.hpp has the
// lines and the argument).  The end and the skip are strict, so the ties at the bound are still tested and the index decides them.
// No shell is skipped for lying in front of `after`: a row has no upper depth bound, and a ray that continues walks its first
// shells again.  A lane whose direction fan_dir_of does not form sweeps its origin's full table behind the wave's walk (k_query_fan's
// loop body with the per-ray exact-only override) into the same list; a lane whose `after` distance is NaN takes no list and still
// writes its slots and its count.
// Positions do not travel with the keys: the winners are tested once more at the end, with the very test the walk ran (the origin
// table's row of the winner and tris15: the same operations on the same operands, no fused forms), which gives the position's bits.
// Built with -ffp-contract=off like every kernel of the library.
#include "ordered_fans.hpp"
#include "order_bound.hpp"
#include "order_device.hpp"

namespace mirt {

// `mine`: the lane has a ray of this launch (a ray inside the call, and of this pass's origins): any other lane takes no list, sweeps
// nothing and writes no slot -- it reads position 0's values (fans_lane); `zero`: the lane's count is written 0 though the ray is
// not of this launch (a ray whose index names no origin of the call).  `ray` must index the call's arrays whenever `mine` or `zero`
// is set.  The `after` record of a ray is read before any of its slots is written, by the lane that writes them, and a ray is
// `mine` in exactly one pass: a call that peels in place (after == hits, max_hits == 1) may run in passes.
// k: the position of the ray's origin in the cube, S the origin, bin_base the first bin of position k, tab its origin table.
template <int K, bool STATS>
__device__ __forceinline__ void fan_order_walk(const QueryFanFrame &q, long long ray, bool ok, bool mine, bool zero, uint32_t k, v3 S, uint32_t bin_base,
                                               const OriginRow *tab, const OrderOut &o)
{
    const CubeView &cv = q.cube;
    const float4 *rows4 = reinterpret_cast<const float4 *>(cv.light_rows);
    const v3 dir = ld3(q.dirs + 3 * (size_t)(ok ? ray : 0));
    const v3 nd = neg3(dir);                                       // negD = -dir (:229); dir is used as given
    float a;
    int ak;
    order_after(o, ray, mine, &a, &ak);
    const bool open = mine && a == a;                              // (a NaN record admits nothing: no walk)
    const FanDir fd = fan_dir_of(nd);
    const bool binned = open && fd.formed, swept = open && !fd.formed;
    const BinFrameDesc *lf = cv.light_frames + 6 * (size_t)k;
    const float d0 = lf->shell_d0, iw = lf->shell_iw;
    HitList<K> hl;
    hit_list_clear(hl);
    float bound = order_bound(hit_list_bound(hl));
    uint32_t e = 0u, end = 0u, key = 0u;
    if (binned) key = fan_list(cv, k, bin_base, fd.d, bound, &e, &end);
    unsigned long long n_cand = 0, n_tests = 0;
    float4 c0, c1, c2;
    walk_row(rows4, e < end ? e : 0u, c0, c1, c2);
    for (;;) {
        const int act = (int)(e < end);
        if (!__any(act)) break;
        const TestDots td = test_dots(c0, c1, c2, nd);
        const int near_ok = act & (int)order_near_ok(c1.w, bound);         // strictly beyond the K-th entry: cannot enter the list
        if (STATS) { n_cand += (unsigned)act; n_tests += (unsigned)near_ok; }
        if (near_ok & (int)maybe_hit(td)) {
            const int tri = (int)cv.light_tri[e];
            v3 hp;
            float dist;
            if (exact_hit(td, c0.w, q.tris15 + (size_t)15 * tri, S, &hp, &dist)) {
                hit_list_consider(hl, dist, tri, a, ak);
                const float b = order_bound(hit_list_bound(hl));
                if (b < bound) {                                   // (the K-th entry arrived or moved in: so does the list's end)
                    bound = b;
                    end = min(end, cv.light_off[key + order_shells(bin_shell_of(b, d0, iw, cv.shells))]);
                }
            }
        }
        walk_step(rows4, e, end, act & (int)(e + 1u < end), c0, c1, c2);   // (the list's end, old or new: the lane is through)
    }
    if (__any(swept)) {
        // (rare) the lanes the bins do not cover: their origin's full table, k_query_fan's loop body into the same list
        const bool exact_only = !dir_in_filter_range(dir);
        if (STATS && swept) { n_cand += (unsigned)q.n; n_tests += (unsigned)q.n; }
        for (int j = 0; j < q.n; j++) order_offer_origin_row(hl, tab, q.tris15, j, S, nd, swept, exact_only, a, ak);
    }
    if (mine) order_store_list(o, ray, hl, OriginRetest{ tab, q.tris15, S, nd });
    else if (zero) o.counts[ray] = 0;
    if (STATS) flush_query_stats(q.stats, mine ? 1u : 0u, n_cand, n_tests, swept ? 1u : 0u);
}

// ---- k_fan_order: one origin; k, the bin base and S are launch-uniform (k_query_fan_binned's shape) ---------------------------------
template <int K, bool STATS>
__global__ __launch_bounds__(256) void k_fan_order(const FanOrderFrame f)
{
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = ray < f.f.nrays;
    fan_order_walk<K, STATS>(f.f, ray, ok, ok, false, 0u, ld3(f.f.origin), 0u, f.f.tab, f.out);
}

// ---- k_fans_order: one pass of a many-origin call, each lane's position from its ray's index (k_query_fans_binned's shape) ---------
template <int K, bool STATS>
__global__ __launch_bounds__(256) void k_fans_order(const FansOrderFrame f)
{
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = ray < f.f.f.nrays;
    const FansLane l = fans_lane(f.f, ray, ok);
    const bool nobodys = ok && f.f.first == 0 && l.idx >= (uint32_t)f.norigins;
    fan_order_walk<K, STATS>(f.f.f, ray, ok, l.mine, nobodys, l.k, l.S, l.bin_base, l.tab, f.out);
}

#define MIRT_ORDER_FANS_INSTANCES(K)                                                  \
    template __global__ void k_fan_order<K, false>(const FanOrderFrame);              \
    template __global__ void k_fan_order<K, true>(const FanOrderFrame);               \
    template __global__ void k_fans_order<K, false>(const FansOrderFrame);            \
    template __global__ void k_fans_order<K, true>(const FansOrderFrame);
MIRT_ORDER_FANS_INSTANCES(1)
MIRT_ORDER_FANS_INSTANCES(2)
MIRT_ORDER_FANS_INSTANCES(4)
MIRT_ORDER_FANS_INSTANCES(8)
#undef MIRT_ORDER_FANS_INSTANCES

}  // namespace mirt
