// ordered_along.hip -- hand-written gfx950 kernels of mirt_intersect_ordered_along* and mirt_intersect_ordered_alongs*: the max_hits
// first triangles along each of the rays {origins[i], dir} or {origins[i], dirs[dir_of[i]]} in the reference's own order
// (hit_list.hpp), behind an optional `after` record, bit for bit -- through the grid across the direction that mirt_intersect_along*
// and mirt_intersect_alongs* walk (../along/along.hpp; the same tables: a grid one family builds serves the other).
//
// The walk is along_closest_walk's (../along/along_walk.hpp): one lane per ray over its cell's list, front to back in depth shells,
// then the every-ray list; every test is k_query_closest's own (ray_dots, maybe_hit, exact_hit_row on the caller's start and
// negD = -dir).  What differs is what an accepted distance does: it is offered to the K-entry list (hit_list_consider), and the
// bound that moves the cell list's end and skips a row by its depth bound is the list's K-th distance -- FLT_MAX until K entries are
// held (order_bound.hpp has the lines and the argument).  The end and the skip are strict, so the ties at the bound are still
// tested and the index decides them.  The every-ray list has no depth order and is walked whole; a row that is both in the cell and
// on that list offers an equal key, which the list drops.  No shell is skipped for lying in front of `after`: a ray that continues
// walks its first shells again.  A lane the structure does not cover sweeps all n rows behind the wave's walk (order_device.hpp:
// order_sweep_tail); a lane whose `after` distance is NaN takes no list and still writes its slots and its count.
// Positions do not travel with the keys: the winners are tested once more at the end (order_device.hpp).
// Built with -ffp-contract=off like every kernel of the library.
#include "ordered_along.hpp"
#include "order_bound.hpp"
#include "order_device.hpp"
#include "../along/along_lanes.hpp"

namespace mirt {

// The cell list's end under the threshold `thr`: the shells up to the one thr falls into (along_walk.hpp: along_list_end).
__device__ __forceinline__ uint32_t along_order_end(const AlongTables &t, const AlongLane &l, float thr)
{
    return t.off[l.key + order_shells(bin_shell_of(thr, l.shell_d0, l.shell_iw, l.shells))];
}

// `mine`: the lane has a ray of this launch (a ray inside the call, and of this pass's directions): any other lane takes no list,
// sweeps nothing and writes no slot; `zero`: the lane's count is written 0 though the ray is not of this launch (a ray whose index
// names no direction of the call).  `ray` must index the call's arrays whenever `mine` or `zero` is set.  The `after` record of a
// ray is read before any of its slots is written, by the lane that writes them.
template <int K, bool STATS>
__device__ __forceinline__ void along_order_walk(const QueryFrame &q, const AlongTables &t, const AlongLane &l, long long ray, bool mine, bool zero,
                                                 const OrderOut &o, unsigned long long *stats)
{
    float a;
    int k;
    order_after(o, ray, mine, &a, &k);
    const bool open = mine && a == a;                              // (a NaN record admits nothing: no walk)
    const bool binned = open && l.in_reach, swept = open && !l.in_reach;
    HitList<K> hl;
    hit_list_clear(hl);
    float thr = along_order_threshold(l.rs, order_bound(hit_list_bound(hl)));
    uint32_t e = 0u, end = 0u, e2 = 0u, end2 = 0u;
    if (binned) { e2 = t.off[l.every]; end2 = t.off[l.every + 1u]; }
    if (binned && l.has_cell) { e = t.off[l.key]; end = along_order_end(t, l, thr); }
    int stage = 0;
    if (!(e < end)) { e = e2; end = end2; stage = 1; }
    unsigned long long n_cand = 0, n_tests = 0;
    float4 c0, c1, c2;
    AlongAux ax;
    along_row(t, e < end ? e : 0u, c0, c1, c2, ax);
    for (;;) {
        const int act = (int)(e < end);
        if (!__any(act)) break;
        const RowVecs r = unpack_row(c0, c1, c2);
        float e1e2b;
        const TestDots td = ray_dots(r, l.S, l.nd, &e1e2b);
        const int near_ok = act & (int)order_near_ok(ax.near, thr);
        if (STATS) { n_cand += (unsigned)act; n_tests += (unsigned)near_ok; }
        if (near_ok & (int)maybe_hit(td)) {
            v3 hp;
            float dist;
            if (exact_hit_row(td, e1e2b, r, l.S, &hp, &dist)) {
                hit_list_consider(hl, dist, (int)ax.tri, a, k);
                thr = along_order_threshold(l.rs, order_bound(hit_list_bound(hl)));
                if (stage == 0) end = min(end, along_order_end(t, l, thr));
            }
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
        // (rare) the lanes the structure does not cover: every row of the scene
        if (STATS && swept) { n_cand += (unsigned)q.n; n_tests += (unsigned)q.n; }
        order_sweep_tail(hl, q.rows, q.n, l.S, l.nd, swept, l.exact_only, a, k);
    }
    if (mine) order_store_list(o, ray, hl, SceneRetest{ q.rows, l.S, l.nd });
    else if (zero) o.counts[ray] = 0;
    if (STATS) flush_query_stats(stats, mine ? 1u : 0u, n_cand, n_tests, swept ? 1u : 0u);
}

// ---- k_along_order: one direction, its descriptor in the kernel's arguments (k_along_closest's shape) ------------------------------
template <int K, bool STATS>
__global__ __launch_bounds__(256) void k_along_order(const AlongOrderFrame f)
{
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = ray < f.a.q.nrays;
    const AlongTables t = { f.a.v.off, f.a.v.rows, f.a.v.aux };
    along_order_walk<K, STATS>(f.a.q, t, along_lane(f.a, ray, ok), ray, ok, false, f.out, f.a.stats);
}

// ---- k_alongs_order: a group of directions, each lane's descriptor out of LDS by its ray's index (k_alongs_closest's shape) --------
template <int K, bool STATS>
__global__ __launch_bounds__(256) void k_alongs_order(const AlongsOrderFrame f)
{
    __shared__ __attribute__((aligned(8))) uint32_t s_desc[MIRT_MAX_LIGHTS * ALONGS_DESC_WORDS];
    __shared__ float s_dir[MIRT_MAX_LIGHTS * 3];
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const AlongsLane a = alongs_lane(f.a, s_desc, s_dir, ray, ray < f.a.q.nrays);
    const AlongTables t = { f.a.off, f.a.rows, f.a.aux };
    along_order_walk<K, STATS>(f.a.q, t, a.l, ray, a.mine, a.zero, f.out, f.a.stats);
}

#define MIRT_ORDER_ALONG_INSTANCES(K)                                                   \
    template __global__ void k_along_order<K, false>(const AlongOrderFrame);            \
    template __global__ void k_along_order<K, true>(const AlongOrderFrame);             \
    template __global__ void k_alongs_order<K, false>(const AlongsOrderFrame);          \
    template __global__ void k_alongs_order<K, true>(const AlongsOrderFrame);
MIRT_ORDER_ALONG_INSTANCES(1)
MIRT_ORDER_ALONG_INSTANCES(2)
MIRT_ORDER_ALONG_INSTANCES(4)
MIRT_ORDER_ALONG_INSTANCES(8)
#undef MIRT_ORDER_ALONG_INSTANCES

}  // namespace mirt
