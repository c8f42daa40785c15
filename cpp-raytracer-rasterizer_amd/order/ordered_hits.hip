// ordered_hits.hip -- hand-written gfx950 kernels of mirt_intersect_ordered*: the max_hits first triangles along each ray in the
// reference's own order (hit_list.hpp), behind an optional `after` record, bit for bit.
//
// Every (ray, triangle) test is k_query_closest's own: the scene's QueryRow, ray_dots, the conservative filter (maybe_hit) with the
// per-ray exact-only override (ray_exact_only) in front of exact_hit_row, on the caller's start and negD = -dir.  What differs is
// what an accepted distance does: it is offered to a list of the K best keys in registers (hit_list_offer) instead of replacing one
// record.  The list does not care in which order rows arrive nor whether one arrives twice -- equal keys are the same triangle and
// the second is dropped --, and the `after` record only removes candidates, so the three kernels below differ only in which rows
// they offer:
//   k_order_sweep<K>       a lane per ray, all rows staged through LDS in chunks (k_query_closest's structure, one ray a lane);
//   k_order_sweep_wave<K>  a wave per ray, lanes stride over the rows and keep the K best of their own, then K extraction rounds;
//   k_grid_order<K, STATS> a lane per ray through the cell grid (k_grid_closest's walk), reach = the list's bound.
// Positions do not travel with the keys: the K winners are tested once more at the end (exact_hit_row on the winner's row gives the
// same bits -- the same operations on the same operands, no fused forms) and the list stays at two registers an entry
// (order_device.hpp: order_after, order_offer_row, order_store_slot, order_store_list, which all ordered kernels share).
// The `after` record of a ray is read before any of its slots is written, by the lane or wave that writes them: with max_hits == 1
// the caller may pass the output array itself.
// Built with -ffp-contract=off like every kernel of the library.
#include "ordered_hits.hpp"
#include "order_device.hpp"
#include "../grid/ray_grid_device.hpp"

namespace mirt {

// Whether ray `ray` of a call whose rays were written out from (origins, directions, dir_of) names a direction of the call's list
// (o.dir_of NULL: every ray does).  One that names none keeps its slots as the caller left them and gets the count 0.
__device__ __forceinline__ bool order_named(const OrderFrame &o, long long ray)
{
    return !o.dir_of || (uint32_t)o.dir_of[ray] < (uint32_t)o.ndirs;
}

// ---- k_order_sweep: one lane per ray, every ray tests every triangle -------------------------------------------------------------------
// Workgroup = 256 lanes = 256 rays.  The rows are staged through LDS in chunks of RT_CHUNK_ROWS and read as wave-uniform broadcasts.
template <int K>
__global__ __launch_bounds__(256) void k_order_sweep(const OrderFrame o)
{
    extern __shared__ __attribute__((aligned(16))) float4 s_rows[];
    const QueryFrame &q = o.f.q;
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = ray < q.nrays;
    const float *rp = q.rays + (size_t)RAY_WORDS * (ok ? ray : 0);
    const v3 start = ld3(rp), dir = ld3(rp + 3);
    const v3 nd = neg3(dir);                                       // negD = -dir (:229); dir is used as given
    const bool exact_only = ray_exact_only(scene_rows_in_range(q), start, dir);
    float a;
    int k;
    order_after(o.out, ray, ok, &a, &k);
    HitList<K> l;
    hit_list_clear(l);

    for (int base = 0; base < q.n; base += RT_CHUNK_ROWS) {
        const int cnt = min(RT_CHUNK_ROWS, q.n - base);
        stage_rows(s_rows, q.rows + base, cnt);
#pragma unroll 2
        for (int j = 0; j < cnt; j++)
            order_offer_row(l, unpack_row(s_rows[3 * j], s_rows[3 * j + 1], s_rows[3 * j + 2]), base + j, start, nd, true, exact_only, a, k);
    }
    if (ok && order_named(o, ray)) order_store_list(o.out, ray, l, SceneRetest{ q.rows, start, nd });
    else if (ok) o.out.counts[ray] = 0;                            // (a ray of the along calls that names no direction: slots untouched)
}

template __global__ void k_order_sweep<1>(const OrderFrame);
template __global__ void k_order_sweep<2>(const OrderFrame);
template __global__ void k_order_sweep<4>(const OrderFrame);
template __global__ void k_order_sweep<8>(const OrderFrame);

// ---- k_order_sweep_wave: one WAVE per ray, lanes over triangles ------------------------------------------------------------------------
// k_query_closest_wave's shape: the 64 lanes stride over the rows in global memory and each keeps the K best of its own triangles.
// The wave's K best are among them.  Round s takes the smallest list head of the wave (wave_min_key), the one lane that owns it -- a
// row is seen by one lane -- pops it, and lane s keeps it as slot s; then lanes 0 .. max_hits - 1 write a slot each.
template <int K>
__global__ __launch_bounds__(256) void k_order_sweep_wave(const OrderFrame o)
{
    const QueryFrame &q = o.f.q;
    const int lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= q.nrays) return;                                    // (the whole wave)
    const float *rp = q.rays + (size_t)RAY_WORDS * ray;
    const v3 start = ld3(rp), dir = ld3(rp + 3);
    const v3 nd = neg3(dir);                                       // :229
    const bool exact_only = ray_exact_only(scene_rows_in_range(q), start, dir);
    float a;
    int k;
    order_after(o.out, ray, true, &a, &k);
    HitList<K> l;
    hit_list_clear(l);

    for (int i = lane; i < q.n; i += 64) order_offer_row(l, order_row(q.rows, i), i, start, nd, true, exact_only, a, k);

    unsigned long long mine = HIT_KEY_NONE;
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < K; s++)
        if (s < o.out.max_hits) {                                  // (wave-uniform)
            const unsigned long long best = wave_min_key(l.k[0]);
            if (l.k[0] == best) hit_list_pop(l);                   // (all heads empty: popping changes nothing)
            if (lane == s) mine = best;
            cnt += (int)(best != HIT_KEY_NONE);
        }
    if (lane < o.out.max_hits && order_named(o, ray)) order_store_slot(o.out, ray, lane, mine, SceneRetest{ q.rows, start, nd });
    if (lane == 0) o.out.counts[ray] = cnt;
}

template __global__ void k_order_sweep_wave<1>(const OrderFrame);
template __global__ void k_order_sweep_wave<2>(const OrderFrame);
template __global__ void k_order_sweep_wave<4>(const OrderFrame);
template __global__ void k_order_sweep_wave<8>(const OrderFrame);

// ---- k_grid_order: one lane per ray through the cell grid ------------------------------------------------------------------------------
// k_grid_closest's walk -- cells slab by slab, plane index, every-ray list, the swept fallback for the lanes the structure does not
// cover -- with the list in place of the record.  The walk's reach is the list's bound times 1 + 2^-20, +inf until the list is full:
// an accepted pair of distance d is offered under every reach >= d (ray_grid.hpp), so once K entries at or below the bound are held,
// a pair the cells' end cuts off lies strictly beyond the bound and could not enter; the end is strict, so ties at the bound are
// still offered.  No cell is skipped for lying in front of `after`: a ray that continues walks its first cells again.
template <int K, bool STATS>
__global__ __launch_bounds__(256) void k_grid_order(const OrderFrame o)
{
    const GridFrame &f = o.f;
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool mine = ray < f.q.nrays;
    const GridLane gl = grid_lane(f, ray, mine);
    float a;
    int k;
    order_after(o.out, ray, mine, &a, &k);
    const bool open = mine && a == a;                            // (a NaN record admits nothing: no walk)
    const bool swept = open && !gl.fit;
    bool live = open && gl.fit;
    GridWalk w = grid_walk_begin(f.v.d, gl.S, V3(-gl.nd.x, -gl.nd.y, -gl.nd.z), live);
    HitList<K> l;
    hit_list_clear(l);
    float bound = __uint_as_float(0x7f800000u);
    uint32_t e = 0u, end = 0u;
    int src = 0;
    unsigned long long c[GSTAT_WORDS] = {};
    const float4 *rows4 = reinterpret_cast<const float4 *>(f.v.rows);
    for (;;) {
        grid_step_rows(f.v, w, (double)bound * (1.0 + 9.5367431640625e-7), live, e, end, src);
        if (!__any(live)) break;
        const int act = (int)(live && e < end);
        if (!__any(act)) continue;                                 // (a round of steps only)
        float4 c0, c1, c2;
        walk_row(rows4, act ? e : 0u, c0, c1, c2);
        const int tri = (int)f.v.tri[act ? e : 0u];
        const RowVecs r = unpack_row(c0, c1, c2);
        float e1e2b;
        const TestDots td = ray_dots(r, gl.S, gl.nd, &e1e2b);
        if (STATS) {
            c[GSTAT_ROWS_CELLS] += (unsigned)(act & (int)(src == 0));
            c[GSTAT_ROWS_PLANES] += (unsigned)(act & (int)(src == 1));
            c[GSTAT_ROWS_EVERY] += (unsigned)(act & (int)(src == 2));
            c[GSTAT_TESTS] += (unsigned)act;
        }
        if (act & (int)maybe_hit(td)) {
            v3 hp;
            float dist;
            if (exact_hit_row(td, e1e2b, r, gl.S, &hp, &dist)) {
                hit_list_consider(l, dist, tri, a, k);
                bound = hit_list_bound(l);
            }
        }
        e += (uint32_t)act;
    }
    if (__any(swept)) {
        // (rare) the lanes the structure does not cover: every row of the scene
        if (STATS && swept) { c[GSTAT_TESTS] += (unsigned)f.q.n; c[GSTAT_SWEPT] = 1; }
        order_sweep_tail(l, f.q.rows, f.q.n, gl.S, gl.nd, swept, gl.exact_only, a, k);
    }
    if (mine) order_store_list(o.out, ray, l, SceneRetest{ f.q.rows, gl.S, gl.nd });
    if (STATS) { c[GSTAT_RAYS] = mine ? 1u : 0u; flush_grid_stats(f.stats, c); }
}

template __global__ void k_grid_order<1, false>(const OrderFrame);
template __global__ void k_grid_order<1, true>(const OrderFrame);
template __global__ void k_grid_order<2, false>(const OrderFrame);
template __global__ void k_grid_order<2, true>(const OrderFrame);
template __global__ void k_grid_order<4, false>(const OrderFrame);
template __global__ void k_grid_order<4, true>(const OrderFrame);
template __global__ void k_grid_order<8, false>(const OrderFrame);
template __global__ void k_grid_order<8, true>(const OrderFrame);

}  // namespace mirt
