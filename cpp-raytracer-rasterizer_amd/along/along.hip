// along.hip -- hand-written gfx950 kernels of the ray queries along one direction (mirt_intersect_along*, mirt_occluded_along*;
// along.hpp has the structure and the predicate, DESIGN.md section 5.1 the argument).
//
// The build (once per scene version and direction): k_along_pairs files every triangle -- a (cell, shell) key per cell its region
// may reach, or the one key of the every-ray list --, bucket_sort_pairs (../csrc/bin_sort.hpp) orders the pairs, k_along_rows
// writes the 48-byte QueryRow of each pair in key order with the triangle's index and depth bound alongside.
// The walks: one lane per ray, k_query_fan_binned's walk (../query/rt_query.hip: fan_walk) over two lists in turn -- the ray's
// cell, front to back in depth shells, then the every-ray list.  State in plain registers, every step straight-line code for every
// lane (a lane with no row left loads row 0 and ignores it), only the exact stage in a divergent branch; every test that reaches it
// is k_query_closest's own 41 operations on the caller's start and negD = -dir (ray_dots, maybe_hit, exact_hit_row).
// Built with -ffp-contract=off like every kernel of the library.
#include "along.hpp"
#include "../query/rt_query_device.hpp"

namespace mirt {

// ---- the build ---------------------------------------------------------------------------------------------------------------------

// A pair into the list, counted in the workgroup's histogram of the sort's buckets (LDS).
__device__ __forceinline__ void along_emit(const AlongPairs &b, uint32_t *s_hist, uint32_t at, uint32_t key, uint32_t tri)
{
    if (at < b.cap) {                                              // (a list that overflows is counted to its end and built again)
        b.keys[at] = key;
        b.vals[at] = tri;
        atomicAdd(s_hist + (key >> b.bucket_shift), 1u);
    }
}

// One lane per triangle: along_tri_setup on the scene's row, then the cells of its box, each through along_cell_may_hit -- twice:
// once to count the lane's pairs, so that a wave reserves its slice of the list with ONE atomic on the pair counter (a scan over the
// wave), once to write them.  Both passes run the same text on the same operands, so they agree on every cell.  The pairs per sort
// bucket are counted in LDS and reach bucket_cnt with one atomic per workgroup and non-empty bucket: the sort's few hundred counters
// share a handful of cache lines, which a global atomic per pair would all queue on.
__global__ __launch_bounds__(256) void k_along_pairs(const AlongPairs b)
{
    extern __shared__ uint32_t s_hist[];
    for (uint32_t k = threadIdx.x; k < b.nbuckets; k += 256) s_hist[k] = 0u;
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const bool valid = i < b.n;
    const float4 *src = reinterpret_cast<const float4 *>(b.qrows + (valid ? i : 0));
    const RowVecs r = unpack_row(src[0], src[1], src[2]);
    const AlongTri t = along_tri_setup(b.d, r.v0, r.e1, r.e2, r.e1e2);
    const bool every = t.kind == ALONG_EVERY;
    uint32_t cnt = 0u;
    if (valid) {
        b.near[i] = t.near;
        if (every) {
            atomicAdd(b.counters + 1, 1u);
            cnt = 1u;
        } else {
            for (int cj = t.j0; cj <= t.j1; cj++)
                for (int ci = t.i0; ci <= t.i1; ci++) cnt += along_cell_may_hit(b.d, t, ci, cj) ? 1u : 0u;
        }
    }
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    const uint32_t total = __shfl(incl, 63);
    uint32_t base = 0u;
    if (lane == 0 && total) base = atomicAdd(b.counters, total);
    uint32_t at = __shfl(base, 0) + incl - cnt;
    const uint32_t shells = (uint32_t)b.d.shells;
    if (valid && every) along_emit(b, s_hist, at, (uint32_t)(b.d.B * b.d.B) * shells, (uint32_t)i);
    if (valid && !every) {
        const uint32_t shell = bin_shell_of(t.near, b.d.shell_d0, b.d.shell_iw, b.d.shells);
        for (int cj = t.j0; cj <= t.j1; cj++)
            for (int ci = t.i0; ci <= t.i1; ci++)
                if (along_cell_may_hit(b.d, t, ci, cj)) along_emit(b, s_hist, at++, (uint32_t)(cj * b.d.B + ci) * shells + shell, (uint32_t)i);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < b.nbuckets; k += 256)
        if (s_hist[k]) atomicAdd(b.bucket_cnt + k, s_hist[k]);
}

// Row e of the structure: the scene's row of the e-th triangle in key order, its index and depth bound beside it.
__global__ __launch_bounds__(256) void k_along_rows(const AlongRows x)
{
    const uint32_t total = *x.total;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const uint32_t tri = x.entries[e];
        const float4 *src = reinterpret_cast<const float4 *>(x.qrows + tri);
        float4 *dst = reinterpret_cast<float4 *>(x.rows + e);
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
        AlongAux a;
        a.tri = tri; a.near = x.near[tri];
        x.aux[e] = a;
    }
}

// The rays of a call written out for k_query_closest* / k_query_occluded* (BRUTE, and every call the structure is not built for).
__global__ __launch_bounds__(256) void k_along_expand(const AlongExpand x)
{
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    if (ray >= x.nrays) return;
    float *r = x.rays + (size_t)RAY_WORDS * ray;
    st3(r, ld3(x.origins + 3 * (size_t)ray));
    st3(r + 3, V3(x.dir[0], x.dir[1], x.dir[2]));
}

// ---- the walks ---------------------------------------------------------------------------------------------------------------------
//
// A lane's ray: start S, the call's negD, its depth rs = S . dhat and the two lists it walks.  `binned`: the start is finite, within
// smax and inside the filter's range (ray_exact_only false: the scene's rows and a start below 1e8; dir's window keeps negD inside
// it) -- the margins of along_tri_setup hold for exactly these; its cell list is empty when the projection falls outside the grid.
// Any other live lane sweeps all n rows of the scene in index order after the wave's walk, with k_query_closest's loop body.
struct AlongLane {
    v3 S;
    float rs;
    bool exact_only, in_reach;
    uint32_t key;                // first key of the lane's cell (valid while has_cell)
    bool has_cell;
};
__device__ __forceinline__ AlongLane along_lane(const AlongFrame &f, bool scene_ok, long long ray, bool ok)
{
    AlongLane l;
    l.S = ld3(f.origins + 3 * (size_t)(ok ? ray : 0));
    l.exact_only = ray_exact_only(scene_ok, l.S, V3(f.dir[0], f.dir[1], f.dir[2]));
    l.in_reach = along_start_in_reach(f.v.d, l.S) && !l.exact_only;
    l.rs = along_depth_of(f.v.d, l.S);
    const int cell = along_cell_of(f.v.d, l.S);
    l.has_cell = l.in_reach && cell >= 0;
    l.key = (uint32_t)(l.has_cell ? cell : 0) * (uint32_t)f.v.d.shells;
    return l;
}
// The last row (exclusive) of the cell's list a ray whose distance bound is `x` walks: the shells up to the one rs + x falls into.  A
// row with near <= rs + x lies in no later shell (bin_shell_of is monotone), every other row fails the bound (along.hpp: Depth).
__device__ __forceinline__ uint32_t along_list_end(const AlongView &v, uint32_t key, float thr)
{
    return v.off[key + bin_shell_of(thr, v.d.shell_d0, v.d.shell_iw, v.d.shells) + 1u];
}
__device__ __forceinline__ void along_row(const AlongView &v, uint32_t e, float4 &c0, float4 &c1, float4 &c2, AlongAux &ax)
{
    walk_row(reinterpret_cast<const float4 *>(v.rows), e, c0, c1, c2);
    ax = v.aux[e];
}

// k_along_closest: the record rule is fan_walk's -- running (bound, best_i), an accepted d replaces them when bound > d, or bound ==
// d and its index is larger; best_i = -1 stands for the incoming record, which so loses every tie; a negative or NaN incoming
// distance takes no list at all.  The cell list's end moves in with every replacement; the every-ray list (stage 1) has no depth
// order and is walked whole.
template <bool STATS>
__global__ __launch_bounds__(256) void k_along_closest(const AlongFrame f)
{
    const AlongView &v = f.v;
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = ray < f.q.nrays;
    const AlongLane l = along_lane(f, scene_rows_in_range(f.q), ray, ok);
    const v3 nd = V3(-f.dir[0], -f.dir[1], -f.dir[2]);            // negD = -dir (:229); dir is used as given
    uint32_t *h = f.q.hits + (size_t)HIT_WORDS * (ok ? ray : 0);
    float bound = __uint_as_float(h[3]);
    const bool open = ok && bound >= 0.0f;                         // (false for NaN)
    const bool binned = open && l.in_reach, swept = open && !l.in_reach;
    const uint32_t every = (uint32_t)(v.d.B * v.d.B) * (uint32_t)v.d.shells;
    uint32_t e = 0u, end = 0u, e2 = 0u, end2 = 0u;
    if (binned) { e2 = v.off[every]; end2 = v.off[every + 1u]; }
    if (binned && l.has_cell) { e = v.off[l.key]; end = along_list_end(v, l.key, l.rs + bound); }
    int stage = 0;
    if (!(e < end)) { e = e2; end = end2; stage = 1; }
    unsigned long long n_cand = 0, n_tests = 0;
    int best_i = -1, replaced = 0;
    v3 pos = V3(0.0f, 0.0f, 0.0f);
    float4 c0, c1, c2;
    AlongAux ax;
    along_row(v, e < end ? e : 0u, c0, c1, c2, ax);
    for (;;) {
        const int act = (int)(e < end);
        if (!__any(act)) break;
        const RowVecs r = unpack_row(c0, c1, c2);
        float e1e2b;
        const TestDots td = ray_dots(r, l.S, nd, &e1e2b);
        const int near_ok = act & (int)!(ax.near > l.rs + bound);  // strictly beyond the record: cannot pass `bound >= d`
        if (STATS) { n_cand += (unsigned)act; n_tests += (unsigned)near_ok; }
        if (near_ok & (int)maybe_hit(td)) {
            const int tri = (int)ax.tri;
            v3 hp;
            float dist;
            if (exact_hit_row(td, e1e2b, r, l.S, &hp, &dist)) {
                if ((bound > dist) | ((bound == dist) & (tri > best_i))) {
                    bound = dist; best_i = tri; pos = hp; replaced = 1;
                    if (stage == 0) end = min(end, along_list_end(v, l.key, l.rs + dist));
                }
            }
        }
        // on to the next row of the list, else to the every-ray list, else the lane is through
        const int cont = act & (int)(e + 1u < end);
        const int turn = (cont ^ 1) & (int)(stage == 0);
        e = cont ? e + 1u : (turn ? e2 : end);
        end = turn ? end2 : end;
        stage |= turn;
        along_row(v, e < end ? e : 0u, c0, c1, c2, ax);
    }
    if (__any(swept)) {
        // (rare) the lanes the structure does not cover: every row of the scene in index order, the sequential rule itself
        if (STATS && swept) { n_cand += (unsigned)f.q.n; n_tests += (unsigned)f.q.n; }
        for (int j = 0; j < f.q.n; j++) {
            const float4 *src = reinterpret_cast<const float4 *>(f.q.rows + j);
            const RowVecs r = unpack_row(src[0], src[1], src[2]);
            float e1e2b;
            const TestDots td = ray_dots(r, l.S, nd, &e1e2b);
            if (swept && (maybe_hit(td) || l.exact_only)) {
                v3 hp;
                float dist;
                if (exact_hit_row(td, e1e2b, r, l.S, &hp, &dist)) closest_offer(bound, best_i, pos, replaced, dist, j, hp);
            }
        }
    }
    if (ok && replaced) store_record(h, pos, __float_as_uint(bound), (uint32_t)best_i);
    if (STATS) flush_query_stats(f.stats, ok ? 1u : 0u, n_cand, n_tests, swept ? 1u : 0u);
}

template __global__ void k_along_closest<false>(const AlongFrame);
template __global__ void k_along_closest<true>(const AlongFrame);

// k_along_occluded: k_query_occluded_fans_binned's argument with the record distance fixed at the limit L.  A row with d < L has near
// <= rs + d <= rs + L: it lies in a shell no later than L's and passes `!(near > rs + L)`, so the cell list ends at L's shell, that end
// never moves, and the lane is through at its first accepted dist < L.  No list for a limit that is NaN, 0 or negative.  Every byte
// of the call is written.
template <bool STATS>
__global__ __launch_bounds__(256) void k_along_occluded(const AlongFrame f)
{
    const AlongView &v = f.v;
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = ray < f.q.nrays;
    const AlongLane l = along_lane(f, scene_rows_in_range(f.q), ray, ok);
    const v3 nd = V3(-f.dir[0], -f.dir[1], -f.dir[2]);            // negD = -dir (:229); dir is used as given
    const float L = occlusion_limit(f.limit, ray, ok);
    const bool open = ok && L > 0.0f;                              // (false for NaN)
    const bool binned = open && l.in_reach, swept = open && !l.in_reach;
    const float thr = l.rs + L;
    const uint32_t every = (uint32_t)(v.d.B * v.d.B) * (uint32_t)v.d.shells;
    uint32_t e = 0u, end = 0u, e2 = 0u, end2 = 0u;
    if (binned) { e2 = v.off[every]; end2 = v.off[every + 1u]; }
    if (binned && l.has_cell) { e = v.off[l.key]; end = along_list_end(v, l.key, thr); }
    int stage = 0;
    if (!(e < end)) { e = e2; end = end2; stage = 1; }
    unsigned long long n_cand = 0, n_tests = 0;
    int occluded = 0;
    float4 c0, c1, c2;
    AlongAux ax;
    along_row(v, e < end ? e : 0u, c0, c1, c2, ax);
    for (;;) {
        const int act = (int)(e < end);
        if (!__any(act)) break;
        const RowVecs r = unpack_row(c0, c1, c2);
        float e1e2b;
        const TestDots td = ray_dots(r, l.S, nd, &e1e2b);
        const int near_ok = act & (int)!(ax.near > thr);           // every point of the row is beyond the limit: cannot pass `<`
        if (STATS) { n_cand += (unsigned)act; n_tests += (unsigned)near_ok; }
        int done = 0;
        if (near_ok & (int)maybe_hit(td)) {
            v3 hp;
            float dist;
            if (exact_hit_row(td, e1e2b, r, l.S, &hp, &dist)) done = (int)(dist < L);      // :313
        }
        occluded |= done;
        const int cont = act & (done ^ 1) & (int)(e + 1u < end);
        const int turn = (cont ^ 1) & (done ^ 1) & (int)(stage == 0);
        e = cont ? e + 1u : (turn ? e2 : end);
        end = turn ? end2 : end;
        stage |= turn;
        along_row(v, e < end ? e : 0u, c0, c1, c2, ax);
    }
    if (__any(swept)) {
        // the lanes the structure does not cover: every row of the scene, up to the first occluder
        bool live = swept;
        unsigned rows = 0u;
        for (int j = 0; j < f.q.n; j++) {
            if (!__any(live)) break;
            const float4 *src = reinterpret_cast<const float4 *>(f.q.rows + j);
            const RowVecs r = unpack_row(src[0], src[1], src[2]);
            float e1e2b;
            const TestDots td = ray_dots(r, l.S, nd, &e1e2b);
            rows += live ? 1u : 0u;
            if (live && (maybe_hit(td) || l.exact_only)) {
                v3 hp;
                float dist;
                if (exact_hit_row(td, e1e2b, r, l.S, &hp, &dist))
                    if (dist < L) live = false;                    // :313
            }
        }
        occluded |= (int)(swept && !live);
        if (STATS) { n_cand += rows; n_tests += rows; }
    }
    if (ok) f.occluded[ray] = (uint8_t)occluded;
    if (STATS) flush_query_stats(f.stats, ok ? 1u : 0u, n_cand, n_tests, swept ? 1u : 0u);
}

template __global__ void k_along_occluded<false>(const AlongFrame);
template __global__ void k_along_occluded<true>(const AlongFrame);

}  // namespace mirt
