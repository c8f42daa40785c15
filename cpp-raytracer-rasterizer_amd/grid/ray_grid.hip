// ray_grid.hip -- hand-written gfx950 kernels of the arbitrary-ray grid (mirt_set_ray_grid; ray_grid.hpp has the structure, the filing
// predicate and the walk, DESIGN.md section 5.1 the argument).
//
// The build (once per scene version): k_grid_pairs files every triangle -- a key per cell its grown box touches and per plane-index
// bin of its neighbourhood, or the one key of the every-ray list --, bucket_sort_pairs (../csrc/bin_sort.hpp) orders the pairs,
// k_grid_rows writes the 48-byte QueryRow of each pair in key order with the triangle's index alongside.
// The walks: one lane per ray.  A lane takes one grid_walk_step whenever its run of rows is used up (state in plain registers, double
// arithmetic, no LDS), then every lane with a row tests it; every step of the loop is straight-line code for every lane (a lane with no row left
// loads row 0 and ignores it), only the exact stage in a divergent branch; every test that reaches it is k_query_closest's own 41
// operations on the caller's start and negD = -dir (ray_dots, maybe_hit, exact_hit_row).
// Built with -ffp-contract=off like every kernel of the library.
#include "ray_grid.hpp"
#include "ray_grid_device.hpp"
#include "../query/rt_query_device.hpp"

namespace mirt {

// ---- the build ---------------------------------------------------------------------------------------------------------------------

// A pair into the list, counted in the workgroup's histogram of the sort's buckets (LDS).
__device__ __forceinline__ void grid_emit(const GridPairs &b, uint32_t *s_hist, uint32_t at, uint32_t key, uint32_t val)
{
    if (at < b.cap) {                                              // (a list that overflows is counted to its end and built again)
        b.keys[at] = key;
        b.vals[at] = val;
        atomicAdd(s_hist + (key >> b.bucket_shift), 1u);
    }
}

// One lane per triangle of a workgroup of 256: grid_tri_setup on the scene's row, the lane's pair count (its cells counted by the
// enumeration that writes them), ONE
// atomic per wave on the pair counter (a scan over the wave), then grid_tri_keys writes the pairs.  The pairs per sort bucket are
// counted in LDS and reach bucket_cnt with one atomic per workgroup and non-empty bucket (along_file.hpp: the same scheme).
__global__ __launch_bounds__(256) void k_grid_pairs(const GridPairs b)
{
    extern __shared__ uint32_t s_hist[];
    for (uint32_t k = threadIdx.x; k < b.nbuckets; k += 256) s_hist[k] = 0u;
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const bool valid = i < b.n;
    const float4 *src = reinterpret_cast<const float4 *>(b.qrows + (valid ? i : 0));
    const RowVecs r = unpack_row(src[0], src[1], src[2]);
    const GridTri t = grid_tri_setup(b.d, r.v0, r.e1, r.e2, r.e1e2);
    const bool every = t.kind == GRID_EVERY;
    const uint32_t nplane = valid && !every ? grid_tri_plane_keys(t) : 0u;
    const uint32_t cnt = !valid ? 0u : (every ? 1u : grid_tri_cell_keys(b.d, t) + nplane);
    if (valid && every) atomicAdd(b.counters + 1, 1u);
    if (nplane) atomicAdd(b.counters + 2, nplane);
    uint32_t incl = cnt;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t up = __shfl_up(incl, s);
        if (lane >= s) incl += up;
    }
    const uint32_t total = __shfl(incl, 63);
    uint32_t base = 0u;
    if (lane == 0 && total) {
        base = atomicAdd(b.counters, total);
        // (the same sum in 64 bits: should the 32-bit counter ever wrap, the host sees it and the build gives up)
        atomicAdd(reinterpret_cast<unsigned long long *>(b.counters + 4), (unsigned long long)total);
    }
    uint32_t at = __shfl(base, 0) + incl - cnt;
    if (valid) grid_tri_keys(b.d, t, [&](uint32_t key) { grid_emit(b, s_hist, at++, key, (uint32_t)i); });
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < b.nbuckets; k += 256)
        if (s_hist[k]) atomicAdd(b.bucket_cnt + k, s_hist[k]);
}

// Row e of the structure: the scene's row of the e-th triangle in key order (its index stays in `entries`).
__global__ __launch_bounds__(256) void k_grid_rows(const GridRows x)
{
    const uint32_t total = *x.total;
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < total; e += gridDim.x * 256u) {
        const float4 *src = reinterpret_cast<const float4 *>(x.qrows + x.entries[e]);
        float4 *dst = reinterpret_cast<float4 *>(x.rows + e);
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    }
}

// ---- the walks ---------------------------------------------------------------------------------------------------------------------

// Closest hits.  The record rule is fan_walk's: running (bound, best_i), an accepted d replaces them when bound > d, or bound == d
// and its index is larger; best_i = -1 stands for the incoming record, which so loses every tie; a negative or NaN incoming distance
// takes no list at all.  A row offered twice (a triangle filed in several cells of the ray) changes nothing the second time.
template <bool STATS>
__global__ __launch_bounds__(256) void k_grid_closest(const GridFrame f)
{
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool mine = ray < f.q.nrays;
    const GridLane l = grid_lane(f, ray, mine);
    uint32_t *h = f.q.hits + (size_t)HIT_WORDS * (mine ? ray : 0);
    float bound = __uint_as_float(h[3]);
    const bool open = mine && bound >= 0.0f;                       // (false for NaN)
    const bool swept = open && !l.fit;
    bool live = open && l.fit;
    GridWalk w = grid_walk_begin(f.v.d, l.S, V3(-l.nd.x, -l.nd.y, -l.nd.z), live);
    uint32_t e = 0u, end = 0u;
    int src = 0, best_i = -1, replaced = 0;
    unsigned long long c[GSTAT_WORDS] = {};
    v3 pos = V3(0.0f, 0.0f, 0.0f);
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
        const TestDots td = ray_dots(r, l.S, l.nd, &e1e2b);
        if (STATS) {
            c[GSTAT_ROWS_CELLS] += (unsigned)(act & (int)(src == 0));
            c[GSTAT_ROWS_PLANES] += (unsigned)(act & (int)(src == 1));
            c[GSTAT_ROWS_EVERY] += (unsigned)(act & (int)(src == 2));
            c[GSTAT_TESTS] += (unsigned)act;
        }
        if (act & (int)maybe_hit(td)) {
            v3 hp;
            float dist;
            if (exact_hit_row(td, e1e2b, r, l.S, &hp, &dist)) {
                if ((bound > dist) | ((bound == dist) & (tri > best_i))) { bound = dist; best_i = tri; pos = hp; replaced = 1; }
            }
        }
        e += (uint32_t)act;
    }
    if (__any(swept)) {
        // (rare) the lanes the structure does not cover: every row of the scene in index order, the sequential rule itself
        if (STATS && swept) { c[GSTAT_TESTS] += (unsigned)f.q.n; c[GSTAT_SWEPT] = 1; }
        for (int j = 0; j < f.q.n; j++) {
            const float4 *src4 = reinterpret_cast<const float4 *>(f.q.rows + j);
            const RowVecs r = unpack_row(src4[0], src4[1], src4[2]);
            float e1e2b;
            const TestDots td = ray_dots(r, l.S, l.nd, &e1e2b);
            if (swept && (maybe_hit(td) || l.exact_only)) {
                v3 hp;
                float dist;
                if (exact_hit_row(td, e1e2b, r, l.S, &hp, &dist)) closest_offer(bound, best_i, pos, replaced, dist, j, hp);
            }
        }
    }
    if (mine && replaced) store_record(h, pos, __float_as_uint(bound), (uint32_t)best_i);
    if (STATS) { c[GSTAT_RAYS] = mine ? 1u : 0u; flush_grid_stats(f.stats, c); }
}

template __global__ void k_grid_closest<false>(const GridFrame);
template __global__ void k_grid_closest<true>(const GridFrame);

// Occlusion: the same walk with the record distance fixed at the limit L; the lane is through at its first accepted dist < L (:313).
// No list for a limit that is NaN, 0 or negative.  Every byte of the call is written.
template <bool STATS>
__global__ __launch_bounds__(256) void k_grid_occluded(const GridFrame f)
{
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool mine = ray < f.q.nrays;
    const GridLane l = grid_lane(f, ray, mine);
    const float L = occlusion_limit(f.limit, ray, mine);
    const bool open = mine && L > 0.0f;                            // (false for NaN)
    const bool swept = open && !l.fit;
    bool live = open && l.fit;
    GridWalk w = grid_walk_begin(f.v.d, l.S, V3(-l.nd.x, -l.nd.y, -l.nd.z), live);
    const double reach = (double)L * (1.0 + 9.5367431640625e-7);
    uint32_t e = 0u, end = 0u;
    int src = 0, occluded = 0;
    unsigned long long c[GSTAT_WORDS] = {};
    const float4 *rows4 = reinterpret_cast<const float4 *>(f.v.rows);
    for (;;) {
        grid_step_rows(f.v, w, reach, live, e, end, src);
        if (!__any(live)) break;
        const int act = (int)(live && e < end);
        if (!__any(act)) continue;                                 // (a round of steps only)
        float4 c0, c1, c2;
        walk_row(rows4, act ? e : 0u, c0, c1, c2);
        const RowVecs r = unpack_row(c0, c1, c2);
        float e1e2b;
        const TestDots td = ray_dots(r, l.S, l.nd, &e1e2b);
        if (STATS) {
            c[GSTAT_ROWS_CELLS] += (unsigned)(act & (int)(src == 0));
            c[GSTAT_ROWS_PLANES] += (unsigned)(act & (int)(src == 1));
            c[GSTAT_ROWS_EVERY] += (unsigned)(act & (int)(src == 2));
            c[GSTAT_TESTS] += (unsigned)act;
        }
        if (act & (int)maybe_hit(td)) {
            v3 hp;
            float dist;
            if (exact_hit_row(td, e1e2b, r, l.S, &hp, &dist))
                if (dist < L) { occluded = 1; live = false; }      // :313
        }
        e += (uint32_t)act;
    }
    if (__any(swept)) {
        // the lanes the structure does not cover: every row of the scene, up to the first occluder
        bool go = swept;
        unsigned rows = 0u;
        for (int j = 0; j < f.q.n; j++) {
            if (!__any(go)) break;
            const float4 *src4 = reinterpret_cast<const float4 *>(f.q.rows + j);
            const RowVecs r = unpack_row(src4[0], src4[1], src4[2]);
            float e1e2b;
            const TestDots td = ray_dots(r, l.S, l.nd, &e1e2b);
            rows += go ? 1u : 0u;
            if (go && (maybe_hit(td) || l.exact_only)) {
                v3 hp;
                float dist;
                if (exact_hit_row(td, e1e2b, r, l.S, &hp, &dist))
                    if (dist < L) go = false;                      // :313
            }
        }
        occluded |= (int)(swept && !go);
        if (STATS) { c[GSTAT_TESTS] += rows; c[GSTAT_SWEPT] = swept ? 1u : 0u; }
    }
    if (mine) f.occluded[ray] = (uint8_t)occluded;
    if (STATS) { c[GSTAT_RAYS] = mine ? 1u : 0u; flush_grid_stats(f.stats, c); }
}

template __global__ void k_grid_occluded<false>(const GridFrame);
template __global__ void k_grid_occluded<true>(const GridFrame);

}  // namespace mirt
