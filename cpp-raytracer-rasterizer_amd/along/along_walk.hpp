// along_walk.hpp -- the ONE walk of the ray queries along a direction (device code): k_along_closest / k_along_occluded (along.hip:
// one direction, its descriptor in the kernel's arguments) and k_alongs_closest / k_alongs_occluded (alongs.hip: a group of
// directions, each lane's descriptor picked by its ray's index out of LDS) run these two bodies.  What differs between the families
// is where a lane's descriptor, the first key of its direction's part of the tables and its direction come from: along_walk_of
// takes the three and leaves what the walk reads of them in the lane's own registers.
//
// The walk: one lane per ray, k_query_fan_binned's walk (../query/rt_query.hip: fan_walk) over two lists in turn -- the ray's
// cell, front to back in depth shells, then the every-ray list.  State in plain registers, every step straight-line code for every
// lane (a lane with no row left loads row 0 and ignores it), only the exact stage in a divergent branch; every test that reaches it
// is k_query_closest's own 41 operations on the caller's start and negD = -dir (ray_dots, maybe_hit, exact_hit_row).
#pragma once

#include "along.hpp"
#include "../query/rt_query_device.hpp"

namespace mirt {

// The tables a walk reads: the offsets of every key, the rows in key order and the triangle and depth bound beside each.
struct AlongTables {
    const uint32_t *off;
    const QueryRow *rows;        // never NULL: a lane with no row left still loads row 0
    const AlongAux *aux;
};

// A lane's ray: start S, negD = -dir (:229; dir is used as given), its depth rs = S . dhat and the two lists it walks.  `in_reach`:
// the start is finite, within smax and inside the filter's range (ray_exact_only false: the scene's rows and a start below 1e8;
// dir's window keeps negD inside it) -- the margins of along_tri_setup hold for exactly these; its cell list is empty when the
// projection falls outside the grid.  Any other live lane sweeps all n rows of the scene in index order after the wave's walk, with
// k_query_closest's loop body.  The keys are absolute: key_base (the first key of the direction's part of the tables) is in them.
struct AlongLane {
    v3 S, nd;
    float rs;
    bool exact_only, in_reach;
    uint32_t key;                // first key of the lane's cell (valid while has_cell)
    bool has_cell;
    uint32_t every;              // the key of the direction's every-ray list
    float shell_d0, shell_iw;    // bin_shell_of's parameters for the direction
    int shells;
};
__device__ __forceinline__ AlongLane along_walk_of(const AlongDesc &d, uint32_t key_base, v3 dir, bool scene_ok, v3 S)
{
    AlongLane l;
    l.S = S;
    l.nd = V3(-dir.x, -dir.y, -dir.z);
    l.exact_only = ray_exact_only(scene_ok, S, dir);
    l.in_reach = along_start_in_reach(d, S) && !l.exact_only;
    l.rs = along_depth_of(d, S);
    const int cell = along_cell_of(d, S);
    l.has_cell = l.in_reach && cell >= 0;
    l.shells = d.shells;
    l.key = key_base + (uint32_t)(l.has_cell ? cell : 0) * (uint32_t)d.shells;
    l.every = key_base + (uint32_t)(d.B * d.B) * (uint32_t)d.shells;
    l.shell_d0 = d.shell_d0;
    l.shell_iw = d.shell_iw;
    return l;
}
// The last row (exclusive) of the cell's list a ray whose distance bound is `x` walks: the shells up to the one rs + x falls into.  A
// row with near <= rs + x lies in no later shell (bin_shell_of is monotone), every other row fails the bound (along.hpp: Depth).
__device__ __forceinline__ uint32_t along_list_end(const AlongTables &t, const AlongLane &l, float thr)
{
    return t.off[l.key + bin_shell_of(thr, l.shell_d0, l.shell_iw, l.shells) + 1u];
}
__device__ __forceinline__ void along_row(const AlongTables &t, uint32_t e, float4 &c0, float4 &c1, float4 &c2, AlongAux &ax)
{
    walk_row(reinterpret_cast<const float4 *>(t.rows), e, c0, c1, c2);
    ax = t.aux[e];
}

// Closest hits.  The record rule is fan_walk's -- running (bound, best_i), an accepted d replaces them when bound > d, or bound == d
// and its index is larger; best_i = -1 stands for the incoming record, which so loses every tie; a negative or NaN incoming distance
// takes no list at all.  The cell list's end moves in with every replacement; the every-ray list (stage 1) has no depth order and
// is walked whole.  `mine`: the lane has a ray of this launch (a ray inside the call, and of this pass's directions): any other lane
// takes no list, sweeps nothing and writes nothing; `ray` must index the call's arrays whenever `mine` is set.
template <bool STATS>
__device__ __forceinline__ void along_closest_walk(const QueryFrame &q, const AlongTables &t, const AlongLane &l, long long ray, bool mine,
                                                   unsigned long long *stats)
{
    uint32_t *h = q.hits + (size_t)HIT_WORDS * (mine ? ray : 0);
    float bound = __uint_as_float(h[3]);
    const bool open = mine && bound >= 0.0f;                       // (false for NaN)
    const bool binned = open && l.in_reach, swept = open && !l.in_reach;
    uint32_t e = 0u, end = 0u, e2 = 0u, end2 = 0u;
    if (binned) { e2 = t.off[l.every]; end2 = t.off[l.every + 1u]; }
    if (binned && l.has_cell) { e = t.off[l.key]; end = along_list_end(t, l, l.rs + bound); }
    int stage = 0;
    if (!(e < end)) { e = e2; end = end2; stage = 1; }
    unsigned long long n_cand = 0, n_tests = 0;
    int best_i = -1, replaced = 0;
    v3 pos = V3(0.0f, 0.0f, 0.0f);
    float4 c0, c1, c2;
    AlongAux ax;
    along_row(t, e < end ? e : 0u, c0, c1, c2, ax);
    for (;;) {
        const int act = (int)(e < end);
        if (!__any(act)) break;
        const RowVecs r = unpack_row(c0, c1, c2);
        float e1e2b;
        const TestDots td = ray_dots(r, l.S, l.nd, &e1e2b);
        const int near_ok = act & (int)!(ax.near > l.rs + bound);  // strictly beyond the record: cannot pass `bound >= d`
        if (STATS) { n_cand += (unsigned)act; n_tests += (unsigned)near_ok; }
        if (near_ok & (int)maybe_hit(td)) {
            const int tri = (int)ax.tri;
            v3 hp;
            float dist;
            if (exact_hit_row(td, e1e2b, r, l.S, &hp, &dist)) {
                if ((bound > dist) | ((bound == dist) & (tri > best_i))) {
                    bound = dist; best_i = tri; pos = hp; replaced = 1;
                    if (stage == 0) end = min(end, along_list_end(t, l, l.rs + dist));
                }
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
        // (rare) the lanes the structure does not cover: every row of the scene in index order, the sequential rule itself
        if (STATS && swept) { n_cand += (unsigned)q.n; n_tests += (unsigned)q.n; }
        for (int j = 0; j < q.n; j++) {
            const float4 *src = reinterpret_cast<const float4 *>(q.rows + j);
            const RowVecs r = unpack_row(src[0], src[1], src[2]);
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
    if (STATS) flush_query_stats(stats, mine ? 1u : 0u, n_cand, n_tests, swept ? 1u : 0u);
}

// Occlusion: k_query_occluded_fans_binned's argument with the record distance fixed at the limit L.  A row with d < L has near <= rs
// + d <= rs + L: it lies in a shell no later than L's and passes `!(near > rs + L)`, so the cell list ends at L's shell, that end never
// moves, and the lane is through at its first accepted dist < L.  No list for a limit that is NaN, 0 or negative.  Every byte of a
// lane that is `mine` is written; `zero`: the lane's byte is written 0 though the ray is not of this launch (alongs.hip: a ray whose
// index names no direction of the call).
template <bool STATS>
__device__ __forceinline__ void along_occluded_walk(const QueryFrame &q, const AlongTables &t, const AlongLane &l, long long ray, bool mine, bool zero,
                                                    const float *limit, uint8_t *out, unsigned long long *stats)
{
    const float L = occlusion_limit(limit, ray, mine);
    const bool open = mine && L > 0.0f;                            // (false for NaN)
    const bool binned = open && l.in_reach, swept = open && !l.in_reach;
    const float thr = l.rs + L;
    uint32_t e = 0u, end = 0u, e2 = 0u, end2 = 0u;
    if (binned) { e2 = t.off[l.every]; end2 = t.off[l.every + 1u]; }
    if (binned && l.has_cell) { e = t.off[l.key]; end = along_list_end(t, l, thr); }
    int stage = 0;
    if (!(e < end)) { e = e2; end = end2; stage = 1; }
    unsigned long long n_cand = 0, n_tests = 0;
    int occluded = 0;
    float4 c0, c1, c2;
    AlongAux ax;
    along_row(t, e < end ? e : 0u, c0, c1, c2, ax);
    for (;;) {
        const int act = (int)(e < end);
        if (!__any(act)) break;
        const RowVecs r = unpack_row(c0, c1, c2);
        float e1e2b;
        const TestDots td = ray_dots(r, l.S, l.nd, &e1e2b);
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
        along_row(t, e < end ? e : 0u, c0, c1, c2, ax);
    }
    if (__any(swept)) {
        // the lanes the structure does not cover: every row of the scene, up to the first occluder
        bool live = swept;
        unsigned rows = 0u;
        for (int j = 0; j < q.n; j++) {
            if (!__any(live)) break;
            const float4 *src = reinterpret_cast<const float4 *>(q.rows + j);
            const RowVecs r = unpack_row(src[0], src[1], src[2]);
            float e1e2b;
            const TestDots td = ray_dots(r, l.S, l.nd, &e1e2b);
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
    if (mine || zero) out[ray] = (uint8_t)occluded;
    if (STATS) flush_query_stats(stats, mine ? 1u : 0u, n_cand, n_tests, swept ? 1u : 0u);
}

}  // namespace mirt
