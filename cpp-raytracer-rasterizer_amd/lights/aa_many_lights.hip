// aa_many_lights.hip -- hand-written gfx950 kernels of a supersampled frame that shades each carried record once
// (aa_many_lights.hpp; aa_versions.hpp has the argument and the per-pixel state machine both kernels run).
//
// k_aa_primary: one lane per pixel of a chunk of rows, all aa x aa sub-rays of Draw() (raytracer/Source/raytracer.cpp:557-602) in
// the lane.  Every sub-ray is one ClosestIntersection call from a FRESH record, whose result is merged into the record the pixel
// carries in registers (aa_merge); where that begins a new version of the carried record, the record is appended to a compact
// list -- one integer atomic add per wave and append event, the lanes' places by ballot and rank -- and the pixel notes the slot;
// how often each version is shaded is counted in the lane and stored when the version ends.  Which slot a record lands in differs
// from run to run; nothing reads the list except by slot.  Two instantiations:
//   sweep  -- every sub-ray tests every row of the camera's origin table (k_prep_origin), staged through LDS in chunks and read
//             as wave-uniform broadcasts: k_query_fan's loop body, the filter in front of exact_hit with the per-ray override;
//   binned -- every sub-ray walks its bin of the cube around the camera front to back from a bound of FLT_MAX, the list's end
//             moving in with every replacement: k_query_fan_binned's walk (../query/rt_query.hip: fan_walk) on a fresh record.  A
//             direction fan_dir_of does not form sweeps the cube's own origin table in index order.
// k_aa_resolve: one lane per pixel, the pixel's (slot, count) pairs in order: colour * (DirectLight[slot] + indirectLight) added
// `count` times, one addition at a time, divided by aa * aa, stored as k_frame_resolve stores (many_lights.hip).
//
// A sub-ray that is accepted while the carried index is still -1 takes distances that are not finite; the reference then reads
// triangles[-1].  Here such a version is the reset record: DirectLight answers index -1 with zeros, and the resolve takes triangle
// 0's colour for it, so nothing is read out of bounds.
// Built with -ffp-contract=off like every kernel of the library.
#include "aa_many_lights.hpp"
#include "../query/rt_query_device.hpp"

#include <float.h>

namespace mirt {

// Chunk pixel of lane t of block b, whether there is one, and its place in the frame.
struct AaLane { long long i, pixels; bool ok; int x, y; };
__device__ __forceinline__ AaLane aa_lane(const AaFrame &a)
{
    AaLane l;
    l.pixels = (long long)a.W * (a.y1 - a.y0);
    l.i = (long long)blockIdx.x * 256 + threadIdx.x;
    l.ok = l.i < l.pixels;
    const long long j = l.ok ? l.i : 0;
    l.x = (int)(j % a.W);
    l.y = a.y0 + (int)(j / a.W);
    return l;
}

// One sub-ray's ClosestIntersection from a fresh record by the sweep: k_query_fan's loop body for one ray.  Every lane of the
// workgroup takes part in the staging barriers.
template <bool FILTER>
__device__ __forceinline__ bool aa_closest_sweep(const AaFrame &a, float4 *s_tab, v3 S, v3 dir, AaRecord &fresh)
{
    RayDirs<1> rd;
    rd.set(0, neg3(dir));                                          // negD = -dir (:229)
    const bool exact_only = !dir_in_filter_range(dir);
    bool accepted = false, replaced = false;
    for (int base = 0; base < a.n; base += RT_CHUNK_ROWS) {
        const int cnt = min(RT_CHUNK_ROWS, a.n - base);
        stage_rows(s_tab, a.tab + base, cnt);
#pragma unroll 2
        for (int j = 0; j < cnt; j++) {
            const float4 r0 = s_tab[3 * j], r1 = s_tab[3 * j + 1], r2 = s_tab[3 * j + 2];
            TestDots d[1];
            bool maybe[1];
            test_rays<1, FILTER>(r0, r1, r2, rd, d, maybe);
            if (maybe[0] || exact_only) {
                v3 hp;
                float dist;
                if (exact_hit(d[0], r0.w, a.tris15 + (size_t)15 * (base + j), S, &hp, &dist)) {
                    accepted = true;                               // ClosestIntersection's return value (:251)
                    closest_offer(fresh.dist, fresh.index, fresh.pos, replaced, dist, base + j, hp);
                }
            }
        }
    }
    return accepted;
}

// The same through the camera's cube: fan_walk's loop on a fresh record (position 0 of a one-position cube).  `live`: the lane
// has a pixel; a lane without one takes no list and sweeps nothing.
__device__ __forceinline__ bool aa_closest_binned(const AaFrame &a, v3 S, v3 dir, bool live, AaRecord &fresh)
{
    const CubeView &cv = a.cube;
    const float4 *rows4 = reinterpret_cast<const float4 *>(cv.light_rows);
    const v3 nd = neg3(dir);                                       // negD = -dir (:229)
    float bound = fresh.dist;                                      // FLT_MAX
    const FanDir fd = fan_dir_of(nd);
    const bool binned = live && fd.formed, swept = live && !fd.formed;
    const BinFrameDesc *lf = cv.light_frames;
    const float d0 = lf->shell_d0, iw = lf->shell_iw;
    uint32_t e = 0u, end = 0u, key = 0u;
    if (binned) key = fan_list(cv, 0u, 0u, fd.d, bound, &e, &end);
    int best_i = -1, replaced = 0, accepted = 0;
    v3 pos = V3(0.0f, 0.0f, 0.0f);
    float4 c0, c1, c2;
    walk_row(rows4, e < end ? e : 0u, c0, c1, c2);
    for (;;) {
        const int act = (int)(e < end);
        if (!__any(act)) break;
        const TestDots td = test_dots(c0, c1, c2, nd);
        const int near_ok = act & (int)!(c1.w > bound);            // strictly beyond the record: cannot pass `bound >= d`
        if (near_ok & (int)maybe_hit(td)) {
            const int tri = (int)cv.light_tri[e];
            v3 hp;
            float dist;
            if (exact_hit(td, c0.w, a.tris15 + (size_t)15 * tri, S, &hp, &dist)) {
                accepted = 1;                                      // (every distance is finite here: accepted and replaced coincide)
                if ((bound > dist) | ((bound == dist) & (tri > best_i))) {
                    bound = dist; best_i = tri; pos = hp; replaced = 1;
                    end = min(end, cv.light_off[key + bin_shell_of(dist, d0, iw, cv.shells) + 1u]);
                }
            }
        }
        walk_step(rows4, e, end, act & (int)(e + 1u < end), c0, c1, c2);   // (the list's end, old or new: the lane is through)
    }
    if (__any(swept)) {
        // (rare) the lanes the bins do not cover: the camera's full table in index order, the sequential rule itself
        const bool exact_only = !dir_in_filter_range(dir);
        for (int j = 0; j < a.n; j++) {
            const float4 r0 = a.tab[j].r0, r1 = a.tab[j].r1, r2 = a.tab[j].r2;
            const TestDots td = test_dots(r0, r1, r2, nd);
            if (swept && (maybe_hit(td) || exact_only)) {
                v3 hp;
                float dist;
                if (exact_hit(td, r0.w, a.tris15 + (size_t)15 * j, S, &hp, &dist)) {
                    accepted = 1;
                    closest_offer(bound, best_i, pos, replaced, dist, j, hp);
                }
            }
        }
    }
    if (replaced) { fresh.dist = bound; fresh.index = best_i; fresh.pos = pos; }
    return accepted != 0;
}

template <bool BINNED, bool FILTER>
__device__ __forceinline__ void aa_primary_body(const AaFrame &a, float4 *s_tab)
{
    const AaLane l = aa_lane(a);
    const int lane = threadIdx.x & 63;
    const v3 cam = ld3(a.cam);
    const float halfW = (float)a.W / 2.0f, halfH = (float)a.H / 2.0f;
    const int rs = a.aa;                                           // realSamples (:549-554), > 1
    const size_t px = (size_t)l.pixels, i = (size_t)(l.ok ? l.i : 0);

    AaRecord carried = aa_record_reset();                          // Update()'s reset (:335-339), once per frame
    AaRuns runs = aa_runs_reset();
    unsigned hits = 0u;

    float y1 = aa_sub_start(l.y, rs);                              // :566-569
    for (int z = 0; z < rs; z++) {
        float x1 = aa_sub_start(l.x, rs);                          // :573-576
        for (int z2 = 0; z2 < rs; z2++) {
            // d = (x1 - W/2, y1 - H/2, focalLength); dir = cameraRot * d (:579-580)
            const v3 dir = mat3_mul_vec(a.rot, V3(x1 - halfW, y1 - halfH, a.focal));
            AaRecord fresh = aa_record_reset();
            bool accepted;
            if constexpr (BINNED) accepted = aa_closest_binned(a, cam, dir, l.ok, fresh);
            else accepted = aa_closest_sweep<FILTER>(a, s_tab, cam, dir, fresh);
            accepted = accepted && l.ok;
            const bool replaced = aa_merge(carried, accepted, fresh);
            const int ended = runs.count;                          // (of the version a new one ends)
            const int ev = aa_sub_event(runs, accepted, replaced);
            // the versions this step begins, appended: one atomic for the wave, the lanes' slots by rank
            const bool begin = ev == AA_SUB_BEGIN;
            const unsigned long long m = __ballot(begin);
            if (m) {                                               // (wave-uniform)
                const int leader = __ffsll((long long)m) - 1;
                uint32_t base = 0u;
                if (lane == leader) base = atomicAdd(a.cursor, (uint32_t)__popcll(m));
                base = (uint32_t)__shfl((int)base, leader);
                if (begin) {
                    const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    const size_t v = (size_t)(runs.nver - 1);
                    if (v > 0) a.counts[(v - 1) * px + i] = (uint32_t)ended;
                    store_record(a.records + (size_t)HIT_WORDS * slot, carried.pos, __float_as_uint(carried.dist), (uint32_t)carried.index);
                    a.slots[v * px + i] = slot;
                }
            }
            if (accepted) {
                hits++;
                x1 += aa_sub_step(rs);                             // (:593) only after a hit
            }
        }
        y1 += aa_sub_step(rs);                                     // (:596)
    }

    {   // hit sub-rays: the frame's sharded counters (count_hits' convention) and the frame's own statistics
        const unsigned total = wave_sum(hits);
        if (lane == 0 && total) {
            const unsigned shard = (blockIdx.x + (threadIdx.x >> 6) * 61u) % HIT_SHARDS;
            atomicAdd(a.hit_count + (size_t)shard * HIT_SHARD_STRIDE, (unsigned long long)total);
            atomicAdd(a.stats, (unsigned long long)total);
        }
    }
    if (!l.ok) return;
    if (runs.nver > 0) a.counts[(size_t)(runs.nver - 1) * px + i] = (uint32_t)runs.count;
    a.nver[i] = (uint32_t)runs.nver;
    const size_t fpx = (size_t)l.y * a.W + l.x;
    if (a.index) a.index[fpx] = carried.index;
    if (a.fd) a.fd[fpx] = carried.index >= 0 ? carried.dist - a.focal_plane : 0.0f;   // focalDistances (:248-249)
    if (a.dist) a.dist[fpx] = carried.index >= 0 ? carried.dist : 3.402823466e+38f;
    if (a.pos) st3(a.pos + 3 * fpx, carried.index >= 0 ? carried.pos : V3(0.0f, 0.0f, 0.0f));
}

template <bool BINNED>
__global__ __launch_bounds__(256) void k_aa_primary(const AaFrame a)
{
    if constexpr (BINNED) {
        aa_primary_body<true, true>(a, nullptr);
    } else {
        extern __shared__ __attribute__((aligned(16))) float4 s_tab[];
        if (__builtin_amdgcn_readfirstlane(*a.unsafe) == 0u) aa_primary_body<false, true>(a, s_tab);
        else aa_primary_body<false, false>(a, s_tab);
    }
}

template __global__ void k_aa_primary<false>(const AaFrame);
template __global__ void k_aa_primary<true>(const AaFrame);

__global__ __launch_bounds__(256) void k_aa_resolve(const AaFrame a)
{
    // (behind every k_aa_primary of the chunk on the stream: the chunk's appended records join the frame's total)
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.stats + 1, (unsigned long long)*a.cursor);
    const AaLane l = aa_lane(a);
    if (!l.ok) return;
    const size_t px = (size_t)l.pixels, i = (size_t)l.i;
    const int nver = (int)a.nver[i];
    const v3 N = ld3(a.indirect);
    v3 avg = V3(0.0f, 0.0f, 0.0f);
    for (int k = 0; k < nver; k++) {
        const uint32_t slot = a.slots[(size_t)k * px + i];
        const int count = (int)a.counts[(size_t)k * px + i];
        const int idx = (int)a.records[(size_t)HIT_WORDS * slot + 4];
        const v3 tcol = ld3(a.tris15 + (size_t)15 * (idx >= 0 && idx < a.n ? idx : 0) + 12);    // :587
        avg = aa_resolve_add(avg, tcol, ld3(a.direct + 3 * (size_t)slot), N, count);            // :583-591
    }
    const v3 out = aa_resolve_div(avg, a.aa);                      // :599
    const size_t fpx = (size_t)l.y * a.W + l.x;
    if (a.rgb) st3(a.rgb + 3 * fpx, out);
    // CalculateDOF draws interior pixels only (:618-620); the border keeps its old value
    if (l.x >= 1 && l.x < a.W - 1 && l.y >= 1 && l.y < a.H - 1)
        a.xrgb[(size_t)(l.y - a.row_origin) * a.pitch_words + l.x] = pack_xrgb(out);
}

}  // namespace mirt
