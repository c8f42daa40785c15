// count_hits.hip -- hand-written gfx950 kernels of mirt_count_hits*: the number of triangles along each ray that ClosestIntersection
// accepts, a fresh record would take, that come behind an optional `after` record and lie strictly below an optional limit
// (count_rule.hpp) -- one integer a ray, no list and no order.
//
// Every (ray, triangle) test is k_query_closest's own (count_device.hpp).  A sweep offers every row of the scene once, in index order
// per lane, so the count is exact; nothing ends a ray early, so there is no vote.  The two sweeps differ in who owns a ray:
//   k_count_wave       a wave per ray (k_query_closest_wave's shape): the 64 lanes stride over the rows in global memory, each keeps
//                      an integer of its own, one wave reduction sums them and lane 0 stores the result;
//   k_count_lanes<P>   a lane per P rays (k_query_closest's shape and ray numbering): the rows staged through LDS in chunks of
//                      RT_CHUNK_ROWS and read as wave-uniform broadcasts, shared by the lane's P rays.
// A ray nothing can count for -- a NaN `after` distance, a limit that is NaN, 0 or negative -- reads no row and gets 0.
// The walks through the grids across a direction: count_along.hip.
// Built with -ffp-contract=off like every kernel of the library.
#include "count_device.hpp"

namespace mirt {

// ---- k_count_wave: one WAVE per ray, lanes over triangles ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_count_wave(const CountFrame c)
{
    const QueryFrame &q = c.q;
    const int lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= q.nrays) return;                                    // (the whole wave)
    const float *rp = q.rays + (size_t)RAY_WORDS * ray;
    const v3 start = ld3(rp), dir = ld3(rp + 3);
    const v3 nd = neg3(dir);                                       // negD = -dir (:229); dir is used as given
    const bool exact_only = ray_exact_only(scene_rows_in_range(q), start, dir);
    const CountRay cr = count_ray_of(c.out, ray, true);

    int cnt = 0;
    if (cr.open) {                                                 // (wave-uniform)
        for (int i = lane; i < q.n; i += 64) {
            const float4 *src = reinterpret_cast<const float4 *>(q.rows + i);
            cnt += count_row(cr, unpack_row(src[0], src[1], src[2]), i, start, nd, true, exact_only);
        }
    }
    cnt = wave_sum32(cnt);
    if (lane == 0) c.out.counts[ray] = cnt;
}

// ---- k_count_lanes: one lane per P rays, every ray tests every triangle ------------------------------------------------------------
// Lane t of block b owns rays (b * P + p) * 256 + t; a lane without a ray reads ray 0, is not open and stores nothing.
template <int P>
__global__ __launch_bounds__(256) void k_count_lanes(const CountFrame c)
{
    extern __shared__ __attribute__((aligned(16))) float4 s_rows[];
    const QueryFrame &q = c.q;
    const bool scene_ok = scene_rows_in_range(q);

    long long ray[P];
    bool ok[P], exact_only[P];
    v3 start[P], nd[P];
    CountRay cr[P];
    int cnt[P];
#pragma unroll
    for (int p = 0; p < P; p++) {
        ray[p] = ((long long)blockIdx.x * P + p) * 256 + threadIdx.x;
        ok[p] = ray[p] < q.nrays;
        const float *rp = q.rays + (size_t)RAY_WORDS * (ok[p] ? ray[p] : 0);
        start[p] = ld3(rp);
        const v3 dir = ld3(rp + 3);
        nd[p] = neg3(dir);                                         // :229
        exact_only[p] = ray_exact_only(scene_ok, start[p], dir);
        cr[p] = count_ray_of(c.out, ray[p], ok[p]);
        cnt[p] = 0;
    }

    for (int base = 0; base < q.n; base += RT_CHUNK_ROWS) {
        const int n = min(RT_CHUNK_ROWS, q.n - base);
        stage_rows(s_rows, q.rows + base, n);
#pragma unroll 2
        for (int j = 0; j < n; j++) {
            const RowVecs r = unpack_row(s_rows[3 * j], s_rows[3 * j + 1], s_rows[3 * j + 2]);
#pragma unroll
            for (int p = 0; p < P; p++) cnt[p] += count_row(cr[p], r, base + j, start[p], nd[p], cr[p].open, exact_only[p]);
        }
    }

#pragma unroll
    for (int p = 0; p < P; p++)
        if (ok[p]) c.out.counts[ray[p]] = cnt[p];
}

template __global__ void k_count_lanes<COUNT_P>(const CountFrame);

}  // namespace mirt
