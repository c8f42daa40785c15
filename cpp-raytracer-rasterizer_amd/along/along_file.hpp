// along_file.hpp -- the ONE filing body of the builds of the ray queries along a direction (device code): k_along_pairs (along.hip:
// one direction, its descriptor in the kernel's arguments, keys from 0) and k_alongs_pairs (alongs.hip: a group of directions, the
// workgroup's descriptor read from a device table, keys from the slot's first) run it.  What differs between them is the descriptor,
// the first key, the first pair value and the counter of the direction's every-ray list.
#pragma once

#include "along.hpp"
#include "../query/rt_query_device.hpp"

namespace mirt {

// Where a workgroup's pairs go.
struct AlongFiling {
    uint32_t *pairs;             // the pair counter
    uint32_t *every;             // the counter of the direction's every-ray list
    uint32_t *keys, *vals;
    uint32_t cap;
    uint32_t *bucket_cnt;        // nbuckets counts for bucket_sort_pairs (../csrc/bin_sort.hpp)
    uint32_t nbuckets;
    int bucket_shift;
};

// A pair into the list, counted in the workgroup's histogram of the sort's buckets (LDS).
__device__ __forceinline__ void along_emit(const AlongFiling &o, uint32_t *s_hist, uint32_t at, uint32_t key, uint32_t val)
{
    if (at < o.cap) {                                              // (a list that overflows is counted to its end and built again)
        o.keys[at] = key;
        o.vals[at] = val;
        atomicAdd(s_hist + (key >> o.bucket_shift), 1u);
    }
}

// One lane per triangle of a workgroup of 256 (triangle i = blockIdx.x * 256 + threadIdx.x): along_tri_setup on the scene's row, then
// the cells of its box, each through along_cell_may_hit -- twice: once to count the lane's pairs, so that a wave reserves its slice
// of the list with ONE atomic on the pair counter (a scan over the wave), once to write them.  Both passes run the same text on the
// same operands, so they agree on every cell.  The pairs per sort bucket are counted in LDS (s_hist: nbuckets words) and reach
// bucket_cnt with one atomic per workgroup and non-empty bucket: the sort's few hundred counters share a handful of cache lines,
// which a global atomic per pair would all queue on.  A pair is (key0 + the single grid's key, val0 + i); near[i] gets the
// triangle's depth bound under d.
__device__ __forceinline__ void along_file_triangles(const AlongDesc &d, const AlongFiling &o, uint32_t *s_hist, const QueryRow *qrows, int n,
                                                     uint32_t key0, uint32_t val0, float *near)
{
    for (uint32_t k = threadIdx.x; k < o.nbuckets; k += 256) s_hist[k] = 0u;
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const bool valid = i < n;
    const float4 *src = reinterpret_cast<const float4 *>(qrows + (valid ? i : 0));
    const RowVecs r = unpack_row(src[0], src[1], src[2]);
    const AlongTri t = along_tri_setup(d, r.v0, r.e1, r.e2, r.e1e2);
    const bool every = t.kind == ALONG_EVERY;
    const uint32_t val = val0 + (uint32_t)(valid ? i : 0);
    uint32_t cnt = 0u;
    if (valid) {
        near[i] = t.near;
        if (every) {
            atomicAdd(o.every, 1u);
            cnt = 1u;
        } else {
            for (int cj = t.j0; cj <= t.j1; cj++)
                for (int ci = t.i0; ci <= t.i1; ci++) cnt += along_cell_may_hit(d, t, ci, cj) ? 1u : 0u;
        }
    }
    uint32_t incl = cnt;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t up = __shfl_up(incl, s);
        if (lane >= s) incl += up;
    }
    const uint32_t total = __shfl(incl, 63);
    uint32_t base = 0u;
    if (lane == 0 && total) base = atomicAdd(o.pairs, total);
    uint32_t at = __shfl(base, 0) + incl - cnt;
    const uint32_t shells = (uint32_t)d.shells;
    if (valid && every) along_emit(o, s_hist, at, key0 + (uint32_t)(d.B * d.B) * shells, val);
    if (valid && !every) {
        const uint32_t shell = bin_shell_of(t.near, d.shell_d0, d.shell_iw, d.shells);
        for (int cj = t.j0; cj <= t.j1; cj++)
            for (int ci = t.i0; ci <= t.i1; ci++)
                if (along_cell_may_hit(d, t, ci, cj)) along_emit(o, s_hist, at++, key0 + (uint32_t)(cj * d.B + ci) * shells + shell, val);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < o.nbuckets; k += 256)
        if (s_hist[k]) atomicAdd(o.bucket_cnt + k, s_hist[k]);
}

}  // namespace mirt
