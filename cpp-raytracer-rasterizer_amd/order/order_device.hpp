// order_device.hpp -- what every kernel of the ordered hits does around its list (device code; ordered_hits.hip, ordered_along.hip and
// ordered_fans.hip): the `after` record a ray continues behind, a row of a sweep offered to the list, a slot of the answer, and a
// lane's whole answer.  A test comes in two kinds -- the scene's row (ray_dots, exact_hit_row) and an origin table's row with tris15
// (test_dots, exact_hit) --, and so do the offer and the retest that gives a winner's position.
#pragma once

#include "hit_list.hpp"
#include "order_out.hpp"
#include "../query/rt_query_device.hpp"

namespace mirt {

// The record (a, k) ray `ray` continues behind: the caller's, or one that admits everything (no `after`: every eligible distance is
// above -1), or for a lane without a ray one that admits nothing (NaN).
__device__ __forceinline__ void order_after(const OrderOut &o, long long ray, bool ok, float *a, int *k)
{
    *a = ok ? -1.0f : __uint_as_float(0x7fc00000u);
    *k = 0;
    if (ok && o.after) {
        const uint32_t *r = o.after + (size_t)HIT_WORDS * ray;
        *a = __uint_as_float(r[3]);
        *k = (int)r[4];
    }
}

__device__ __forceinline__ RowVecs order_row(const QueryRow *rows, int j)
{
    const float4 *src = reinterpret_cast<const float4 *>(rows + j);
    return unpack_row(src[0], src[1], src[2]);
}

// Row `tri` of a sweep offered to the list of a lane that is `on`: k_query_closest's test (the conservative filter with the per-ray
// exact-only override in front of the exact test), an accepted distance considered behind (a, k).
template <int K>
__device__ __forceinline__ void order_offer_row(HitList<K> &l, const RowVecs &r, int tri, v3 S, v3 nd, bool on, bool exact_only, float a, int k)
{
    float e1e2b;
    const TestDots td = ray_dots(r, S, nd, &e1e2b);
    if (on && (maybe_hit(td) || exact_only)) {
        v3 hp;
        float dist;
        if (exact_hit_row(td, e1e2b, r, S, &hp, &dist)) hit_list_consider(l, dist, tri, a, k);
    }
}
// ... and row `tri` of the origin table `tab`: k_query_fan's test.
template <int K>
__device__ __forceinline__ void order_offer_origin_row(HitList<K> &l, const OriginRow *tab, const float *tris15, int tri, v3 S, v3 nd, bool on, bool exact_only,
                                                       float a, int k)
{
    const float4 r0 = tab[tri].r0, r1 = tab[tri].r1, r2 = tab[tri].r2;
    const TestDots td = test_dots(r0, r1, r2, nd);
    if (on && (maybe_hit(td) || exact_only)) {
        v3 hp;
        float dist;
        if (exact_hit(td, r0.w, tris15 + (size_t)15 * tri, S, &hp, &dist)) hit_list_consider(l, dist, tri, a, k);
    }
}

// The swept fallback of a walk kernel, behind the wave's walk: every row of the scene for the lanes that are `swept` (a wave-uniform
// loop; the other lanes offer nothing).
template <int K>
__device__ __forceinline__ void order_sweep_tail(HitList<K> &l, const QueryRow *rows, int n, v3 S, v3 nd, bool swept, bool exact_only, float a, int k)
{
    for (int j = 0; j < n; j++) order_offer_row(l, order_row(rows, j), j, S, nd, swept, exact_only, a, k);
}

// A winner's position: the test the walk ran, run once more on the winner's row -- the same operations on the same operands, no
// fused forms, so the same bits.  Of the scene's row ...
struct SceneRetest {
    const QueryRow *rows;
    v3 S, nd;
    __device__ __forceinline__ v3 operator()(int tri) const
    {
        const RowVecs r = order_row(rows, tri);
        float e1e2b, dist;
        const TestDots td = ray_dots(r, S, nd, &e1e2b);
        v3 hp = V3(0.0f, 0.0f, 0.0f);
        (void)exact_hit_row(td, e1e2b, r, S, &hp, &dist);
        return hp;
    }
};
// ... and of the origin table's row and tris15.
struct OriginRetest {
    const OriginRow *tab;
    const float *tris15;
    v3 S, nd;
    __device__ __forceinline__ v3 operator()(int tri) const
    {
        const float4 r0 = tab[tri].r0, r1 = tab[tri].r1, r2 = tab[tri].r2;
        const TestDots td = test_dots(r0, r1, r2, nd);
        v3 hp = V3(0.0f, 0.0f, 0.0f);
        float dist;
        (void)exact_hit(td, r0.w, tris15 + (size_t)15 * tri, S, &hp, &dist);
        return hp;
    }
};

// Slot `slot` of ray `ray`: the winner `key` as a whole struct Intersection -- its position from `retest` --, or Update()'s reset for
// an empty entry.
template <class Retest>
__device__ __forceinline__ void order_store_slot(const OrderOut &o, long long ray, int slot, unsigned long long key, const Retest &retest)
{
    uint32_t *h = o.hits + (size_t)HIT_WORDS * ((size_t)ray * (size_t)o.max_hits + (size_t)slot);
    if (key == HIT_KEY_NONE) {
        store_record(h, V3(0.0f, 0.0f, 0.0f), 0x7f7fffffu, 0xffffffffu);                   // :335-339: FLT_MAX, -1
        return;
    }
    const int tri = hit_key_index(key);
    store_record(h, retest(tri), hit_key_distance_bits(key), (uint32_t)tri);
}

// A lane's whole answer: its max_hits slots from its own list, and the count.
template <int K, class Retest>
__device__ __forceinline__ void order_store_list(const OrderOut &o, long long ray, const HitList<K> &l, const Retest &retest)
{
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < K; s++)
        if (s < o.max_hits) {
            order_store_slot(o, ray, s, l.k[s], retest);
            cnt += (int)(l.k[s] != HIT_KEY_NONE);
        }
    o.counts[ray] = cnt;
}

}  // namespace mirt
