// order_device.hpp -- what every kernel of the ordered hits does around its list (device code; ordered_hits.hip and
// ordered_along.hip): the `after` record a ray continues behind, a slot of the answer, and a lane's whole answer.
#pragma once

#include "ordered_hits.hpp"
#include "../query/rt_query_device.hpp"

namespace mirt {

// The record (a, k) ray `ray` continues behind: the caller's, or one that admits everything (no `after`: every eligible distance is
// above -1), or for a lane without a ray one that admits nothing (NaN).
__device__ __forceinline__ void order_after(const OrderFrame &o, long long ray, bool ok, float *a, int *k)
{
    *a = ok ? -1.0f : __uint_as_float(0x7fc00000u);
    *k = 0;
    if (ok && o.after) {
        const uint32_t *r = o.after + (size_t)HIT_WORDS * ray;
        *a = __uint_as_float(r[3]);
        *k = (int)r[4];
    }
}

// Slot `slot` of ray `ray`: the winner `key` as a whole struct Intersection -- its position from the test run once more --, or
// Update()'s reset for an empty entry.
__device__ __forceinline__ void order_store_slot(const OrderFrame &o, long long ray, int slot, unsigned long long key, v3 S, v3 nd)
{
    const QueryFrame &q = o.f.q;
    uint32_t *h = q.hits + (size_t)HIT_WORDS * ((size_t)ray * (size_t)o.max_hits + (size_t)slot);
    if (key == HIT_KEY_NONE) {
        store_record(h, V3(0.0f, 0.0f, 0.0f), 0x7f7fffffu, 0xffffffffu);                   // :335-339: FLT_MAX, -1
        return;
    }
    const int tri = hit_key_index(key);
    const float4 *src = reinterpret_cast<const float4 *>(q.rows + tri);
    const RowVecs r = unpack_row(src[0], src[1], src[2]);
    float e1e2b, dist;
    const TestDots td = ray_dots(r, S, nd, &e1e2b);
    v3 hp = V3(0.0f, 0.0f, 0.0f);
    (void)exact_hit_row(td, e1e2b, r, S, &hp, &dist);
    store_record(h, hp, hit_key_distance_bits(key), (uint32_t)tri);
}

// A lane's whole answer: its max_hits slots from its own list, and the count.
template <int K>
__device__ __forceinline__ void order_store_list(const OrderFrame &o, long long ray, const HitList<K> &l, v3 S, v3 nd)
{
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < K; s++)
        if (s < o.max_hits) {
            order_store_slot(o, ray, s, l.k[s], S, nd);
            cnt += (int)(l.k[s] != HIT_KEY_NONE);
        }
    o.counts[ray] = cnt;
}

// Whether ray `ray` of a call whose rays were written out from (origins, directions, dir_of) names a direction of the call's list
// (o.dir_of NULL: every ray does).  One that names none keeps its slots as the caller left them and gets the count 0.
__device__ __forceinline__ bool order_named(const OrderFrame &o, long long ray)
{
    return !o.dir_of || (uint32_t)o.dir_of[ray] < (uint32_t)o.ndirs;
}

}  // namespace mirt
