// hit_list.hpp -- the K first hits of a ray in the reference's own order (mirt_intersect_ordered*): the one rule of the list, for the
// kernels (ordered_hits.hip), the host (../capi/order.cpp) and tests/cpp/hit_list_test.cpp.  Plain C++ under any compiler; MIRT_HD
// under hipcc.
//
// The order.  ClosestIntersection (raytracer.cpp:202-257) accepts a set of triangles per ray, each with a distance d_j (:242), and its
// record rule `closest.distance >= distance` (:243) ranks them: the smaller distance first, and among equal distances the LATER index
// first (the later triangle of a tie replaces the earlier).  "The first of that order" is what mirt_intersect returns on a fresh record;
// "the K first" is this list.
//
// The key.  A triangle is eligible when a fresh record would take it, FLT_MAX >= d_j: such a distance is a square root, so >= +0, not
// NaN and finite, and its bits order as an unsigned integer the way the floats order.  With 0xFFFFFFFF - index in the low word the
// 64-bit keys order exactly as the rule above (../csrc/rt_common.hpp: min_t_key is the same packing), equal keys mean the same
// triangle, and the all-ones key -- above every real one -- stands for an empty entry.
//
// The `after` record of a continuation is NOT compared by key: -0.0f must behave as 0.0f and a NaN must admit nothing, which the float
// and signed-int comparisons as written do and the bit patterns do not.
#pragma once

#if defined(__HIPCC__)
#include "../csrc/mirt_math.hpp"
#else
#define MIRT_HD inline
#endif
#if defined(__clang__)
#define HIT_UNROLL _Pragma("unroll")
#else
#define HIT_UNROLL
#endif

#include <float.h>
#include <stdint.h>
#include <string.h>

namespace mirt {

constexpr int HIT_LIST_MAX = 8;                                   // MIRT_MAX_ORDERED_HITS
constexpr unsigned long long HIT_KEY_NONE = ~0ull;

MIRT_HD uint32_t hit_float_bits(float x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __float_as_uint(x);
#else
    uint32_t u; memcpy(&u, &x, 4); return u;
#endif
}
MIRT_HD float hit_bits_float(uint32_t u)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(u);
#else
    float x; memcpy(&x, &u, 4); return x;
#endif
}

// (dist + 0.0f: -0.0f, which no square root of a sum of squares yields, is keyed as the 0.0f it compares equal to; every other value
// is unchanged)
MIRT_HD unsigned long long hit_key(float dist, int index)
{
    return ((unsigned long long)hit_float_bits(dist + 0.0f) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)index);
}
MIRT_HD int hit_key_index(unsigned long long key) { return (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)); }
MIRT_HD uint32_t hit_key_distance_bits(unsigned long long key) { return (uint32_t)(key >> 32); }

// What a fresh record takes (:243 with closest.distance = FLT_MAX): never a NaN or +inf distance.
MIRT_HD bool hit_eligible(float d) { return FLT_MAX >= d; }

// Whether triangle j at distance d comes strictly behind the record (a, k) in the order: float and signed-int comparisons as written.
// A NaN a admits nothing, a negative a everything, -0.0f is 0.0f.
MIRT_HD bool hit_after(float d, int j, float a, int k) { return d > a || (d == a && j < k); }

// The list: at most K keys, ascending, empty entries (HIT_KEY_NONE) behind them.  Always indexed by constants, so that the entries
// are registers of their own.
template <int K> struct HitList { unsigned long long k[K]; };

template <int K> MIRT_HD void hit_list_clear(HitList<K> &l)
{
    HIT_UNROLL
    for (int i = 0; i < K; i++) l.k[i] = HIT_KEY_NONE;
}

// The list's bound: the K-th entry's distance once the list is full -- nothing farther can still enter --, +inf before.
template <int K> MIRT_HD float hit_list_bound(const HitList<K> &l)
{
    return l.k[K - 1] == HIT_KEY_NONE ? hit_bits_float(0x7f800000u) : hit_bits_float(hit_key_distance_bits(l.k[K - 1]));
}

// Offers `key`: a compare-and-swap chain down the list.  The smaller of (entry, carried key) stays, the larger is carried on; a key
// equal to an entry is dropped there (the carried key becomes the empty one, which moves nothing), so a row offered twice changes
// nothing the second time.  What falls off the end is the (K + 1)-th.  Returns the bound.
template <int K> MIRT_HD float hit_list_offer(HitList<K> &l, unsigned long long key)
{
    unsigned long long x = key;
    HIT_UNROLL
    for (int i = 0; i < K; i++) {
        const unsigned long long a = l.k[i];
        const unsigned long long lo = a < x ? a : x, hi = a < x ? x : a;
        l.k[i] = lo;
        x = a == x ? HIT_KEY_NONE : hi;
    }
    return hit_list_bound(l);
}

// An accepted triangle `tri` at distance `dist`, for a ray that continues behind (a, k): into the list when it is eligible and behind
// the record.  A key that is not below the list's last entry is that entry again or falls off the end: no chain for it.
template <int K> MIRT_HD void hit_list_consider(HitList<K> &l, float dist, int tri, float a, int k)
{
    if (hit_eligible(dist) && hit_after(dist, tri, a, k)) {
        const unsigned long long key = hit_key(dist, tri);
        if (key < l.k[K - 1]) hit_list_offer(l, key);
    }
}

// The head leaves the list (the wave kernel's extraction rounds).
template <int K> MIRT_HD void hit_list_pop(HitList<K> &l)
{
    HIT_UNROLL
    for (int i = 0; i + 1 < K; i++) l.k[i] = l.k[i + 1];
    l.k[K - 1] = HIT_KEY_NONE;
}

// The instantiation that serves max_hits: 1, 2, 4 or 8.
inline int hit_list_size_for(int max_hits) { return max_hits <= 1 ? 1 : (max_hits <= 2 ? 2 : (max_hits <= 4 ? 4 : 8)); }

}  // namespace mirt
