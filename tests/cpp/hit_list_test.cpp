// The list rule of mirt_intersect_ordered* (order/hit_list.hpp) on the CPU, against a plain sort:
//   1. seeded offer sequences -- a table of triangles (index, distance) offered in random order with repeats -- through
//      hit_list_consider<K>, K = 1, 2, 4, 8, under `after` records of every kind; after EVERY offer the list equals the first K of the
//      eligible triangles offered so far, sorted by (distance rising, index falling) with float and int comparisons, and the bound is
//      +inf until the list is full and the K-th distance from then on;
//      the distances include runs of equal values with rising and falling indices, 0 and -0.0f, subnormals, neighbouring floats,
//      FLT_MAX, +inf and NaN; the indices 0 and INT_MAX;
//      the `after` records: before everything (-1), at an entry, one float above and one float below an entry's distance, a tie with
//      index -1 and with INT_MAX, -0.0f, FLT_MAX, +inf and NaN;
//   2. the same sequences through a planted fault -- a chain that does not drop a key equal to an entry -- must be caught.
#include "../../cpp-raytracer-rasterizer_amd/order/hit_list.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mirt;

static uint32_t rng_state = 2463534242u;
static uint32_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

struct Tri { float d; int j; };

// the order of the contract, as written there
static bool before(const Tri &x, const Tri &y) { return x.d < y.d || (x.d == y.d && x.j > y.j); }

struct Good {
    template <int K> static void consider(HitList<K> &l, float d, int j, float a, int k) { hit_list_consider(l, d, j, a, k); }
};
// the planted fault: hit_list_consider with a chain that carries an equal key on instead of dropping it
struct KeepsEqualKeys {
    template <int K> static void consider(HitList<K> &l, float d, int j, float a, int k)
    {
        if (!(hit_eligible(d) && hit_after(d, j, a, k))) return;
        unsigned long long x = hit_key(d, j);
        if (!(x < l.k[K - 1])) return;
        for (int i = 0; i < K; i++) {
            const unsigned long long e = l.k[i];
            l.k[i] = e < x ? e : x;
            x = e < x ? x : e;
        }
    }
};

static float some_distance(int kind)
{
    const float base[] = { 0.0f, -0.0f, 1.401298464e-45f, FLT_MIN, 0.5f, 1.0f, 1.0f, 2.75f, 1e10f, FLT_MAX, INFINITY, NAN };
    if (kind < 12) return base[kind];
    if (kind < 16) return std::nextafterf(kind & 1 ? 1.0f : 0.5f, kind & 2 ? 4.0f : 0.0f);
    return (float)(rng() % 1000u) * 0.01f;                         // a coarse lattice: many exact ties
}

// One sequence under one `after` record through list length K; returns the number of offers after which the list (or its bound)
// differs from the sort's.
template <int K, class Rule>
static long run_sequence(const std::vector<Tri> &offers, float a, int k, long *full_lists)
{
    long wrong = 0;
    HitList<K> l;
    hit_list_clear(l);
    std::vector<Tri> seen;                                          // the eligible triangles offered so far, each once
    for (const Tri &t : offers) {
        Rule::template consider<K>(l, t.d, t.j, a, k);
        const bool eligible = FLT_MAX >= t.d && (t.d > a || (t.d == a && t.j < k));
        bool known = false;
        for (const Tri &s : seen) known |= s.j == t.j;
        if (eligible && !known) seen.push_back(t);
        std::sort(seen.begin(), seen.end(), before);
        bool same = true;
        for (int i = 0; i < K; i++) {
            // (-0.0f is keyed as the 0.0f it equals)
            const unsigned long long want = i < (int)seen.size() ? hit_key(seen[i].d, seen[i].j) : HIT_KEY_NONE;
            same &= l.k[i] == want;
            if (i < (int)seen.size()) same &= hit_key_index(l.k[i]) == seen[i].j && hit_bits_float(hit_key_distance_bits(l.k[i])) == seen[i].d;
        }
        const float bound = hit_list_bound(l);
        if ((int)seen.size() >= K) { same &= bound == seen[K - 1].d; (*full_lists)++; }
        else same &= std::isinf(bound) && bound > 0.0f;
        wrong += same ? 0 : 1;
    }
    return wrong;
}

template <class Rule>
static long run_all(long *sequences, long *offers_made, long *full_lists)
{
    long wrong = 0;
    rng_state = 2463534242u;
    for (int seq = 0; seq < 300; seq++) {
        // the table: unique indices, each with one distance; every third table is a run of equal distances over rising indices
        std::vector<Tri> table;
        const int ntri = 1 + (int)(rng() % 24u);
        for (int t = 0; t < ntri; t++) {
            int j = seq % 4 == 0 ? (t == 0 ? 0 : (t == 1 ? INT_MAX : (int)(rng() & 0x7fffffffu))) : (int)(rng() % 64u);
            bool dup = false;
            for (const Tri &s : table) dup |= s.j == j;
            if (dup) continue;
            const float d = seq % 3 == 0 ? some_distance(4 + (int)(rng() % 3u)) : some_distance((int)(rng() % 24u));
            table.push_back({ d, j });
        }
        // the offers: the table rising, falling or shuffled, then a third of it again (a row offered twice)
        std::vector<Tri> offers = table;
        std::sort(offers.begin(), offers.end(), [](const Tri &x, const Tri &y) { return x.j < y.j; });
        if (seq % 3 == 1) std::reverse(offers.begin(), offers.end());
        if (seq % 3 == 2) for (size_t i = offers.size(); i > 1; i--) std::swap(offers[i - 1], offers[rng() % i]);
        const size_t n0 = offers.size();
        for (size_t i = 0; i < n0; i++) if (rng() % 3u == 0) offers.push_back(offers[rng() % n0]);
        // the `after` records, around an entry of the table
        const Tri e = table[rng() % table.size()];
        const float ed = std::isfinite(e.d) ? e.d : 1.0f;
        const struct { float a; int k; } afters[] = {
            { -1.0f, 0 }, { ed, e.j }, { std::nextafterf(ed, INFINITY), e.j }, { std::nextafterf(ed, -INFINITY), e.j }, { ed, -1 }, { ed, INT_MAX },
            { -0.0f, INT_MAX }, { 0.0f, -1 }, { FLT_MAX, -1 }, { FLT_MAX, INT_MAX }, { INFINITY, INT_MAX }, { NAN, INT_MAX } };
        for (const auto &af : afters) {
            wrong += run_sequence<1, Rule>(offers, af.a, af.k, full_lists);
            wrong += run_sequence<2, Rule>(offers, af.a, af.k, full_lists);
            wrong += run_sequence<4, Rule>(offers, af.a, af.k, full_lists);
            wrong += run_sequence<8, Rule>(offers, af.a, af.k, full_lists);
            *sequences += 4;
            *offers_made += 4 * (long)offers.size();
        }
    }
    return wrong;
}

int main()
{
    // the predicate on its own: the cases the key comparison would get wrong
    if (!(hit_after(0.0f, 3, -0.0f, 4) && !hit_after(0.0f, 4, -0.0f, 4) && hit_after(1e-30f, 0, -0.0f, INT_MAX))) { printf("FAILED -0.0f\n"); return 1; }
    if (hit_after(1.0f, 0, NAN, INT_MAX) || hit_after(FLT_MAX, 0, NAN, INT_MAX)) { printf("FAILED NaN admits\n"); return 1; }
    if (!hit_after(0.0f, INT_MAX, -1.0f, -1) || hit_after(1.0f, 5, 1.0f, -1) || !hit_after(1.0f, 5, 1.0f, INT_MAX)) { printf("FAILED ties\n"); return 1; }
    if (hit_after(FLT_MAX, 0, FLT_MAX, -1) || hit_eligible(INFINITY) || hit_eligible(NAN) || !hit_eligible(FLT_MAX) || !hit_eligible(0.0f)) { printf("FAILED eligibility\n"); return 1; }
    if (hit_list_size_for(1) != 1 || hit_list_size_for(2) != 2 || hit_list_size_for(3) != 4 || hit_list_size_for(4) != 4 || hit_list_size_for(5) != 8 ||
        hit_list_size_for(8) != 8) { printf("FAILED sizes\n"); return 1; }

    long sequences = 0, offers = 0, full = 0, s2 = 0, o2 = 0, f2 = 0;
    const long wrong = run_all<Good>(&sequences, &offers, &full);
    const long caught = run_all<KeepsEqualKeys>(&s2, &o2, &f2);
    printf("sequences %ld offers %ld full_lists %ld wrong %ld planted_fault_caught %ld\n", sequences, offers, full, wrong, caught);
    if (wrong != 0) { printf("FAILED: the list differs from the sort after %ld offers\n", wrong); return 1; }
    if (caught == 0) { printf("FAILED: a list that keeps equal keys passes: the sequences offer nothing twice\n"); return 1; }
    if (full < 1000) { printf("FAILED: hardly any list ever fills\n"); return 1; }
    printf("ok\n");
    return 0;
}
