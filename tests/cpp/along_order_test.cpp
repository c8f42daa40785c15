// The bound rule of the ordered hits along a direction (order/order_bound.hpp) together with the list rule (order/hit_list.hpp),
// against a plain sort, on the CPU (built with -ffp-contract=off like the library).
//
// A ray's input is laid out as the structure of along/along.hpp lays it out: the rows of its cell, shells in rising order (a row's
// shell is bin_shell_of(near), rows within a shell in any order), each accepted row carrying near <= rs + dist in float -- rows with
// near exactly AT rs + dist among them --, then an unordered every-ray list (no depth bound); some rows stand both in the cell and on
// that list.  The model walk is k_along_order's: the threshold rs + bound with the list's K-th distance for bound (FLT_MAX while the
// list is not full), the cell list's end at the threshold's shell + 1, the row skipped when near > threshold, both moved after every
// accepted row; then the every-ray list whole.  It must return the first K of the sort of all eligible (distance, index) pairs, for
// K = 1, 2, 4, 8, with ties at the K-th distance on both sides of the cut, behind `after` records of every kind of
// tests/ordered_helpers.py: after_records, and for rays with fewer than K hits.
// A planted fault -- the row skipped when near >= threshold -- must be caught.
//
// The far regime: |rs| in [2^8, 2^12) -- a scene a thousand units from the origin -- with distances in [0.01, 3], a few floats apart.
// One ulp of rs + d is then up to 2.4e-4 and a thousand ulps of d: distinct distances collapse onto one threshold, rows of a SMALLER
// distance stand with near exactly AT the threshold of the list's bound, and only the strictness of the reject keeps them.  The rays
// with two distinct eligible distances of one float sum, and those where such a pair straddles the cut at K = 1, 2, 4 or 8, are
// counted (floors below), and the planted fault must be caught by this regime alone.
//
// Two builds.  Plain g++ under the address and undefined-behaviour sanitizers: the headers of the rule are plain C++, the shell of a
// depth is shell_model below -- a monotone clamp, in this file's own words.  The library's own bin_shell_of (csrc/rt_binned.hpp) is
// HIP source: with -DALONG_ORDER_LIBRARY_SHELL, as the host side of a hipcc build, the same program runs on it, checks that the model
// equals it on a sweep of depths, and states what it returns for thresholds of +inf and FLT_MAX.
#ifdef ALONG_ORDER_LIBRARY_SHELL
#include "../../cpp-raytracer-rasterizer_amd/along/along.hpp"
#endif
#include "../../cpp-raytracer-rasterizer_amd/order/order_bound.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <vector>

using namespace mirt;

// bin_shell_of in this file's words: shell (int)((x - d0) * iw) clamped to [0, shells - 1]; 0 for a NaN product.
static uint32_t shell_model(float x, float d0, float iw, int shells)
{
    const float s = (x - d0) * iw;
    if (!(s >= 0.0f)) return 0u;
    return s >= (float)(shells - 1) ? (uint32_t)(shells - 1) : (uint32_t)(int)s;
}
#ifdef ALONG_ORDER_LIBRARY_SHELL
static uint32_t shell_of(float x, float d0, float iw, int shells) { return bin_shell_of(x, d0, iw, shells); }
constexpr int SHELLS = ALONG_SHELLS;
#else
static uint32_t shell_of(float x, float d0, float iw, int shells) { return shell_model(x, d0, iw, shells); }
constexpr int SHELLS = 8;                                          // along/along.hpp: ALONG_SHELLS
#endif

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni(double a, double b) { return a + (b - a) * (double)(rnd() >> 11) / 9007199254740992.0; }
static int pick(int n) { return (int)(rnd() % (uint64_t)n); }

struct Row { int tri; float near; bool accepted; float dist; };
struct Ray {
    float rs, d0, iw;
    int shells;
    std::vector<Row> rows;           // the cell's rows in key order, then the every-ray list
    std::vector<uint32_t> off;       // shells + 1 offsets into rows; the every-ray list is [off[shells], rows.size())
};

// One ray's rows.  Distances come from a small set so that ties abound; `flat`: the direction's shells have no width (iw = 0).
// `far`: rs of magnitude 2^8 .. 2^12 with the shells laid around it, distances in [0.01, 3] that differ by 0 .. 3 floats.
static Ray make_ray(int nrows, bool flat, bool far = false)
{
    Ray r;
    r.shells = SHELLS;
    r.rs = far ? (float)((pick(2) ? 1.0 : -1.0) * ldexp(uni(1.0, 2.0), 8 + pick(4))) : (float)uni(-6.0, 2.0);
    r.d0 = far ? (float)((double)r.rs + uni(-1.0, 2.0)) : (float)uni(-3.0, -1.0);
    r.iw = flat ? 0.0f : (float)(r.shells / uni(2.0, 6.0));
    const int ndist = 1 + pick(6);
    float dists[6];
    for (int i = 0; i < ndist; i++) dists[i] = far ? (float)uni(0.01, 3.0) : (pick(9) == 0 ? 0.0f : (float)uni(0.0, 9.0));
    std::vector<Row> cell, every;
    for (int i = 0; i < nrows; i++) {
        Row w;
        w.tri = pick(4 * nrows + 4);
        w.accepted = pick(4) != 0;
        w.dist = dists[pick(ndist)];
        if (far)
            for (int step = pick(4); step > 0; step--) w.dist = nextafterf(w.dist, INFINITY);
        if (pick(40) == 0) w.dist = pick(2) ? INFINITY : NAN;                // accepted by the test, not eligible
        const float sum = r.rs + (w.accepted && w.dist == w.dist && w.dist < INFINITY ? w.dist : (float)(far ? uni(0.01, 3.0) : uni(0.0, 9.0)));
        // near <= rs + dist: exactly at it, one float below, or well below
        const int how = pick(4);
        w.near = how == 0 ? sum : (how == 1 ? nextafterf(sum, -INFINITY) : sum - (float)uni(0.0, 3.0));
        if (pick(5) == 0) { w.near = -INFINITY; every.push_back(w); }
        else cell.push_back(w);
    }
    // one tri, one distance: a row offered twice is the same triangle
    std::sort(cell.begin(), cell.end(), [](const Row &a, const Row &b) { return a.tri < b.tri; });
    for (size_t i = 1; i < cell.size(); i++)
        if (cell[i].tri == cell[i - 1].tri) cell[i].tri = -1;
    cell.erase(std::remove_if(cell.begin(), cell.end(), [](const Row &a) { return a.tri < 0; }), cell.end());
    for (Row &e : every)
        for (const Row &c : cell)
            if (c.tri == e.tri) { e.accepted = c.accepted; e.dist = c.dist; }   // (in the cell AND on the list: the same test result)
    for (size_t i = 0; i < every.size(); i++)
        for (size_t j = 0; j < i; j++)
            if (every[j].tri == every[i].tri) { every[i].accepted = every[j].accepted; every[i].dist = every[j].dist; }
    // some cell rows stand on the every-ray list too
    for (const Row &c : cell)
        if (pick(8) == 0) { Row e = c; e.near = -INFINITY; every.push_back(e); }
    // key order: shell rising, any order within
    for (size_t i = cell.size(); i > 1; i--) std::swap(cell[i - 1], cell[(size_t)pick((int)i)]);
    std::stable_sort(cell.begin(), cell.end(), [&](const Row &a, const Row &b) {
        return shell_of(a.near, r.d0, r.iw, r.shells) < shell_of(b.near, r.d0, r.iw, r.shells);
    });
    for (size_t i = every.size(); i > 1; i--) std::swap(every[i - 1], every[(size_t)pick((int)i)]);
    r.off.assign((size_t)r.shells + 1, 0u);
    for (const Row &c : cell)
        for (uint32_t s = shell_of(c.near, r.d0, r.iw, r.shells) + 1u; s <= (uint32_t)r.shells; s++) r.off[s]++;
    r.rows = cell;
    r.rows.insert(r.rows.end(), every.begin(), every.end());
    return r;
}

// k_along_order's walk.  `fault`: the skip is not strict.  *offered counts the rows the walk looked at.
template <int K>
static HitList<K> model_walk(const Ray &r, float a, int k, bool fault, long *offered)
{
    HitList<K> l;
    hit_list_clear(l);
    if (!(a == a)) return l;                                               // a NaN record admits nothing: no walk
    float thr = along_order_threshold(r.rs, order_bound(hit_list_bound(l)));
    uint32_t end = r.off[order_shells(shell_of(thr, r.d0, r.iw, r.shells))];
    for (uint32_t e = 0; e < end; e++) {
        const Row &w = r.rows[e];
        ++*offered;
        const bool near_ok = fault ? !(w.near >= thr) : order_near_ok(w.near, thr);
        if (!near_ok || !w.accepted) continue;
        hit_list_consider(l, w.dist, w.tri, a, k);
        thr = along_order_threshold(r.rs, order_bound(hit_list_bound(l)));
        end = std::min(end, r.off[order_shells(shell_of(thr, r.d0, r.iw, r.shells))]);
    }
    for (size_t e = r.off[(size_t)r.shells]; e < r.rows.size(); e++) {
        const Row &w = r.rows[e];
        ++*offered;
        if (!order_near_ok(w.near, thr) || !w.accepted) continue;
        hit_list_consider(l, w.dist, w.tri, a, k);
        thr = along_order_threshold(r.rs, order_bound(hit_list_bound(l)));
    }
    return l;
}

// The plain sort: every accepted row whose distance a fresh record takes and that comes behind (a, k), once per triangle.
static std::vector<unsigned long long> plain_sort(const Ray &r, float a, int k)
{
    std::vector<unsigned long long> keys;
    for (const Row &w : r.rows)
        if (w.accepted && FLT_MAX >= w.dist && (w.dist > a || (w.dist == a && w.tri < k))) keys.push_back(hit_key(w.dist, w.tri));
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    return keys;
}

struct Tally { long rays = 0, calls = 0, wrong = 0, caught = 0, short_lists = 0, ties_at_cut = 0, near_at_sum = 0, rows = 0, offered = 0, dup = 0, collide = 0, collide_at_cut = 0; };

// The far regime's floors, half of what a run shows: of 6000 rays 4849 hold a collision and 4101 one at a cut with shell_model, 4832
// and 4070 on the library's shells (that build draws its depth sweep first); none of the 6000 rays around the origin holds one.
constexpr long FAR_COLLISIONS_FLOOR = 2400, FAR_AT_CUT_FLOOR = 2000;

// Two distinct eligible distances of the ray with one float sum rs + d: anywhere in its sorted hits (*any), and as the K-th and the
// (K + 1)-th of them for K = 1, 2, 4 or 8 (*at_cut).
static void collisions(const Ray &r, bool *any, bool *at_cut)
{
    const std::vector<unsigned long long> all = plain_sort(r, -1.0f, 0);
    *any = *at_cut = false;
    for (size_t i = 0; i + 1 < all.size(); i++) {
        const float a = hit_bits_float(hit_key_distance_bits(all[i])), b = hit_bits_float(hit_key_distance_bits(all[i + 1]));
        if (a != b && r.rs + a == r.rs + b) {
            *any = true;
            if (i == 0 || i == 1 || i == 3 || i == 7) *at_cut = true;
        }
    }
}

template <int K>
static void check(const Ray &r, float a, int k, Tally &T)
{
    const std::vector<unsigned long long> want = plain_sort(r, a, k);
    long offered = 0, unused = 0;
    const HitList<K> got = model_walk<K>(r, a, k, false, &offered);
    const HitList<K> bad = model_walk<K>(r, a, k, true, &unused);
    bool ok = true, bad_ok = true;
    for (int s = 0; s < K; s++) {
        const unsigned long long w = (size_t)s < want.size() ? want[(size_t)s] : HIT_KEY_NONE;
        ok = ok && got.k[s] == w;
        bad_ok = bad_ok && bad.k[s] == w;
    }
    T.calls++;
    T.offered += offered;
    T.rows += (long)r.rows.size();
    if (!ok) {
        if (T.wrong++ < 5) fprintf(stderr, "K %d: the walk differs from the sort (rs %a, after %a / %d, %zu eligible)\n", K, r.rs, a, k, want.size());
    }
    if (!bad_ok) T.caught++;
    if (want.size() < (size_t)K) T.short_lists++;
    if (want.size() > (size_t)K && hit_key_distance_bits(want[(size_t)K]) == hit_key_distance_bits(want[(size_t)K - 1])) T.ties_at_cut++;
}

int main()
{
    // what the shell of a threshold is at the ends: +inf and FLT_MAX, with a shell width and without
    const uint32_t inf_w = shell_of(INFINITY, -2.0f, 1.5f, SHELLS), max_w = shell_of(FLT_MAX, -2.0f, 1.5f, SHELLS);
    const uint32_t inf_0 = shell_of(INFINITY, -2.0f, 0.0f, SHELLS), max_0 = shell_of(FLT_MAX, -2.0f, 0.0f, SHELLS);
    const uint32_t sum_w = shell_of(-5.0f + FLT_MAX, -2.0f, 1.5f, SHELLS);
#ifdef ALONG_ORDER_LIBRARY_SHELL
    printf("bin_shell_of: ");
    long differ = 0;
    for (int i = 0; i < 200000; i++) {
        const float d0 = (float)uni(-3.0, -1.0), iw = i % 9 == 0 ? 0.0f : (float)(SHELLS / uni(2.0, 6.0));
        const float x = i % 5 == 0 ? (float)uni(-1e30, 1e30) : (float)uni(-8.0, 12.0);
        differ += (long)(bin_shell_of(x, d0, iw, SHELLS) != shell_model(x, d0, iw, SHELLS));
    }
    printf("model_differs %ld; ", differ);
    if (differ) { printf("FAILED\n"); return 1; }
#else
    printf("shell_model: ");
#endif
    printf("+inf -> %u, FLT_MAX -> %u, rs + FLT_MAX -> %u of %d shells; with no shell width +inf -> %u (inf * 0 is NaN), FLT_MAX -> %u\n",
           inf_w, max_w, sum_w, SHELLS, inf_0, max_0);
    if (inf_w != SHELLS - 1 || max_w != SHELLS - 1 || sum_w != SHELLS - 1 || inf_0 != 0u || max_0 != 0u) { printf("FAILED\n"); return 1; }
    if (order_bound(INFINITY) != FLT_MAX || order_bound(3.5f) != 3.5f || order_bound(0.0f) != 0.0f) { printf("FAILED\n"); return 1; }

    Tally N, F;                                                         // the regime around the origin (first, as it always ran), the far one
    for (int it = 0; it < 12000; it++) {
        const bool far = it >= 6000;
        Tally &T = far ? F : N;
        const Ray r = make_ray(it % 7 == 0 ? pick(4) : 2 + pick(40), it % 11 == 0, far);
        T.rays++;
        bool any, at_cut;
        collisions(r, &any, &at_cut);
        T.collide += (long)any;
        T.collide_at_cut += (long)at_cut;
        for (const Row &w : r.rows) T.near_at_sum += (long)(w.accepted && w.near == r.rs + w.dist);
        for (size_t e = r.off[(size_t)r.shells]; e < r.rows.size(); e++)
            for (size_t c = 0; c < r.off[(size_t)r.shells]; c++) T.dup += (long)(r.rows[c].tri == r.rows[e].tri);
        // the ray's own first hit, for the `after` kinds
        const std::vector<unsigned long long> all = plain_sort(r, -1.0f, 0);
        const float d = all.empty() ? 1.0f : hit_bits_float(hit_key_distance_bits(all[0]));
        const int ix = all.empty() ? 3 : hit_key_index(all[0]);
        const float qnan = hit_bits_float(0x7fc00000u);
        const float ad[11] = { -1.0f, d, d, d, d, d, nextafterf(d, INFINITY), nextafterf(d, 0.0f), FLT_MAX, INFINITY, qnan };
        const int ai[11] = { ix, -1, ix, ix - 1, ix + 1, INT_MAX, ix, ix, ix, ix, ix };
        for (int kind = 0; kind < 11; kind++) {
            if (kind > 0 && (it + kind) % 3) continue;                         // (every ray from the start, a third of the other kinds)
            check<1>(r, ad[kind], ai[kind], T);
            check<2>(r, ad[kind], ai[kind], T);
            check<4>(r, ad[kind], ai[kind], T);
            check<8>(r, ad[kind], ai[kind], T);
        }
    }
    const Tally &T = N;
    printf("rays %ld calls %ld wrong %ld planted_fault_caught %ld short_lists %ld ties_at_cut %ld near_at_sum %ld in_cell_and_on_list %ld rows %ld offered %ld\n",
           T.rays, T.calls, T.wrong, T.caught, T.short_lists, T.ties_at_cut, T.near_at_sum, T.dup, T.rows, T.offered);
    printf("far: rays %ld calls %ld wrong %ld planted_fault_caught %ld short_lists %ld ties_at_cut %ld near_at_sum %ld collisions %ld collisions_at_cut %ld "
           "rows %ld offered %ld (collisions around the origin: %ld)\n",
           F.rays, F.calls, F.wrong, F.caught, F.short_lists, F.ties_at_cut, F.near_at_sum, F.collide, F.collide_at_cut, F.rows, F.offered, N.collide);
    bool pass = T.wrong == 0 && T.caught > 0 && T.short_lists > 100 && T.ties_at_cut > 100 && T.near_at_sum > 1000 && T.dup > 100 && T.offered < T.rows;
    // the far regime alone: right, the planted fault caught, and its collisions above their floors
    pass = pass && F.wrong == 0 && F.caught > 0 && F.collide >= FAR_COLLISIONS_FLOOR && F.collide_at_cut >= FAR_AT_CUT_FLOOR && F.offered < F.rows;
    printf(pass ? "ok\n" : "FAILED\n");
    return pass ? 0 : 1;
}
