// The admission rule of the hit counts (count/count_rule.hpp) and a model of the count walk along a direction (count/count_walk.hpp),
// against a plain count, on the CPU (built with -ffp-contract=off like the library).
//
// A ray's input is laid out as the structure of along/along.hpp lays it out: the rows of its cell, shells in rising order (a row's
// shell is bin_shell_of(near), rows within a shell in any order), each accepted row carrying near <= rs + dist in float -- rows with
// near exactly AT rs + dist among them --, then an unordered every-ray list (no depth bound).  Every triangle stands on ONE of the two
// lists, once: what along_file_triangles files.  The model walk is along_count_walk's: no list at all for a ray that is not open
// (count_open), the threshold count_threshold(rs, L), the cell list's end at the threshold's shell + 1, the row skipped when
// near > threshold (order_near_ok), an accepted row counted when count_admits says so; then the every-ray list whole.  It must return
// the plain count: the accepted rows with FLT_MAX >= d, behind `after`, with d < L.
//
// The limits sit at one of the ray's own distances, one float above it and one float below it, at +inf, FLT_MAX, NaN, 0 and -1, and
// there are calls without one; the `after` records are every kind of tests/ordered_helpers.py: after_records.  In the far regime
// (|rs| in [2^8, 2^12), distances a few floats apart) distinct distances collapse onto one float sum rs + d: rows of a distance BELOW
// the limit stand with near exactly AT the threshold, and only the strictness of the reject keeps them.
//
// Two planted faults must be caught: the row skipped when near >= threshold, and a row offered twice (some cell rows stand on the
// every-ray list as well -- what a structure that files a triangle under several keys of one ray would do).
//
// Two builds.  Plain g++ under the address and undefined-behaviour sanitizers with shell_model below -- a monotone clamp, in this
// file's own words; and with -DCOUNT_RULE_LIBRARY_SHELL, as the host side of a hipcc build, on the library's own bin_shell_of.
#ifdef COUNT_RULE_LIBRARY_SHELL
#include "../../cpp-raytracer-rasterizer_amd/along/along.hpp"
#endif
#include "../../cpp-raytracer-rasterizer_amd/count/count_rule.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <vector>

using namespace mirt;

static uint32_t shell_model(float x, float d0, float iw, int shells)
{
    const float s = (x - d0) * iw;
    if (!(s >= 0.0f)) return 0u;
    return s >= (float)(shells - 1) ? (uint32_t)(shells - 1) : (uint32_t)(int)s;
}
#ifdef COUNT_RULE_LIBRARY_SHELL
static uint32_t shell_of(float x, float d0, float iw, int shells) { return bin_shell_of(x, d0, iw, shells); }
constexpr int SHELLS = ALONG_SHELLS;
#else
static uint32_t shell_of(float x, float d0, float iw, int shells) { return shell_model(x, d0, iw, shells); }
constexpr int SHELLS = 8;                                          // along/along.hpp: ALONG_SHELLS
#endif

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double uni(double a, double b) { return a + (b - a) * (double)(rnd() >> 11) / 9007199254740992.0; }
static int pick(int n) { return (int)(rnd() % (uint64_t)n); }

struct Row { int tri; float near; bool accepted; float dist; };
struct Ray {
    float rs, d0, iw;
    std::vector<Row> rows;           // the cell's rows in key order, then the every-ray list
    std::vector<uint32_t> off;       // SHELLS + 1 offsets into rows; the every-ray list is [off[SHELLS], rows.size())
    std::vector<Row> twice;          // the planted fault's extra every-ray rows: cell rows offered a second time
};

// One ray's rows, every triangle once.  `flat`: the direction's shells have no width.  `far`: rs of magnitude 2^8 .. 2^12 with the
// shells laid around it, distances in [0.01, 3] that differ by 0 .. 3 floats.
static Ray make_ray(int nrows, bool flat, bool far)
{
    Ray r;
    r.rs = far ? (float)((pick(2) ? 1.0 : -1.0) * ldexp(uni(1.0, 2.0), 8 + pick(4))) : (float)uni(-6.0, 2.0);
    r.d0 = far ? (float)((double)r.rs + uni(-1.0, 2.0)) : (float)uni(-3.0, -1.0);
    r.iw = flat ? 0.0f : (float)(SHELLS / uni(2.0, 6.0));
    const int ndist = 1 + pick(6);
    float dists[6];
    for (int i = 0; i < ndist; i++) dists[i] = far ? (float)uni(0.01, 3.0) : (pick(9) == 0 ? 0.0f : (float)uni(0.0, 9.0));
    std::vector<Row> cell, every;
    for (int i = 0; i < nrows; i++) {
        Row w;
        w.tri = 3 * i + pick(3);                                               // (distinct, rising: shuffled below)
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
    for (const Row &c : cell)
        if (pick(6) == 0) { Row e = c; e.near = -INFINITY; r.twice.push_back(e); }
    // key order: shell rising, any order within
    for (size_t i = cell.size(); i > 1; i--) std::swap(cell[i - 1], cell[(size_t)pick((int)i)]);
    std::stable_sort(cell.begin(), cell.end(), [&](const Row &a, const Row &b) { return shell_of(a.near, r.d0, r.iw, SHELLS) < shell_of(b.near, r.d0, r.iw, SHELLS); });
    for (size_t i = every.size(); i > 1; i--) std::swap(every[i - 1], every[(size_t)pick((int)i)]);
    r.off.assign((size_t)SHELLS + 1, 0u);
    for (const Row &c : cell)
        for (uint32_t s = shell_of(c.near, r.d0, r.iw, SHELLS) + 1u; s <= (uint32_t)SHELLS; s++) r.off[s]++;
    r.rows = cell;
    r.rows.insert(r.rows.end(), every.begin(), every.end());
    return r;
}

enum Fault { NONE, NOT_STRICT, OFFERED_TWICE };

// along_count_walk.  *offered counts the rows the walk looked at.
static int model_walk(const Ray &r, bool has_after, float a, int k, float L, Fault fault, long *offered)
{
    if (!count_open(has_after, a, L)) return 0;
    const float thr = count_threshold(r.rs, L);
    const uint32_t end = r.off[shell_of(thr, r.d0, r.iw, SHELLS) + 1u];
    int cnt = 0;
    auto offer = [&](const Row &w) {
        ++*offered;
        const bool near_ok = fault == NOT_STRICT ? !(w.near >= thr) : order_near_ok(w.near, thr);
        if (near_ok && w.accepted) cnt += (int)count_admits(w.dist, w.tri, has_after, a, k, L);
    };
    for (uint32_t e = 0; e < end; e++) offer(r.rows[e]);
    for (size_t e = r.off[(size_t)SHELLS]; e < r.rows.size(); e++) offer(r.rows[e]);
    if (fault == OFFERED_TWICE)
        for (const Row &w : r.twice) offer(w);
    return cnt;
}

// The plain count, in this file's own words.
static int plain_count(const Ray &r, bool has_after, float a, int k, bool limited, float L)
{
    int cnt = 0;
    for (const Row &w : r.rows) {
        if (!w.accepted || !(FLT_MAX >= w.dist)) continue;
        if (has_after && !(w.dist > a || (w.dist == a && w.tri < k))) continue;
        if (limited && !(w.dist < L)) continue;
        cnt++;
    }
    return cnt;
}

struct Tally { long rays = 0, calls = 0, wrong = 0, caught_strict = 0, caught_twice = 0, deep = 0, zero = 0, near_at_thr = 0, limit_cuts = 0, rows = 0, offered = 0; };

static void check(const Ray &r, bool has_after, float a, int k, bool limited, float L, Tally &T)
{
    const float Lw = limited ? L : INFINITY;                                   // (no limit array stands for +inf)
    const int want = plain_count(r, has_after, a, k, limited, L);
    long offered = 0, unused = 0;
    const int got = model_walk(r, has_after, a, k, Lw, NONE, &offered);
    T.calls++;
    T.offered += offered;
    T.rows += (long)r.rows.size();
    if (got != want && T.wrong++ < 5)
        fprintf(stderr, "the walk counts %d, the plain count is %d (rs %a, after %d %a / %d, limit %d %a)\n", got, want, r.rs, (int)has_after, a, k, (int)limited, L);
    T.caught_strict += (long)(model_walk(r, has_after, a, k, Lw, NOT_STRICT, &unused) != want);
    T.caught_twice += (long)(model_walk(r, has_after, a, k, Lw, OFFERED_TWICE, &unused) != want);
    T.deep += (long)(want > 8);
    T.zero += (long)(want == 0);
    if (limited && count_open(has_after, a, L)) {
        T.limit_cuts += (long)(want < plain_count(r, has_after, a, k, false, 0.0f));
        const float thr = count_threshold(r.rs, L);
        for (const Row &w : r.rows) T.near_at_thr += (long)(w.accepted && w.near == thr && count_admits(w.dist, w.tri, has_after, a, k, L));
    }
}

int main()
{
    // the predicate at its edges
    const float qnan = hit_bits_float(0x7fc00000u);
    bool rule = count_admits(1.0f, 3, false, 0.0f, 0, INFINITY) && !count_admits(INFINITY, 3, false, 0.0f, 0, INFINITY) && !count_admits(qnan, 3, false, 0.0f, 0, INFINITY) &&
                count_admits(FLT_MAX, 3, false, 0.0f, 0, INFINITY) && !count_admits(FLT_MAX, 3, false, 0.0f, 0, FLT_MAX) && !count_admits(1.0f, 3, false, 0.0f, 0, 1.0f) &&
                count_admits(1.0f, 3, false, 0.0f, 0, nextafterf(1.0f, 2.0f)) && !count_admits(1.0f, 3, false, 0.0f, 0, qnan) && !count_admits(0.0f, 3, false, 0.0f, 0, 0.0f) &&
                count_admits(1.0f, 3, true, 1.0f, 4, 2.0f) && !count_admits(1.0f, 3, true, 1.0f, 3, 2.0f) && !count_admits(1.0f, 3, true, qnan, 9, 2.0f) &&
                count_admits(0.0f, 3, true, -0.0f, 4, 2.0f) && count_admits(0.0f, 3, true, -1.0f, 0, 2.0f);
    rule = rule && count_open(false, qnan, INFINITY) && !count_open(true, qnan, INFINITY) && !count_open(false, 0.0f, 0.0f) && !count_open(false, 0.0f, -1.0f) &&
           !count_open(false, 0.0f, qnan) && count_threshold(-5.0f, INFINITY) == -5.0f + FLT_MAX && count_threshold(2.0f, 3.0f) == 5.0f;
    const uint32_t max_w = shell_of(count_threshold(-5.0f, INFINITY), -2.0f, 1.5f, SHELLS), max_0 = shell_of(count_threshold(-5.0f, INFINITY), -2.0f, 0.0f, SHELLS);
#ifdef COUNT_RULE_LIBRARY_SHELL
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
    printf("rule %s; the threshold without a limit -> shell %u of %d, %u with no shell width\n", rule ? "ok" : "WRONG", max_w, SHELLS, max_0);
    if (!rule || max_w != SHELLS - 1 || max_0 != 0u) { printf("FAILED\n"); return 1; }

    Tally N, F;                                                         // the regime around the origin, the far one
    for (int it = 0; it < 12000; it++) {
        const bool far = it >= 6000;
        Tally &T = far ? F : N;
        const Ray r = make_ray(it % 7 == 0 ? pick(4) : 2 + pick(60), it % 11 == 0, far);
        T.rays++;
        // the ray's eligible distances, and its first hit in the reference's order, for the limits and the `after` kinds
        std::vector<unsigned long long> all;
        for (const Row &w : r.rows)
            if (w.accepted && FLT_MAX >= w.dist) all.push_back(hit_key(w.dist, w.tri));
        std::sort(all.begin(), all.end());
        const float d = all.empty() ? 1.0f : hit_bits_float(hit_key_distance_bits(all[0]));
        const int ix = all.empty() ? 3 : hit_key_index(all[0]);
        const float ad[11] = { -1.0f, d, d, d, d, d, nextafterf(d, INFINITY), nextafterf(d, 0.0f), FLT_MAX, INFINITY, qnan };
        const int ai[11] = { ix, -1, ix, ix - 1, ix + 1, INT_MAX, ix, ix, ix, ix, ix };
        const float at = all.empty() ? 1.0f : hit_bits_float(hit_key_distance_bits(all[(size_t)pick((int)all.size())]));
        const float lim[8] = { at, nextafterf(at, INFINITY), nextafterf(at, 0.0f), INFINITY, FLT_MAX, qnan, 0.0f, -1.0f };
        for (int kind = -1; kind < 11; kind++) {                               // (-1: no `after` at all)
            if (kind > 0 && (it + kind) % 3) continue;                         // (every ray without `after` and from the start, a third of the other kinds)
            const bool has_after = kind >= 0;
            const float a = has_after ? ad[kind] : 0.0f;
            const int k = has_after ? ai[kind] : 0;
            check(r, has_after, a, k, false, 0.0f, T);
            for (int l = 0; l < 8; l++)
                if (l < 3 || (it + kind + l) % 2 == 0) check(r, has_after, a, k, true, lim[l], T);
        }
    }
    printf("rays %ld calls %ld wrong %ld not_strict_caught %ld offered_twice_caught %ld deep %ld zero %ld near_at_threshold %ld limit_cuts %ld rows %ld offered %ld\n",
           N.rays, N.calls, N.wrong, N.caught_strict, N.caught_twice, N.deep, N.zero, N.near_at_thr, N.limit_cuts, N.rows, N.offered);
    printf("far: rays %ld calls %ld wrong %ld not_strict_caught %ld offered_twice_caught %ld deep %ld zero %ld near_at_threshold %ld limit_cuts %ld rows %ld offered %ld\n",
           F.rays, F.calls, F.wrong, F.caught_strict, F.caught_twice, F.deep, F.zero, F.near_at_thr, F.limit_cuts, F.rows, F.offered);
    bool pass = true;
    for (const Tally *T : { &N, &F })
        pass = pass && T->wrong == 0 && T->caught_strict > 0 && T->caught_twice > 0 && T->deep > 100 && T->zero > 100 && T->near_at_thr > 100 &&
               T->limit_cuts > 100 && T->offered < T->rows;
    printf(pass ? "ok\n" : "FAILED\n");
    return pass ? 0 : 1;
}
