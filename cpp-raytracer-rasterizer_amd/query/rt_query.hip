// rt_query.hip -- hand-written gfx950 kernels for ray queries: ClosestIntersection (raytracer/Source/raytracer.cpp:202-257) and
// DirectLight (:265-327) as the free functions they are in the reference, called with rays and Intersection records of the
// caller's own (a mirror bounce, a pick, an occlusion probe, a second light pass) instead of the camera's.
//
// The frame kernels (csrc/) hoist everything of a test that depends on the ray ORIGIN into a per-origin table, because all their
// rays leave one point.  Caller rays share no origin, so here only what depends on no ray at all is hoisted -- v0, e1, e2 and
// e1e2 = cross(e1, e2), one 48-byte QueryRow per triangle (k_query_rows) -- and b = start - v0, be2, e1b and e1e2b are computed
// per (ray, triangle), in the reference's order: 41 non-fused operations a test against 15 of the frame kernels.  The accept
// arithmetic, the conservative filter in front of it and the wave reduction are the shared primitives of csrc/rt_common.hpp.
// Built with -ffp-contract=off like every kernel of the library.
//
// Filter safety.  maybe_hit (rt_common.hpp) never rejects a test the reference accepts PROVIDED every operand of the three dot
// products is finite and below MIRT_SAFE_MAG = 1e18 in magnitude.  The frame path establishes that on the
// host; rays that live in device memory cannot be inspected there, so each kernel decides per ray, once, outside the triangle
// loop (ray_exact_only):
//   * the rows: with V = max |v0|, E1 = max |e1|, E2 = max |e2| over all components of the scene (k_query_rows leaves them as
//     float bits, a NaN ordering above everything) and |start| < 1e8 per component, every |b| component is below B = 1e8 + V, so
//     every component of be2 = cross(b, e2) is below 2 B E2 and of e1b = cross(e1, b) below 2 E1 B (two products each); the
//     scene passes when 2 B max(E1, E2) < 1e18 and max |e1e2| < 1e18 (with all coordinates below 1e8 -- scene_finite -- both hold:
//     B < 2e8, E < 2e8, so 8e16).  e1e2b only feeds t = e1e2b / e1e2d and is not an operand of the filter.
//   * the ray: every |dir| component below 1e6, so each product of a dot is below 1e24 and each sum finite.
// These are the bounds of the frame path (rt_frame.cpp: operands_safe, rt_common.hpp: origin_row_safe).  A ray outside them --
// huge, infinite or NaN components -- runs every test through the exact divisions (its filter verdict is overridden, whatever
// it was).  The filter only ever skips tests the exact path would reject, so no result depends on which path a ray took.
#include "rt_query.hpp"
#include "rt_query_device.hpp"

#include <float.h>

namespace mirt {

// ---- k_query_rows: the ray-independent part of ClosestIntersection, once per scene ----------------------------------
// One thread per triangle.  scene_max (QMAX_WORDS words, zeroed before the launch) receives the largest |component| of each of
// the four vectors as float bits: a butterfly over the wave, then one atomic per wave and word.
__global__ __launch_bounds__(256) void k_query_rows(const float *__restrict__ tris15, int n, QueryRow *__restrict__ rows,
                                                    uint32_t *__restrict__ scene_max)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t m[QMAX_WORDS] = { 0u, 0u, 0u, 0u };
    if (i < n) {
        const float *t = tris15 + (size_t)15 * i;
        const v3 v0 = ld3(t), v1 = ld3(t + 3), v2 = ld3(t + 6);
        const v3 e1 = sub3(v1, v0), e2 = sub3(v2, v0);             // :216-217
        const v3 e1e2 = cross3(e1, e2);                            // :225
        QueryRow r;
        r.a = make_float4(v0.x, v0.y, v0.z, e1.x);
        r.b = make_float4(e1.y, e1.z, e2.x, e2.y);
        r.c = make_float4(e2.z, e1e2.x, e1e2.y, e1e2.z);
        rows[i] = r;
        const v3 vec[QMAX_WORDS] = { v0, e1, e2, e1e2 };
#pragma unroll
        for (int k = 0; k < QMAX_WORDS; k++) {
            const uint32_t x = __float_as_uint(vec[k].x) & 0x7fffffffu, y = __float_as_uint(vec[k].y) & 0x7fffffffu,
                           z = __float_as_uint(vec[k].z) & 0x7fffffffu;
            m[k] = max(max(x, y), z);
        }
    }
#pragma unroll
    for (int k = 0; k < QMAX_WORDS; k++) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m[k] = max(m[k], (uint32_t)__shfl_xor((int)m[k], d));
        if ((threadIdx.x & 63) == 0 && m[k]) atomicMax(scene_max + k, m[k]);
    }
}

// Ray p of the P that lane t of block b owns: (b * P + p) * 256 + t; its incoming distance -- a lane without a ray carries a record
// nothing can replace --; and the write-back: a record nothing replaced is not written at all.
template <int P> __device__ __forceinline__ long long lane_ray(int p) { return ((long long)blockIdx.x * P + p) * 256 + threadIdx.x; }
// glm::cross for two rays per lane: x.y * y.z - y.y * x.z, ... (mirt_math.hpp: cross3), every operation packed.
__device__ __forceinline__ v3p cross3p(const v3p &x, const v3p &y)
{
    return V3P(x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y);
}

// The same for the two rays of a lane, packed FP32: each v_pk_* rounds its halves like the scalar instruction.
__device__ __forceinline__ TestDots2 ray_dots2(const RowVecs &r, const v3p &start, const v3p &nd, f2 *e1e2b)
{
    const v3p e1 = splat3(r.e1), e2 = splat3(r.e2), x = splat3(r.e1e2);
    // (b one half at a time: written as a packed subtraction of splat(v0) the compiler pairs the neighbouring words of the row's
    // 128-bit reads and realigns the odd pairs through 16 bytes of scratch; v_sub_f32 rounds like either half of v_pk_add_f32)
    v3p b;
    b.x = (f2){ start.x.x - r.v0.x, start.x.y - r.v0.x };
    b.y = (f2){ start.y.x - r.v0.y, start.y.y - r.v0.y };
    b.z = (f2){ start.z.x - r.v0.z, start.z.y - r.v0.z };
    const v3p be2 = cross3p(b, e2), e1b = cross3p(e1, b);
    *e1e2b = x.x * b.x + x.y * b.y + x.z * b.z;
    TestDots2 d;
    d.den = x.x * nd.x + x.y * nd.y + x.z * nd.z;
    d.pu = be2.x * nd.x + be2.y * nd.y + be2.z * nd.z;
    d.qv = e1b.x * nd.x + e1b.y * nd.y + e1b.z * nd.z;
    return d;
}

// ---- what the lane-per-ray sweeps (k_query_closest, k_query_occluded) share: a lane's P rays, one row against them ------------
//
// Lane t of block b owns rays (b * P + p) * 256 + t (a lane without a ray reads ray 0).  Ray p of the lane: its number, whether
// there is one, start, negD and whether it takes the exact path for every row (ray_exact_only, the header comment), into the
// kernel's own registers.  The kernels call this from the loop that sets up what is their own of ray p, and for P = 2 pack start
// and negD there as well, element by element into their own v3p: done through a reference in here, the same stores turn every
// packed multiply of the row test around and reschedule the loop.
template <int P>
__device__ __forceinline__ void load_lane_ray(const QueryFrame &q, bool scene_ok, int p, long long &ray, bool &ok, v3 &start, v3 &nd, bool &exact_only)
{
    ray = lane_ray<P>(p);
    ok = ray < q.nrays;
    const float *r = q.rays + (size_t)RAY_WORDS * (ok ? ray : 0);
    start = ld3(r);
    const v3 dir = ld3(r + 3);
    nd = neg3(dir);                                                // negD = -dir (:229); dir is used as given
    exact_only = ray_exact_only(scene_ok, start, dir);
}

// Row r against the lane's P rays: the dots, e1e2b and the filter's verdict of each -- packed for P = 2, ray by ray otherwise.
template <int P>
__device__ __forceinline__ void test_row(const RowVecs &r, const v3 (&start)[P], const v3 (&nd)[P], const v3p &startp, const v3p &ndp,
                                         TestDots (&d)[P], float (&e1e2b)[P], bool (&maybe)[P])
{
    if constexpr (P == 2) {
        f2 eb;
        const TestDots2 t = ray_dots2(r, startp, ndp, &eb);
        maybe_hit2(t, &maybe[0], &maybe[1]);
        d[0] = dots_half(t, 0); d[1] = dots_half(t, 1);
        e1e2b[0] = eb.x; e1e2b[1] = eb.y;
    } else {
#pragma unroll
        for (int p = 0; p < P; p++) {
            d[p] = ray_dots(r, start[p], nd[p], &e1e2b[p]);
            maybe[p] = maybe_hit(d[p]);
        }
    }
}

// ---- k_query_closest: one lane per P rays, every ray tests every triangle --------------------------------------------
//
// Workgroup = 256 lanes.  The rows are staged through LDS in chunks of RT_CHUNK_ROWS (48 KiB) and read as wave-uniform
// broadcasts, three ds_read_b128 per triangle shared by the lane's P rays.
// hits[ray] is the reference's in/out `closestIntersection`, updated sequentially in index order (closest_offer).
template <int P>
__global__ __launch_bounds__(256) void k_query_closest(const QueryFrame q)
{
    extern __shared__ __attribute__((aligned(16))) float4 s_rows[];
    const bool scene_ok = scene_rows_in_range(q);

    long long ray[P];
    bool ok[P], exact_only[P], replaced[P];
    v3 start[P], nd[P], pos[P];
    v3p startp, ndp;
    float best_d[P];
    int best_i[P];
#pragma unroll
    for (int p = 0; p < P; p++) {
        load_lane_ray<P>(q, scene_ok, p, ray[p], ok[p], start[p], nd[p], exact_only[p]);
        if constexpr (P == 2) {
            startp.x[p] = start[p].x; startp.y[p] = start[p].y; startp.z[p] = start[p].z;
            ndp.x[p] = nd[p].x; ndp.y[p] = nd[p].y; ndp.z[p] = nd[p].z;
        }
        best_d[p] = incoming_distance(q.hits, ray[p], ok[p]);
        best_i[p] = -1;
        pos[p] = V3(0.0f, 0.0f, 0.0f);
        replaced[p] = false;
    }

    for (int base = 0; base < q.n; base += RT_CHUNK_ROWS) {
        const int cnt = min(RT_CHUNK_ROWS, q.n - base);
        stage_rows(s_rows, q.rows + base, cnt);
#pragma unroll 2
        for (int j = 0; j < cnt; j++) {
            const RowVecs r = unpack_row(s_rows[3 * j], s_rows[3 * j + 1], s_rows[3 * j + 2]);
            TestDots d[P];
            float e1e2b[P];
            bool maybe[P];
            test_row<P>(r, start, nd, startp, ndp, d, e1e2b, maybe);
#pragma unroll
            for (int p = 0; p < P; p++) {
                if (maybe[p] || exact_only[p]) {
                    v3 hp;
                    float dist;
                    if (exact_hit_row(d[p], e1e2b[p], r, start[p], &hp, &dist)) closest_offer(best_d[p], best_i[p], pos[p], replaced[p], dist, base + j, hp);
                }
            }
        }
    }

#pragma unroll
    for (int p = 0; p < P; p++)
        if (ok[p] && replaced[p]) store_record(q.hits + (size_t)HIT_WORDS * ray[p], pos[p], __float_as_uint(best_d[p]), (uint32_t)best_i[p]);
}

template __global__ void k_query_closest<QUERY_P>(const QueryFrame);

// ---- k_query_closest_wave: one WAVE per ray, lanes over triangles ------------------------------------------------------
//
// For few rays against many triangles (a pick, a handful of probes) a lane per ray leaves the chip empty and walks the whole
// triangle list serially.  Here the 64 lanes of a wave stride over the rows (coalesced 48-byte rows from global memory), each
// keeps the best of its own triangles, and the wave reduces them with the packed min-t key (rt_common.hpp: wave_min_key); the
// lane that owns the winner broadcasts its hit point, as in k_rt_wave.
// The sequential rule in key form: the record only ever moves to a distance that is <= the incoming one, so the final record is
// the smallest accepted distance d with `incoming >= d` -- the latest index among equals -- or the incoming record when there is
// none.  Such d are >= 0 and not NaN (+inf only under an incoming +inf), so their bits order as unsigned integers; "no candidate"
// is the all-ones key, above every one of them.
constexpr unsigned long long QUERY_KEY_NONE = ~0ull;

__global__ __launch_bounds__(256) void k_query_closest_wave(const QueryFrame q)
{
    const int lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= q.nrays) return;                                    // (the whole wave)
    const float *rp = q.rays + (size_t)RAY_WORDS * ray;
    const v3 start = ld3(rp), dir = ld3(rp + 3);
    const v3 nd = neg3(dir);                                       // :229
    const bool exact_only = ray_exact_only(scene_rows_in_range(q), start, dir);
    uint32_t *h = q.hits + (size_t)HIT_WORDS * ray;
    const float incoming = __uint_as_float(h[3]);

    unsigned long long key = QUERY_KEY_NONE;
    v3 pos = V3(0.0f, 0.0f, 0.0f);
    for (int i = lane; i < q.n; i += 64) {
        const float4 *src = reinterpret_cast<const float4 *>(q.rows + i);
        const RowVecs r = unpack_row(src[0], src[1], src[2]);
        float e1e2b;
        const TestDots td = ray_dots(r, start, nd, &e1e2b);
        if (maybe_hit(td) || exact_only) {
            v3 hp;
            float dist;
            if (exact_hit_row(td, e1e2b, r, start, &hp, &dist) && incoming >= dist) {
                const unsigned long long k = min_t_key(dist, i);
                if (k < key) { key = k; pos = hp; }                // lane-local: smallest distance, then largest index
            }
        }
    }
    const unsigned long long best = wave_min_key(key);
    if (best == QUERY_KEY_NONE) return;                            // nothing replaces the record: all 20 bytes stay
    const int owner = __builtin_ctzll(__ballot(key == best) | (1ull << 63));
    pos.x = __shfl(pos.x, owner); pos.y = __shfl(pos.y, owner); pos.z = __shfl(pos.z, owner);
    if (lane != 0) return;
    store_record(h, pos, (uint32_t)(best >> 32), (uint32_t)min_t_index(best));
}

// ---- k_query_direct_light: DirectLight per hit record -----------------------------------------------------------------
//
// One lane per P records.  Per light position k (the lights, or their jittered soft-shadow positions): the light term
// (light_term, :294-304), then the shadow ray -- start = the light, dir = -rDir (:310) -- swept over light k's origin table
// (k_prep_origin: shadow rays DO share their origin), staged through LDS in chunks; a lane stops testing at its first
// occluder closer than 0.99 r (any-hit is exact: SURVEY A-5).  result += D per position, result2 += result after each
// light's samples (the reference's double count, :319-322), and the return value result2 * colour (:325-326).
// Filter range: the tables' rows are checked by k_prep_origin (f.unsafe, wave-uniform); rDir is a unit vector unless the
// record's position is not finite, which the lane checks per light (|rDir| components below MIRT_QUERY_DIR_MAX, false for NaN).
// A record whose index is outside [0, n) -- the reference would read outside `triangles` -- yields (0, 0, 0).
// NaN colours.  A record whose position is not finite, or is the light itself, shades to NaN (:294-304: inf * 0, 0 / 0), and the
// bits of a NaN are outside IEEE 754: the reference is an x86 program, whose invalid operations GENERATE the default NaN with the
// sign bit set (0xffc00000) and whose operations on a NaN operand hand that operand on, quieted, sign and payload as they came;
// what this hardware generates and what its negated operands do to a NaN's sign is its own affair.  So a NaN component is stored
// as the reference's: the record's first NaN coordinate, quieted, when the NaN came in with the position -- every later operation
// only hands it on --, the generated default otherwise (an infinite coordinate, a position equal to the light).  Light and triangle
// data are finite wherever a NaN could come from nowhere else (scene_finite, the lights' range; a NaN in them takes its own course).
__device__ __forceinline__ v3 reference_nan(v3 c, v3 pos)
{
    uint32_t q = 0xffc00000u;
    if (pos.z != pos.z) q = __float_as_uint(pos.z) | 0x00400000u;
    if (pos.y != pos.y) q = __float_as_uint(pos.y) | 0x00400000u;
    if (pos.x != pos.x) q = __float_as_uint(pos.x) | 0x00400000u;
    const float n = __uint_as_float(q);
    return V3(c.x != c.x ? n : c.x, c.y != c.y ? n : c.y, c.z != c.z ? n : c.z);
}

// Record `rec` as DirectLight reads it (record 0 for a lane without one): its position, its triangle's 15 words and unit normal,
// and whether it names a triangle of the scene at all (triangle 0's words are read where it does not).
__device__ __forceinline__ bool light_record(const QueryLightFrame &q, long long rec, bool ok, v3 *pos, const float **t, v3 *nDir)
{
    const uint32_t *h = q.hits + (size_t)HIT_WORDS * (ok ? rec : 0);
    *pos = V3(__uint_as_float(h[0]), __uint_as_float(h[1]), __uint_as_float(h[2]));
    const int idx = (int)h[4];
    const bool valid = ok && idx >= 0 && idx < q.f.n;
    *t = q.f.tris15 + (size_t)15 * (valid ? idx : 0);
    *nDir = normalize3(ld3(*t + 9));                               // glm::normalize(triangles[i.triangleIndex].normal) (:300)
    return valid;
}

// The accumulators of record `rec` between two passes of a call (light_passes.hpp): plane c of the carry at c * nhits.
__device__ __forceinline__ void carry_load(const QueryLightFrame &q, long long rec, v3 *result, v3 *result2)
{
    const float *c = q.carry + rec;
    const size_t n = (size_t)q.nhits;
    *result = V3(c[0], c[n], c[2 * n]);
    *result2 = V3(c[3 * n], c[4 * n], c[5 * n]);
}
__device__ __forceinline__ void carry_store(const QueryLightFrame &q, long long rec, v3 result, v3 result2)
{
    float *c = q.carry + rec;
    const size_t n = (size_t)q.nhits;
    c[0] = result.x; c[n] = result.y; c[2 * n] = result.z;
    c[3 * n] = result2.x; c[4 * n] = result2.y; c[5 * n] = result2.z;
}

// The position of record `rec` alone (record 0 for a lane without one): what a shadow decision depends on.  The index is not read.
__device__ __forceinline__ v3 record_position(const QueryLightFrame &q, long long rec, bool ok)
{
    const uint32_t *h = q.hits + (size_t)HIT_WORDS * (ok ? rec : 0);
    return V3(__uint_as_float(h[0]), __uint_as_float(h[1]), __uint_as_float(h[2]));
}

// CARRY: one pass of a call of several (light_passes.hpp) -- the accumulators come from the carry unless the pass is the first,
// result2 takes result where the GLOBAL position closes a light, and they go back raw unless the pass is the last.
// MASK: the shadow decisions themselves (mirt_shadow_mask*; light_mask.hpp) instead of the colours -- every record that exists
// casts its rays, whatever its index says (a lane is live for `ok`, not `valid`), collects one bit per position of the pass and
// stores them once, after the pass's last position.  The sweep and its arithmetic are the ones below, untouched; light_term is
// called for rDir and r (nothing else of it survives: no accumulators, no carry, no triangle colour).  STATS (MASK only, profiling
// on): the QSTAT_WORDS counters in q.stats -- shadow rays, the rows offered to them (all n each), the rows a lane tested while it
// was live, and no fallback: this IS the sweep.
template <int P, bool FILTER, bool CARRY = false, bool MASK = false, bool STATS = false>
__device__ __forceinline__ void direct_light_body(const QueryLightFrame &q, float4 *s_tab)
{
    static_assert(!(CARRY && MASK), "a mask carries nothing from pass to pass");
    static_assert(MASK || !STATS, "only the mask's sweep counts");
    unsigned long long n_rays = 0, n_tests = 0;
    const RtFrame &f = q.f;
    const int first = CARRY ? q.first : 0;
    long long rec[P];
    bool ok[P], valid[P];
    v3 pos[P], nDir[P], tcol[P], result[P], result2[P];
    uint32_t bits[P];
#pragma unroll
    for (int p = 0; p < P; p++) {
        rec[p] = lane_ray<P>(p);
        ok[p] = rec[p] < q.nhits;
        if constexpr (MASK) {
            pos[p] = record_position(q, rec[p], ok[p]);
            nDir[p] = V3(0.0f, 0.0f, 0.0f);
            valid[p] = ok[p];
            bits[p] = 0u;
        } else {
            const float *t;
            valid[p] = light_record(q, rec[p], ok[p], &pos[p], &t, &nDir[p]);
            tcol[p] = ld3(t + 12);
            result[p] = result2[p] = V3(0.0f, 0.0f, 0.0f);
            if (CARRY && ok[p] && !(q.pass_flags & LIGHT_PASS_FIRST)) carry_load(q, rec[p], &result[p], &result2[p]);
        }
    }

    for (int k = 0; k < f.nlights; k++) {
        const v3 L = ld3(f.lpos[k]);
        v3 D[P];
        RayDirs<P> rd;
        float thr[P];
        bool live[P], exact_only[P];
        bool any_live = false;
#pragma unroll
        for (int p = 0; p < P; p++) {
            float r;
            v3 rdp;
            D[p] = light_term(f, k, pos[p], nDir[p], &rdp, &r);
            rd.set(p, rdp);                                        // shadow ray: dir = -rDir, so negD = rDir (:310, :229)
            thr[p] = r * 0.99f;                                    // j.distance < r*0.99f (:313)
            live[p] = valid[p];
            exact_only[p] = !dir_in_filter_range(rdp);
            any_live |= live[p];
            if (STATS) n_rays += valid[p] ? 1u : 0u;
        }
        const OriginRow *tab = f.light_tab + (size_t)k * f.n;
        // every wave of the block takes part in the staging barriers; a wave with nothing left to test skips the inner loop
        for (int base = 0; base < f.n; base += RT_CHUNK_ROWS) {
            const int cnt = min(RT_CHUNK_ROWS, f.n - base);
            stage_rows(s_tab, tab + base, cnt);
            if (!__any(any_live)) continue;
#pragma unroll 2
            for (int j = 0; j < cnt; j++) {
                const float4 r0 = s_tab[3 * j], r1 = s_tab[3 * j + 1], r2 = s_tab[3 * j + 2];
                TestDots d[P];
                bool maybe[P];
                test_rays<P, FILTER>(r0, r1, r2, rd, d, maybe);
#pragma unroll
                for (int p = 0; p < P; p++) {
                    if (STATS) n_tests += live[p] ? 1u : 0u;
                    if (live[p] && (maybe[p] || exact_only[p])) {
                        v3 hp;
                        float dist;
                        if (exact_hit(d[p], r0.w, f.tris15 + (size_t)15 * (base + j), L, &hp, &dist))
                            if (dist < thr[p]) live[p] = false, D[p] = V3(0.0f, 0.0f, 0.0f);      // :313-314
                    }
                }
            }
            any_live = false;
#pragma unroll
            for (int p = 0; p < P; p++) any_live |= live[p];
        }
#pragma unroll
        for (int p = 0; p < P; p++) {
            if constexpr (MASK) {
                bits[p] |= (uint32_t)(valid[p] && !live[p]) << k;                          // the lane that executed :314
            } else {
                result[p] = add3(result[p], D[p]);                                             // :319
                if (light_pass_closes(first, k, f.samples)) result2[p] = add3(result2[p], result[p]);   // :322
            }
        }
    }

#pragma unroll
    for (int p = 0; p < P; p++) {
        if (!ok[p]) continue;
        if constexpr (MASK) {
            light_mask_store(q.mask, (size_t)q.nhits, (size_t)rec[p], q.first, f.nlights, bits[p]);
        } else {
            if (CARRY && !(q.pass_flags & LIGHT_PASS_LAST)) { carry_store(q, rec[p], result[p], result2[p]); continue; }
            st3(q.rgb + 3 * (size_t)rec[p], valid[p] ? reference_nan(mul3(result2[p], tcol[p]), pos[p]) : V3(0.0f, 0.0f, 0.0f));   // :325-326
        }
    }
    if (STATS) flush_query_stats(q.stats, n_rays, n_rays * (unsigned)f.n, n_tests, 0ull);
}

template <int P, bool CARRY, bool MASK, bool STATS>
__global__ __launch_bounds__(256) void k_query_direct_light(const QueryLightFrame q)
{
    extern __shared__ __attribute__((aligned(16))) float4 s_tab[];
    if (__builtin_amdgcn_readfirstlane(*q.f.unsafe) == 0u) direct_light_body<P, true, CARRY, MASK, STATS>(q, s_tab);
    else direct_light_body<P, false, CARRY, MASK, STATS>(q, s_tab);
}

template __global__ void k_query_direct_light<QUERY_P, false, false, false>(const QueryLightFrame);
template __global__ void k_query_direct_light<QUERY_P, true, false, false>(const QueryLightFrame);
template __global__ void k_query_direct_light<QUERY_P, false, true, false>(const QueryLightFrame);
template __global__ void k_query_direct_light<QUERY_P, false, true, true>(const QueryLightFrame);

// ---- k_query_direct_light_binned: DirectLight per hit record, every shadow ray through its light-cube bin ------------------
//
// A shadow ray of DirectLight starts at a light position whatever the record (:310), so the ray family of that position's cube
// -- negD = rDir ~ s e_k + u e_k1 + v e_k2 over six faces (rt_binned.hpp) -- holds the shadow ray of EVERY record: a triangle the
// reference's test accepts for rDir is on the list of rDir's bin, and of a list only the shells up to
// the one 0.99 r falls into can hold a row whose `near` bound is below 0.99 r (bin_shell_of is monotone).  Per row: skipped when
// its `near` is beyond 0.99 r; the filter; a certain hit (sure_hit) of a triangle no point of which is farther than 0.99 r
// (`far`, r2.w) occludes without the divisions; anything else is decided by exact_hit, the arithmetic of k_query_direct_light.
// Any-hit is exact (SURVEY A-5): which occluder ends a ray does not show in the result, only whether there is one.
//
// One lane per record.  Lists differ per lane, so nothing is staged: every lane reads its own rows from global memory, three
// 16-byte loads a row.  Records that neighbour each other in a G-buffer fall into the same or neighbouring bins, whose lanes
// then read the same 48 bytes in the same step -- one request to the cache -- and walk lists of similar length.  The walk is
// k_rt_trace2's: its state lives in plain integer registers, every step is straight-line code for every lane (row 0 is loaded
// where a lane has none left), and only the exact stage -- a few steps in a thousand -- sits in a divergent branch.
//
// What the bins do not cover.  The proof needs rDir to be a direction: finite, with its largest component near 1 (the margins
// of the edge functions scale with it, dmax = 2).  rDir = normalize(L - pos) is that unless pos is not finite (a NaN or an
// infinite component: NaN in rDir), lies so far out that |L - pos|^2 overflows (rDir = 0), or equals L up to underflow (0 / 0,
// or infinite components).  Such a lane (`formed` false, or r * 0.99 not finite) sweeps light k's whole origin table after the
// wave's walk, as brute_l does in k_rt_trace2 and with the loop body of k_query_direct_light, the per-ray exact-only override
// included -- it can only be set on such a lane: a formed rDir is below 1.5 per component, far inside MIRT_QUERY_DIR_MAX.  The
// scene's and the lights' range is the host's to check (query.cpp): outside it the call takes k_query_direct_light.
// The any-hit sweep of the lanes a cube's bins do not cover (`swept`; rare), called by the whole wave after its walk: the full
// origin table `tab` of the lane's start point S in index order, k_query_direct_light's loop body -- the filter with the per-ray
// exact-only override in front of exact_hit -- and a lane live until its first accepted dist < thr (:313-314); the wave leaves when
// none of its lanes is live.  Returns whether the lane found an occluder; *rows is the number of rows it tested while live, for the
// caller's statistics.
__device__ __forceinline__ bool sweep_any_hit(const OriginRow *tab, int n, const float *tris15, v3 S, v3 nd, float thr, bool swept, bool exact_only,
                                              unsigned *rows)
{
    bool live = swept;
    unsigned tested = 0u;
    for (int j = 0; j < n; j++) {
        if (!__any(live)) break;
        const float4 r0 = tab[j].r0, r1 = tab[j].r1, r2 = tab[j].r2;
        const TestDots td = test_dots(r0, r1, r2, nd);
        tested += live ? 1u : 0u;
        if (live && (maybe_hit(td) || exact_only)) {
            v3 hp;
            float dist;
            if (exact_hit(td, r0.w, tris15 + (size_t)15 * j, S, &hp, &dist))
                if (dist < thr) live = false;                                              // :313-314
        }
    }
    *rows = tested;
    return swept && !live;
}

// MASK (mirt_shadow_mask*): the decisions instead of the colours, as in direct_light_body -- a record's position alone is read, a
// lane is live for `ok`, `occluded` becomes bit k of the pass and the bits are stored once (light_mask.hpp).
template <int P, bool STATS, bool CARRY, bool MASK>
__global__ __launch_bounds__(256) void k_query_direct_light_binned(const QueryBinnedFrame b)
{
    static_assert(!(CARRY && MASK), "a mask carries nothing from pass to pass");
    const QueryLightFrame &q = b.q;
    const RtFrame &f = q.f;
    const int first = CARRY ? q.first : 0;                         // (CARRY: direct_light_body's comment)
    const CubeView &cv = b.cube;
    const float4 *rows4 = reinterpret_cast<const float4 *>(cv.light_rows);
    const uint32_t face_bins = (uint32_t)(cv.cube_bins * cv.cube_bins) * 6u;
    unsigned long long n_rays = 0, n_cand = 0, n_tests = 0, n_fall = 0;
#pragma unroll 1
    for (int p = 0; p < P; p++) {
        const long long rec = lane_ray<P>(p);
        const bool ok = rec < q.nhits;
        v3 pos, nDir = V3(0.0f, 0.0f, 0.0f);
        const float *t = nullptr;
        bool valid = ok;
        if constexpr (MASK) pos = record_position(q, rec, ok);
        else valid = light_record(q, rec, ok, &pos, &t, &nDir);
        v3 result = V3(0.0f, 0.0f, 0.0f), result2 = result;
        uint32_t bits = 0u;
        if (CARRY && ok && !(q.pass_flags & LIGHT_PASS_FIRST)) carry_load(q, rec, &result, &result2);
        bool fell = false;
        for (int k = 0; k < f.nlights; k++) {
            const v3 L = ld3(f.lpos[k]);
            v3 rd;
            float r;
            v3 D = light_term(f, k, pos, nDir, &rd, &r);
            const float thr = r * 0.99f;                           // j.distance < r*0.99f (:313)
            const float ax = fabsf(rd.x), ay = fabsf(rd.y), az = fabsf(rd.z);
            // (every comparison is false for NaN)
            const bool formed = ax <= 1.5f && ay <= 1.5f && az <= 1.5f && fmaxf(fmaxf(ax, ay), az) >= 0.5f && thr <= FLT_MAX;
            const bool binned = valid && formed, swept = valid && !formed;
            uint32_t e = 0u, end = 0u;
            if (binned) {
                const uint32_t bin = cube_bin_of(rd, (uint32_t)k * face_bins, cv.cube_bins);
                const BinFrameDesc *lf = cv.light_frames + 6 * k;
                const uint32_t key = bin * (uint32_t)cv.shells;
                e = cv.light_off[key];
                end = cv.light_off[key + bin_shell_of(thr, lf->shell_d0, lf->shell_iw, cv.shells) + 1u];
            }
            if (STATS) { n_rays += valid ? 1u : 0u; n_cand += end - e; }
            int occluded = 0;
            float4 c0, c1, c2;
            walk_row(rows4, e < end ? e : 0u, c0, c1, c2);
            for (;;) {
                const int act = (int)(e < end);
                if (!__any(act)) break;
                if (STATS) n_tests += (unsigned)act;
                const TestDots td = test_dots(c0, c1, c2, rd);     // negD = rDir (:310, :229)
                // a candidate none of whose points is closer to the light than 0.99 r cannot occlude (:313)
                const int pass = act & (int)!(c1.w > thr) & (int)maybe_hit(td);
                const int sure = pass & (int)(c2.w < thr) & (int)sure_hit(td, c0.w);
                int done = sure;
                if (pass & (sure ^ 1)) {
                    v3 hp;
                    float dist;
                    if (exact_hit(td, c0.w, f.tris15 + (size_t)15 * cv.light_tri[e], L, &hp, &dist)) done = (int)(dist < thr);   // :313
                }
                occluded |= done;
                walk_step(rows4, e, end, act & (done ^ 1) & (int)(e + 1u < end), c0, c1, c2);     // (done, or the list's end: the lane is through)
            }
            if (__any(swept)) {
                // the lanes the bins do not cover: light k's full origin table (sweep_any_hit)
                unsigned rows;
                occluded |= (int)sweep_any_hit(f.light_tab + (size_t)k * f.n, f.n, f.tris15, L, rd, thr, swept, !dir_in_filter_range(rd), &rows);
                if (STATS && swept) { n_cand += (unsigned)f.n; fell = true; }
                if (STATS) n_tests += rows;
            }
            if constexpr (MASK) {
                bits |= (uint32_t)occluded << k;                                           // the lane that would execute :314
                continue;
            }
            if (occluded) D = V3(0.0f, 0.0f, 0.0f);                                        // :314
            result = add3(result, D);                                                      // :319
            if (light_pass_closes(first, k, f.samples)) result2 = add3(result2, result);   // :322
        }
        if (STATS) n_fall += fell ? 1u : 0u;
        if constexpr (MASK) {
            if (ok) light_mask_store(q.mask, (size_t)q.nhits, (size_t)rec, q.first, f.nlights, bits);
            continue;
        }
        if (CARRY && !(q.pass_flags & LIGHT_PASS_LAST)) {
            if (ok) carry_store(q, rec, result, result2);
            continue;
        }
        if (ok) st3(q.rgb + 3 * (size_t)rec, valid ? reference_nan(mul3(result2, ld3(t + 12)), pos) : V3(0.0f, 0.0f, 0.0f));   // :325-326
    }
    if (STATS) flush_query_stats(b.stats, n_rays, n_cand, n_tests, n_fall);
}

template __global__ void k_query_direct_light_binned<QUERY_BIN_P, false, false, false>(const QueryBinnedFrame);
template __global__ void k_query_direct_light_binned<QUERY_BIN_P, true, false, false>(const QueryBinnedFrame);
template __global__ void k_query_direct_light_binned<QUERY_BIN_P, false, true, false>(const QueryBinnedFrame);
template __global__ void k_query_direct_light_binned<QUERY_BIN_P, true, true, false>(const QueryBinnedFrame);
template __global__ void k_query_direct_light_binned<QUERY_BIN_P, false, false, true>(const QueryBinnedFrame);
template __global__ void k_query_direct_light_binned<QUERY_BIN_P, true, false, true>(const QueryBinnedFrame);

// ---- k_query_relight: DirectLight with the shadow rays replaced by a mask's bits (mirt_direct_light_masked*) ------------------
//
// D = bit ? (0, 0, 0) : light_term per position, then DirectLight's own bookkeeping to the letter: result += D (:319), result2 +=
// result where the position closes a light (:322), result2 * colour (:325-326), reference_nan, and (0, 0, 0) for an index outside
// the scene.  Every operand is the one k_query_direct_light* has at that place and the additions run in the same order, so with the
// mask those kernels' MASK instantiations wrote the colours are theirs bit for bit; a prefix of the lights with the same `samples`
// reads a prefix of the planes.
// One lane per record and ONE launch for all of up to MIRT_MAX_LIGHT_POSITIONS positions: no ray is cast, so there is nothing to cut
// into passes and no carry.  The positions' lpos / lcol are a table in device memory (six floats a position) indexed by the loop
// counter alone -- wave-uniform, so they arrive by scalar loads; the record's words of the mask are read one plane at a time, the
// lanes of a wave reading neighbouring words.  light_term wants its RtFrame: position j is handed over as light 0 of a frame of
// which nothing else is read.  Traffic: 20 bytes of record, 4 per plane, 12 out and a gathered 60-byte triangle row per lane, which
// is the time for a few positions; from 32 positions on light_term's own arithmetic per position is.
__global__ __launch_bounds__(256) void k_query_relight(const QueryRelightFrame r)
{
    const QueryLightFrame &q = r.q;
    const long long rec = (long long)blockIdx.x * 256 + threadIdx.x;
    if (rec >= q.nhits) return;
    v3 pos, nDir;
    const float *t;
    const bool valid = light_record(q, rec, true, &pos, &t, &nDir);
    v3 result = V3(0.0f, 0.0f, 0.0f), result2 = result;
    RtFrame one;                                                   // (lpos[0] and lcol[0] are all light_term reads of it)
    for (int base = 0; base < r.npos; base += LIGHT_MASK_BITS) {
        const uint32_t m = q.mask[light_mask_index(base / LIGHT_MASK_BITS, (size_t)q.nhits, (size_t)rec)];
        const int cnt = min(LIGHT_MASK_BITS, r.npos - base);
        for (int k = 0; k < cnt; k++) {
            const float *l = r.lights + 6 * (size_t)(base + k);
            one.lpos[0][0] = l[0]; one.lpos[0][1] = l[1]; one.lpos[0][2] = l[2];
            one.lcol[0][0] = l[3]; one.lcol[0][1] = l[4]; one.lcol[0][2] = l[5];
            v3 rd;
            float rr;
            v3 D = light_term(one, 0, pos, nDir, &rd, &rr);
            if ((m >> k) & 1u) D = V3(0.0f, 0.0f, 0.0f);                                   // :314
            result = add3(result, D);                                                      // :319
            if (light_pass_closes(base, k, q.f.samples)) result2 = add3(result2, result);  // :322
        }
    }
    st3(q.rgb + 3 * (size_t)rec, valid ? reference_nan(mul3(result2, ld3(t + 12)), pos) : V3(0.0f, 0.0f, 0.0f));   // :325-326
}

// ---- k_query_fan: ClosestIntersection for many directions from one origin, every ray tests every triangle ------------------
//
// Rays of one origin share the per-origin hoist of the frame kernels (rt_common.hpp: OriginRow, 15 operations a test against the
// 41 of k_query_closest); the table is the query's own (k_prep_origin with first origin 1) or the cube's.  One lane per P rays,
// rows staged through LDS in chunks of RT_CHUNK_ROWS and read as wave-uniform broadcasts, the sweep written from the header
// primitives like k_query_direct_light's.  The record rule is k_query_closest's, sequentially in index order from the incoming
// record: `if (record.distance >= distance)` (:243).  The rows are inside the filter's range unless *unsafe says otherwise
// (k_prep_origin, or the host for a scene or origin beyond 1e8: every test through the exact divisions then); a ray with a
// |dir| component not below MIRT_QUERY_DIR_MAX -- NaN included -- has its verdicts overridden per ray.
template <int P, bool FILTER>
__device__ __forceinline__ void fan_body(const QueryFanFrame &q, float4 *s_tab)
{
    const v3 S = ld3(q.origin);
    long long ray[P];
    bool ok[P], exact_only[P], replaced[P];
    RayDirs<P> rd;
    v3 pos[P];
    float best_d[P];
    int best_i[P];
#pragma unroll
    for (int p = 0; p < P; p++) {
        ray[p] = lane_ray<P>(p);
        ok[p] = ray[p] < q.nrays;
        const v3 dir = ld3(q.dirs + 3 * (size_t)(ok[p] ? ray[p] : 0));
        rd.set(p, neg3(dir));                                      // negD = -dir (:229); dir is used as given
        exact_only[p] = !dir_in_filter_range(dir);
        best_d[p] = incoming_distance(q.hits, ray[p], ok[p]);
        best_i[p] = -1;
        pos[p] = V3(0.0f, 0.0f, 0.0f);
        replaced[p] = false;
    }
    for (int base = 0; base < q.n; base += RT_CHUNK_ROWS) {
        const int cnt = min(RT_CHUNK_ROWS, q.n - base);
        stage_rows(s_tab, q.tab + base, cnt);
#pragma unroll 2
        for (int j = 0; j < cnt; j++) {
            const float4 r0 = s_tab[3 * j], r1 = s_tab[3 * j + 1], r2 = s_tab[3 * j + 2];
            TestDots d[P];
            bool maybe[P];
            test_rays<P, FILTER>(r0, r1, r2, rd, d, maybe);
#pragma unroll
            for (int p = 0; p < P; p++) {
                if (maybe[p] || exact_only[p]) {
                    v3 hp;
                    float dist;
                    if (exact_hit(d[p], r0.w, q.tris15 + (size_t)15 * (base + j), S, &hp, &dist))
                        closest_offer(best_d[p], best_i[p], pos[p], replaced[p], dist, base + j, hp);
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < P; p++)
        if (ok[p] && replaced[p]) store_record(q.hits + (size_t)HIT_WORDS * ray[p], pos[p], __float_as_uint(best_d[p]), (uint32_t)best_i[p]);
}

template <int P>
__global__ __launch_bounds__(256) void k_query_fan(const QueryFanFrame q)
{
    extern __shared__ __attribute__((aligned(16))) float4 s_tab[];
    if (__builtin_amdgcn_readfirstlane(*q.unsafe) == 0u) fan_body<P, true>(q, s_tab);
    else fan_body<P, false>(q, s_tab);
}

template __global__ void k_query_fan<QUERY_P>(const QueryFanFrame);

// ---- k_query_fan_binned, k_query_fans_binned: the same, every ray through its bin of the cube around its origin -----------------
//
// The cube of a point (capi.hpp: LightCache, built by light_cache_ensure for a list of positions) holds every direction from it:
// a triangle the reference accepts for negD is on the list of the bin of d' = negD * 2^k (rt_query.hpp: fan_dir_of; DESIGN.md
// section 5.1).  A bin's list is ordered front to back in depth shells of the rows' `near` bound, and `near` bounds the distance
// the reference computes whatever the direction's length -- pos = v0 + u e1 + v e2 lies on the triangle --, so of a list only the
// shells up to the one the ray's current record distance (`bound`) falls into can hold a row with near <= bound (bin_shell_of is
// monotone), and every other row fails `bound >= d`.  The list ends there, and the end moves in with every replacement.
//
// Record rule.  The reference's loop moves the record only to distances <= the incoming one, ties to the later index, so its
// result is (smallest accepted d with incoming >= d, largest index among equals), or the incoming record when there is none:
// order-independent, which a walk in shell order needs.  Kept as running (bound, best_i): an accepted d replaces them when
// bound > d, or bound == d and its index is larger -- best_i = -1 stands for the incoming record, which so loses every tie.  A
// row is skipped only when near > bound, strictly: a row with d == bound has near <= bound and is tested.  An incoming distance
// that is negative or NaN is replaced by nothing (`>=` is false): the lane takes no list at all.
//
// One lane per ray, no LDS; the walk (fan_walk) is k_query_direct_light_binned's: state in plain integer registers, every step
// straight-line code (a lane with no row left loads row 0 and ignores it), verdicts as integers combined with `&`, only the exact
// stage in a divergent branch.  Lanes the bins do not cover (fan_dir_of: not formed) sweep their origin's full table after the
// wave's walk, with k_query_fan's loop body and per-ray override.
//
// Two entries call the one walk with the position k of the ray's origin in the cube, the origin S, the first bin of position k
// and its sweep table; the shell descriptor is light_frames[6 k].  k_query_fan_binned has one position, so all of these are
// launch-uniform: k and the bin base are literal 0 and S comes from the kernel's arguments.  k_query_fans_binned is one pass of
// mirt_intersect_fans* (rt_query.hpp: QueryFansFrame): the cube holds `count` of the call's origins as its positions, as
// DirectLight's cube holds the lights, and each lane takes k from origin_of, so lanes of a wave may hold different origins --
// their lists differ per lane anyway.  Each ray's argument is the single fan's, unchanged: position k of a many-position cube is
// built by the same kernels from the same descriptors as the one position of a fan's cube (fill_light_frames), only its keys
// start at k 6 B B shells.  A lane whose index lies outside [first, first + count) -- another pass's ray, or an index outside the
// call's list -- is not `mine`: it takes no list, sweeps nothing and writes nothing; it reads position 0's values so that every
// load stays inside the cube's tables.

// (the origin of a lane in one pass of a many-origin call -- FansLane, fans_lane: rt_query_device.hpp)

template <bool STATS>
__device__ __forceinline__ void fan_walk(const QueryFanFrame &q, long long ray, bool ok, bool mine, uint32_t k, v3 S, uint32_t bin_base,
                                         const OriginRow *tab)
{
    const CubeView &cv = q.cube;
    const float4 *rows4 = reinterpret_cast<const float4 *>(cv.light_rows);
    const v3 dir = ld3(q.dirs + 3 * (size_t)(ok ? ray : 0));
    const v3 nd = neg3(dir);                                       // negD = -dir (:229); dir is used as given
    uint32_t *h = q.hits + (size_t)HIT_WORDS * (ok ? ray : 0);
    float bound = __uint_as_float(h[3]);
    const bool open = mine && bound >= 0.0f;                       // (false for NaN)
    const FanDir fd = fan_dir_of(nd);
    const bool binned = open && fd.formed, swept = open && !fd.formed;
    const BinFrameDesc *lf = cv.light_frames + 6 * (size_t)k;
    const float d0 = lf->shell_d0, iw = lf->shell_iw;
    uint32_t e = 0u, end = 0u, key = 0u;
    if (binned) key = fan_list(cv, k, bin_base, fd.d, bound, &e, &end);
    unsigned long long n_cand = 0, n_tests = 0;
    int best_i = -1, replaced = 0;
    v3 pos = V3(0.0f, 0.0f, 0.0f);
    float4 c0, c1, c2;
    walk_row(rows4, e < end ? e : 0u, c0, c1, c2);
    for (;;) {
        const int act = (int)(e < end);
        if (!__any(act)) break;
        const TestDots td = test_dots(c0, c1, c2, nd);
        const int near_ok = act & (int)!(c1.w > bound);            // strictly beyond the record: cannot pass `bound >= d`
        if (STATS) { n_cand += (unsigned)act; n_tests += (unsigned)near_ok; }
        if (near_ok & (int)maybe_hit(td)) {
            const int tri = (int)cv.light_tri[e];
            v3 hp;
            float dist;
            if (exact_hit(td, c0.w, q.tris15 + (size_t)15 * tri, S, &hp, &dist)) {
                if ((bound > dist) | ((bound == dist) & (tri > best_i))) {
                    bound = dist; best_i = tri; pos = hp; replaced = 1;
                    end = min(end, cv.light_off[key + bin_shell_of(dist, d0, iw, cv.shells) + 1u]);
                }
            }
        }
        walk_step(rows4, e, end, act & (int)(e + 1u < end), c0, c1, c2);   // (the list's end, old or new: the lane is through)
    }
    if (__any(swept)) {
        // (rare) the lanes the bins do not cover: their origin's full table in index order, the sequential rule itself
        const bool exact_only = !dir_in_filter_range(dir);
        if (STATS && swept) { n_cand += (unsigned)q.n; n_tests += (unsigned)q.n; }
        for (int j = 0; j < q.n; j++) {
            const float4 r0 = tab[j].r0, r1 = tab[j].r1, r2 = tab[j].r2;
            const TestDots td = test_dots(r0, r1, r2, nd);
            if (swept && (maybe_hit(td) || exact_only)) {
                v3 hp;
                float dist;
                if (exact_hit(td, r0.w, q.tris15 + (size_t)15 * j, S, &hp, &dist)) closest_offer(bound, best_i, pos, replaced, dist, j, hp);
            }
        }
    }
    if (mine && replaced) store_record(h, pos, __float_as_uint(bound), (uint32_t)best_i);
    if (STATS) flush_query_stats(q.stats, mine ? 1u : 0u, n_cand, n_tests, swept ? 1u : 0u);
}

template <bool STATS>
__global__ __launch_bounds__(256) void k_query_fan_binned(const QueryFanFrame q)
{
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = ray < q.nrays;
    fan_walk<STATS>(q, ray, ok, ok, 0u, ld3(q.origin), 0u, q.tab);
}

template __global__ void k_query_fan_binned<false>(const QueryFanFrame);
template __global__ void k_query_fan_binned<true>(const QueryFanFrame);

template <bool STATS>
__global__ __launch_bounds__(256) void k_query_fans_binned(const QueryFansFrame qf)
{
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = ray < qf.f.nrays;
    const FansLane l = fans_lane(qf, ray, ok);
    fan_walk<STATS>(qf.f, ray, ok, l.mine, l.k, l.S, l.bin_base, l.tab);
}

template __global__ void k_query_fans_binned<false>(const QueryFansFrame);
template __global__ void k_query_fans_binned<true>(const QueryFansFrame);

// ---- k_query_fans_expand: the rays of a many-origin call written out for k_query_closest* ---------------------------------------
// One lane per ray: { origins[origin_of[i]], dirs[i] } as the caller gave them.  An index outside [0, norigins) reads no origin and
// becomes a ray that no triangle accepts, whatever the scene -- a NaN start makes every u, v and t of the accept test NaN, and
// ray_exact_only sends it past the filter --, so its record stays unwritten as in the binned kernel.
__global__ __launch_bounds__(256) void k_query_fans_expand(const QueryFansExpand x)
{
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    if (ray >= x.nrays) return;
    const uint32_t idx = x.origin_of ? (uint32_t)x.origin_of[ray] : 0u;
    const bool valid = idx < (uint32_t)x.norigins;
    const float qnan = __uint_as_float(0x7fc00000u);
    const v3 S = valid ? ld3(x.origins + 3 * (size_t)idx) : V3(qnan, qnan, qnan);
    const v3 d = valid ? ld3(x.dirs + 3 * (size_t)ray) : V3(0.0f, 0.0f, 0.0f);
    float *r = x.rays + (size_t)RAY_WORDS * ray;
    st3(r, S);
    st3(r + 3, d);
}

// ---- occlusion queries: "is anything in the way before distance L" (mirt_occluded*) ----------------------------------------------
//
// DirectLight's shadow decision (:306-315) for the caller's own ray and limit: occluded = some triangle ClosestIntersection accepts
// (:239) has distance < L, strictly (:313).  With a fresh record (distance FLT_MAX) the reference's two steps -- the closest hit,
// then `j.distance < L` -- give exactly that for every L, +inf included: a computed distance of +inf or NaN neither replaces the
// fresh record nor passes `<`.  Any-hit is exact (SURVEY A-5): which occluder settles a ray does not show in the byte, so a ray
// stops at its first one, in whatever order it meets the rows.  A limit nothing is below -- NaN, 0, negative -- settles its ray
// before any row is read (`L > 0` is false for NaN); a missing limit array stands for +inf.
// k_query_occluded: k_query_closest's sweep -- a lane per P rays (load_lane_ray), QueryRow chunks of RT_CHUNK_ROWS through LDS, the
// row test with the filter in front of the exact divisions (test_row) -- with a ray open until its first accepted dist < L.  A wave none of whose
// rays is open leaves the rows of a chunk alone (in steps of 64 rows: nothing in there waits for another wave), but goes on taking
// part in the staging barriers; the sweep itself ends when the WHOLE workgroup has no open ray, by a block-wide vote every one of
// the 256 lanes reaches at the top of each chunk -- stage_rows has two barriers, so no wave may leave that loop on its own.
template <int P>
__global__ __launch_bounds__(256) void k_query_occluded(const QueryOccludedFrame o)
{
    extern __shared__ __attribute__((aligned(16))) float4 s_rows[];
    const QueryFrame &q = o.q;
    const bool scene_ok = scene_rows_in_range(q);

    long long ray[P];
    bool ok[P], exact_only[P], open[P];
    v3 start[P], nd[P];
    v3p startp, ndp;
    float L[P];
#pragma unroll
    for (int p = 0; p < P; p++) {
        load_lane_ray<P>(q, scene_ok, p, ray[p], ok[p], start[p], nd[p], exact_only[p]);
        if constexpr (P == 2) {
            startp.x[p] = start[p].x; startp.y[p] = start[p].y; startp.z[p] = start[p].z;
            ndp.x[p] = nd[p].x; ndp.y[p] = nd[p].y; ndp.z[p] = nd[p].z;
        }
        L[p] = occlusion_limit(o.limit, ray[p], ok[p]);
        open[p] = L[p] > 0.0f;                                     // (false for NaN, and for a lane without a ray)
    }

    for (int base = 0; base < q.n; base += RT_CHUNK_ROWS) {
        bool any_open = false;
#pragma unroll
        for (int p = 0; p < P; p++) any_open |= open[p];
        if (!__syncthreads_or((int)any_open)) break;               // workgroup-uniform: every lane votes, every lane leaves
        const int cnt = min(RT_CHUNK_ROWS, q.n - base);
        stage_rows(s_rows, q.rows + base, cnt);
        for (int j0 = 0; j0 < cnt; j0 += 64) {
            if (!__any((int)any_open)) break;                      // (the wave only: no barrier between here and the chunk's end)
            const int j1 = min(j0 + 64, cnt);
#pragma unroll 2
            for (int j = j0; j < j1; j++) {
                const RowVecs r = unpack_row(s_rows[3 * j], s_rows[3 * j + 1], s_rows[3 * j + 2]);
                TestDots d[P];
                float e1e2b[P];
                bool maybe[P];
                test_row<P>(r, start, nd, startp, ndp, d, e1e2b, maybe);
#pragma unroll
                for (int p = 0; p < P; p++) {
                    if (open[p] && (maybe[p] || exact_only[p])) {
                        v3 hp;
                        float dist;
                        if (exact_hit_row(d[p], e1e2b[p], r, start[p], &hp, &dist))
                            if (dist < L[p]) open[p] = false;                              // :313
                    }
                }
            }
            any_open = false;
#pragma unroll
            for (int p = 0; p < P; p++) any_open |= open[p];
        }
    }

    // a ray is occluded exactly when it began open and was closed by a row
#pragma unroll
    for (int p = 0; p < P; p++)
        if (ok[p]) o.occluded[ray[p]] = (uint8_t)((L[p] > 0.0f) && !open[p]);
}

template __global__ void k_query_occluded<QUERY_P>(const QueryOccludedFrame);

// k_query_occluded_wave: one WAVE per ray, lanes over the rows as in k_query_closest_wave; the wave leaves the list at the first
// step in which any of its lanes found an occluder, and lane 0 stores the byte.  No barrier anywhere: a wave returns on its own.
constexpr int OCC_WAVE_ROWS = 4;                  // rows per lane and step: 256 rows of the list between two votes
__global__ __launch_bounds__(256) void k_query_occluded_wave(const QueryOccludedFrame o)
{
    const QueryFrame &q = o.q;
    const int lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= q.nrays) return;                                    // (the whole wave)
    const float *rp = q.rays + (size_t)RAY_WORDS * ray;
    const v3 start = ld3(rp), dir = ld3(rp + 3);
    const v3 nd = neg3(dir);                                       // :229
    const bool exact_only = ray_exact_only(scene_rows_in_range(q), start, dir);
    const float L = occlusion_limit(o.limit, ray, true);

    int occluded = 0;
    if (L > 0.0f) {                                                // (wave-uniform; false for NaN)
        // OCC_WAVE_ROWS rows a lane and step, all loaded before the first is tested (a lane past the table's end loads its last
        // row and ignores it), and one vote a step: a wave that meets no occluder pays one ballot per 256 rows
        for (int base = 0; base < q.n; base += 64 * OCC_WAVE_ROWS) {
            float4 a[OCC_WAVE_ROWS], b[OCC_WAVE_ROWS], c[OCC_WAVE_ROWS];
#pragma unroll
            for (int s = 0; s < OCC_WAVE_ROWS; s++) {
                const float4 *src = reinterpret_cast<const float4 *>(q.rows + min(base + 64 * s + lane, q.n - 1));
                a[s] = src[0]; b[s] = src[1]; c[s] = src[2];
            }
            bool found = false;
#pragma unroll
            for (int s = 0; s < OCC_WAVE_ROWS; s++) {
                const RowVecs r = unpack_row(a[s], b[s], c[s]);
                float e1e2b;
                const TestDots td = ray_dots(r, start, nd, &e1e2b);
                if (base + 64 * s + lane < q.n && (maybe_hit(td) || exact_only)) {
                    v3 hp;
                    float dist;
                    if (exact_hit_row(td, e1e2b, r, start, &hp, &dist) && dist < L) found = true;      // :313
                }
            }
            if (__any((int)found)) { occluded = 1; break; }
        }
    }
    if (lane == 0) o.occluded[ray] = (uint8_t)occluded;
}

// k_query_occluded_fans_binned: one pass of mirt_occluded_fans*, every ray through its bin of its origin's position in the cube.
//
// fan_walk's argument with the record distance fixed at L.  A row the reference accepts for negD is on the list of the bin of
// d' (fan_dir_of), and its `near` bounds the distance the reference computes: a row with d < L has near <= d < L, so it lies in a
// shell no later than bin_shell_of(L) (monotone) and passes `!(near > L)`.  The list therefore ends at L's shell, and that end never
// moves; a row is skipped when near > L; the lane is through at its first accepted dist < L.  What is conservative for the record
// rule's `>=` is conservative for `<`: every row that could occlude is on the part of the list that is walked.  No list for a limit
// that is NaN, 0 or negative.  Lanes whose direction fan_dir_of does not form sweep their origin's table, ending at the first occluder.
//
// A pass writes the bytes of its own rays only, each exactly once.  A ray whose index lies outside [0, norigins) belongs to no
// pass: the pass that starts at origin 0 writes its 0, and reads nothing for it but its index.
// STATS: rays of the pass, rows stepped over, those of them not beyond the limit, rays that swept.
template <bool STATS>
__global__ __launch_bounds__(256) void k_query_occluded_fans_binned(const QueryOccludedFansFrame of)
{
    const QueryFansFrame &qf = of.f;
    const QueryFanFrame &q = qf.f;
    const CubeView &cv = q.cube;
    const float4 *rows4 = reinterpret_cast<const float4 *>(cv.light_rows);
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = ray < q.nrays;
    const FansLane l = fans_lane(qf, ray, ok);
    const bool mine = l.mine, nobodys = ok && qf.first == 0 && l.idx >= (uint32_t)of.norigins;

    const v3 dir = ld3(q.dirs + 3 * (size_t)(ok ? ray : 0));
    const v3 nd = neg3(dir);                                       // negD = -dir (:229); dir is used as given
    const float L = occlusion_limit(of.limit, ray, ok);
    const bool open = mine && L > 0.0f;                            // (false for NaN)
    const FanDir fd = fan_dir_of(nd);
    const bool binned = open && fd.formed, swept = open && !fd.formed;
    uint32_t e = 0u, end = 0u;
    if (binned) fan_list(cv, l.k, l.bin_base, fd.d, L, &e, &end);
    unsigned long long n_cand = 0, n_tests = 0;
    int occluded = 0;
    float4 c0, c1, c2;
    walk_row(rows4, e < end ? e : 0u, c0, c1, c2);
    for (;;) {
        const int act = (int)(e < end);
        if (!__any(act)) break;
        const TestDots td = test_dots(c0, c1, c2, nd);
        const int near_ok = act & (int)!(c1.w > L);                // every point of the row is beyond the limit: cannot pass `<`
        if (STATS) { n_cand += (unsigned)act; n_tests += (unsigned)near_ok; }
        int done = 0;
        if (near_ok & (int)maybe_hit(td)) {
            v3 hp;
            float dist;
            if (exact_hit(td, c0.w, q.tris15 + (size_t)15 * cv.light_tri[e], l.S, &hp, &dist)) done = (int)(dist < L);    // :313
        }
        occluded |= done;
        walk_step(rows4, e, end, act & (done ^ 1) & (int)(e + 1u < end), c0, c1, c2);     // (done, or the list's end: the lane is through)
    }
    if (__any(swept)) {
        // the lanes the bins do not cover: their origin's full table, up to the first occluder (sweep_any_hit)
        unsigned rows;
        occluded |= (int)sweep_any_hit(l.tab, q.n, q.tris15, l.S, nd, L, swept, !dir_in_filter_range(dir), &rows);
        if (STATS) { n_cand += rows; n_tests += rows; }
    }
    if (mine || nobodys) of.occluded[ray] = (uint8_t)occluded;     // (nobodys: 0 -- such a lane is not open)
    if (STATS) flush_query_stats(q.stats, mine ? 1u : 0u, n_cand, n_tests, swept ? 1u : 0u);
}

template __global__ void k_query_occluded_fans_binned<false>(const QueryOccludedFansFrame);
template __global__ void k_query_occluded_fans_binned<true>(const QueryOccludedFansFrame);

}  // namespace mirt
