// query.cpp -- ray queries: ClosestIntersection and DirectLight for the caller's own rays and records (mirt_intersect*,
// mirt_direct_light*; the kernels: ../query/rt_query.hip).  The ray-independent rows of the scene are built once per scene
// version and shared by the streams, and so is the light cube whose bins the shadow rays of DirectLight walk (per scene version
// and light positions); a query takes the next stream as a frame does (mirt_set_frames_in_flight, mirt_sync) but leaves the
// statistics of the last render call alone (DirectLight has its own: mirt_set_query_mode, mirt_get_query_stats, defined here).
// DirectLight over more than MIRT_MAX_LIGHTS light positions runs in passes that hand its accumulators on (direct_light_passes; the
// deferred frames of rt_frame.cpp run the same passes over one record per pixel), each binned pass through a kept cube of its own.
// Many rays from ONE origin (mirt_intersect_from*) walk a cube of the same kind around that origin, kept apart from DirectLight's;
// rays from SEVERAL origins in one call (mirt_intersect_fans*) walk cubes that hold up to MIRT_MAX_LIGHTS of the origins each.
// Occlusion queries (mirt_occluded*, mirt_occluded_fans*) answer one byte per ray through the same rows and the same cubes.
// Shadow masks (mirt_shadow_mask*) are DirectLight's pass loop with its kernels' MASK instantiations -- the shadow decision per
// (record, position) instead of the colours --, and mirt_direct_light_masked* is DirectLight from those bits in one launch.
#include "capi.hpp"

namespace mirt {

// Which kernel answers mirt_intersect*: one wave per ray while the rays are at most MIRT_QUERY_WAVE_RAYS (0: never; a huge value:
// always), a lane per ray beyond.  A wave per ray finishes a ray's triangle list 64 lanes wide, so it is ahead until the lane-per-ray
// grid fills the chip too; both kernels walk the same list, so the triangle count hardly moves the crossing.  The default is the
// frame path's figure for its own wave kernel (rt_frame.cpp: at most 4096 rays); tools/ray_query_bench.py sweeps both kernels over
// 1 .. 2^20 rays and reports where the curves cross (profiles/ray_query_bench.txt).
constexpr long QUERY_WAVE_RAYS_DEFAULT = 4096;
long query_wave_rays()
{
    static const long v = env_int("MIRT_QUERY_WAVE_RAYS", QUERY_WAVE_RAYS_DEFAULT);
    return v;
}

// The rows of the current scene on the current stream: built here when the scene changed (mirt_scene_upload waited for every
// stream, so nothing still reads the old ones), otherwise this stream is ordered behind the build once, by its event.
int query_rows()
{
    int rc;
    QueryRows &Q = g.qrows;
    QueryScratch &S = g.cur().query;
    if (Q.version != g.scene_version) {
        Q.version = 0;
        if (Q.n != g.n && (rc = dev_grow(&Q.d_rows, &Q.n, g.n, (size_t)g.n, false))) return rc;
        if (!Q.d_max) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&Q.d_max), sizeof(uint32_t) * QMAX_WORDS));
        if (!Q.ev_built) HIP_TRY(hipEventCreateWithFlags(&Q.ev_built, hipEventDisableTiming));
        HIP_TRY(hipMemsetAsync(Q.d_max, 0, sizeof(uint32_t) * QMAX_WORDS, g.stream));
        hipLaunchKernelGGL(k_query_rows, dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, g.stream, g.d_tris, g.n, Q.d_rows, Q.d_max);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(Q.ev_built, g.stream));
        Q.version = g.scene_version;
        S.rows_seen = Q.version;
    } else if (S.rows_seen != Q.version) {
        HIP_TRY(hipStreamWaitEvent(g.stream, Q.ev_built, 0));
        S.rows_seen = Q.version;
    }
    return MIRT_OK;
}

static int check_query_args(const void *in, int count, const void *out, const char *what)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (count < 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "%s count %d is negative", what, count);
    if (count > 0 && (!in || !out)) return fail(MIRT_ERR_INVALID_ARGUMENT, "%s arrays must not be NULL when the count is > 0", what);
    return MIRT_OK;
}

// The arguments of a call from one origin alone, without a look at the library's state (order_fans.cpp checks them in front of it).
int from_args(const float *origin, const void *dirs3, int nrays, const void *hits)
{
    if (nrays < 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "direction count %d is negative", nrays);
    if (nrays > 0 && (!dirs3 || !hits)) return fail(MIRT_ERR_INVALID_ARGUMENT, "direction arrays must not be NULL when the count is > 0");
    if (nrays > 0 && !origin) return fail(MIRT_ERR_INVALID_ARGUMENT, "origin must not be NULL when the count is > 0");
    return MIRT_OK;
}

// ... of mirt_intersect_from*: check_query_args, then the origin (a call without rays needs none).
static int check_from_args(const float *origin, const void *dirs3, int nrays, const void *hits)
{
    int rc;
    if ((rc = check_query_args(dirs3, nrays, hits, "direction"))) return rc;
    if (nrays > 0 && !origin) return fail(MIRT_ERR_INVALID_ARGUMENT, "origin must not be NULL when the count is > 0");
    return MIRT_OK;
}

int query_need_scene()
{
    if (g.n <= 0) return fail(MIRT_ERR_NO_SCENE, "no scene uploaded (mirt_scene_upload)");
    return MIRT_OK;
}

// What the brute-force kernels read of the scene (query_rows) and of the caller: nrays rays and, for closest hits, their records.
QueryFrame rows_frame(const void *d_rays, int nrays, void *d_hits)
{
    QueryFrame q;
    q.rows = g.qrows.d_rows;
    q.n = g.n;
    q.scene_max = g.qrows.d_max;
    q.scene_finite = g.scene_finite ? 1 : 0;
    q.rays = static_cast<const float *>(d_rays);
    q.nrays = nrays;
    q.hits = static_cast<uint32_t *>(d_hits);
    return q;
}

// The kernel pair of a brute-force query over nrays > 0 rays on the current stream: a wave per ray up to query_wave_rays(), a lane
// per ray beyond.
template <class Frame>
static int launch_sweep(void (*wave)(Frame), void (*lane)(Frame), int nrays, const Frame &f)
{
    if ((long)nrays <= query_wave_rays()) {
        hipLaunchKernelGGL(wave, dim3((unsigned)((nrays + 3) / 4)), dim3(256), 0, g.stream, f);
    } else {
        hipLaunchKernelGGL(lane, dim3((unsigned)((nrays + QUERY_BLOCK_RAYS - 1) / QUERY_BLOCK_RAYS)), dim3(256), sweep_lds_bytes(), g.stream, f);
    }
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}

// ClosestIntersection by brute force for nrays > 0 rays on the current stream: the scene's rows, then one of the two kernels.
int intersect_launch(const void *d_rays, int nrays, void *d_hits)
{
    int rc;
    if ((rc = query_rows())) return rc;
    return launch_sweep(k_query_closest_wave, k_query_closest<QUERY_P>, nrays, rows_frame(d_rays, nrays, d_hits));
}

int query_intersect(const void *d_rays, int nrays, void *d_hits)
{
    int rc;
    if ((rc = check_query_args(d_rays, nrays, d_hits, "ray"))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    stream_begin();
    if (g.ray_grid) {                                        // mirt_set_ray_grid: through the cell grid whenever it can be built
        bool done = false;
        if ((rc = ray_grid_intersect(d_rays, nrays, d_hits, &done)) || done) return rc;
    }
    return intersect_launch(d_rays, nrays, d_hits);
}

// ---- what the queries that walk a cube share: its view, their statistics ------------------------------------------------------

// (the view of a cube's tables, cube_view: capi.hpp)

// A query of `kind` starts on the current stream: its statistics begin afresh.
QueryStats &stats_begin(int kind, bool binned)
{
    QueryStats &Q = g.qstats[kind];
    memset(&Q.s, 0, sizeof Q.s);
    Q.s.mode_used = binned ? MIRT_QUERY_BINNED : MIRT_QUERY_BRUTE;
    Q.stream = g.stream;
    Q.dev = nullptr;
    return Q;
}
// ... and the cube its walk takes, noted.
static void stats_cube(QueryStats &Q, const LightCache &C, int source)
{
    Q.s.cube_source = source;
    Q.s.cube_bins = C.cube_bins;
    Q.s.shells = C.shells;
}

// With profiling on, the stream's counters of `kind` zeroed on the stream and noted for query_get_stats: *counters is what the
// STATS instantiation of the walk kernel counts into, NULL says to launch the plain one.
int stats_arm(int kind, unsigned long long **counters)
{
    *counters = nullptr;
    if (!g.profiling) return MIRT_OK;
    unsigned long long *&d = g.cur().query.d_stats[kind];
    if (!d) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), sizeof(unsigned long long) * QSTAT_WORDS));
    HIP_TRY(hipMemsetAsync(d, 0, sizeof(unsigned long long) * QSTAT_WORDS, g.stream));
    g.qstats[kind].dev = *counters = d;
    return MIRT_OK;
}

// The STATS or the plain instantiation of a walk kernel over `f` on the current stream, as stats_arm decided.
template <class Frame>
static int launch_walk(void (*plain)(Frame), void (*counting)(Frame), bool stats, dim3 grid, const Frame &f)
{
    hipLaunchKernelGGL(stats ? counting : plain, grid, dim3(256), 0, g.stream, f);
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}

// Whether the scene and every one of the npos start points pos3 are inside the filter's proven range (rt_frame.cpp: operands_safe):
// what is not, is never binned, whatever the mode -- the frame path does not bin it either (rt_enqueue).
static bool starts_safe(const float *pos3, int npos)
{
    bool safe = g.scene_finite;
    for (int k = 0; k < npos; k++) safe = safe && start_in_filter_range(pos3 + 3 * (size_t)k);
    return safe;
}

// The cube a walk from the npos positions origins[3 ..] reads on a grid of cube_bins, and the cube_source that makes.  A cube
// somebody else holds for these very positions on this very grid comes first -- `foreign`, in the caller's order, each with its
// source code; read, never written, nor its owner's tracking --, else the caller's own.  held_cube builds nothing and answers
// with no cube when none is held (the `held` of AUTO); walk_cube builds the caller's own if need be, in the stream's LIGHT
// scratch set as the shared cube's build (the pass that set kept for moving lights is invalidated there).  An own cube that is
// held is returned without a call of light_cache_ensure: for a held cube that function returns at once, built = false, having
// touched nothing (binned.cpp) -- should it ever do more for a held cube, walk_cube has to call it in that case too.
// (struct CubeChoice: capi.hpp)
static CubeChoice held_cube(std::initializer_list<CubeChoice> foreign, const LightCache &own, const float *origins, int npos, int cube_bins)
{
    const uint64_t key = light_key_of(origins, npos);
    for (const CubeChoice &f : foreign)
        if (f.cube->holds(key, cube_bins)) return f;
    return CubeChoice{ own.holds(key, cube_bins) ? &own : nullptr, 2 };
}
static int walk_cube(std::initializer_list<CubeChoice> foreign, LightCache &own, const float *origins, int npos, int cube_bins, CubeChoice *out)
{
    int rc;
    *out = held_cube(foreign, own, origins, npos, cube_bins);
    if (out->cube) return MIRT_OK;
    bool built = false;
    if ((rc = light_cache_ensure(own, g.cur().lt, origins, npos, cube_bins, &built))) return rc;
    *out = CubeChoice{ &own, built ? 1 : 2 };
    return MIRT_OK;
}

// The cube list of a pass: row 0 is the camera's place (light_key_of, light_cache_ensure), rows 1 .. count the pass's origins
// (of a many-origin call) or light positions (of DirectLight).
static void fans_pass_origins(const float *origins3, const FanPass &p, float *po)
{
    po[0] = po[1] = po[2] = 0.0f;
    memcpy(po + 3, origins3 + 3 * (size_t)p.first, sizeof(float) * 3 * p.count);
}

// Whether every pass of `plan` over the call's positions origins3 finds its cube held -- the `held` of AUTO for a call in passes:
// pass i's own cube is own[i % QUERY_LIGHT_CUBES]; somebody else's may serve pass 0 (foreign0) and the later passes (foreign).
static bool passes_held(const std::vector<FanPass> &plan, const LightCache *own, std::initializer_list<CubeChoice> foreign0,
                        std::initializer_list<CubeChoice> foreign, const float *origins3)
{
    float po[(1 + MIRT_MAX_LIGHTS) * 3];
    for (size_t i = 0; i < plan.size(); i++) {
        fans_pass_origins(origins3, plan[i], po);
        if (!held_cube(i == 0 ? foreign0 : foreign, own[i % QueryRows::QUERY_LIGHT_CUBES], po, plan[i].count, plan[i].cube_bins).cube) return false;
    }
    return true;
}

int query_get_stats(int kind, mirt_query_stats *out)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (!out) return fail(MIRT_ERR_INVALID_ARGUMENT, "out must not be NULL");
    QueryStats &Q = g.qstats[kind];
    if (Q.stream) HIP_TRY(hipStreamSynchronize(Q.stream));
    if (Q.dev) {
        unsigned long long c[QSTAT_WORDS] = {};
        HIP_TRY(hipMemcpy(c, Q.dev, sizeof c, hipMemcpyDeviceToHost));
        Q.s.shadow_rays = c[QSTAT_SHADOW_RAYS];
        Q.s.candidates = c[QSTAT_CANDIDATES];
        Q.s.tests = c[QSTAT_TESTS];
        Q.s.fallback_records = c[QSTAT_FALLBACK];
        Q.dev = nullptr;                         // (read once: a later query of the kind on the stream zeroes the words again)
    }
    *out = Q.s;
    return MIRT_OK;
}

// ---- DirectLight: which kernel, which cube ----------------------------------------------------------------------------------

// AUTO bins under the frame path's own rule (rt_frame.cpp: mode_bins) with the query's shadow work in the place of the frame's
// pixels x triangles: a scene of MIRT_BIN_THRESHOLD triangles or more and records x light positions x triangles >= 4e7 -- below it
// the cube's build (a binning pass and a sort, with one host read-back) costs more than the sweep it saves.
// tools/ray_query_bench.py sweeps the record count for the crossing (profiles/ray_query_bench.txt).
static bool auto_bins(int nhits, int npos)
{
    return g.n >= auto_bin_threshold() && (long long)nhits * npos * g.n >= 40000000LL;
}

// Origin tables of the query's own for origins[3 ..] (npos positions) on the current stream, and their `unsafe` flag: k_prep_origin
// into the stream's frame tables would overwrite the camera rows a kept binning pass counts on (rt_frame.cpp: rt_dispatch_brute).
static int query_origin_tables(const float *origins, int npos, bool safe)
{
    int rc;
    QueryScratch &S = g.cur().query;
    if (npos > S.tab_lights || S.tab_n != g.n) {
        if ((rc = dev_grow(&S.d_light_tab, &S.tab_lights, npos, (size_t)npos * g.n, false))) return rc;
        S.tab_n = g.n;
    }
    if (!S.d_origins) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&S.d_origins), sizeof(float) * 3 * (1 + MIRT_MAX_LIGHTS)));
    if (!S.d_flags) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&S.d_flags), 16));
    const uint32_t flags_init[4] = { safe ? 0u : 1u, 0u, 0u, 0u };
    HIP_TRY(upload_small(S.d_flags, flags_init, sizeof flags_init, g.stream));
    if (npos > 0) {
        HIP_TRY(upload_small(S.d_origins, origins, sizeof(float) * 3 * (1 + npos), g.stream));
        // origins 1 .. npos only: the launch never touches a camera table
        hipLaunchKernelGGL(k_prep_origin, dim3((unsigned)((g.n + 255) / 256), (unsigned)npos), dim3(256), 0, g.stream,
                           g.d_tris, g.n, S.d_origins, V3(0.0f, 0.0f, 0.0f), 1, (OriginRow *)nullptr, S.d_light_tab, S.d_flags,
                           (unsigned long long *)nullptr, (uint32_t *)nullptr);
        HIP_TRY(hipGetLastError());
    }
    return MIRT_OK;
}

// The brute-force kernel over those tables; carry: one pass of several (light_passes.hpp).  With q.mask set the kernel is the MASK
// instantiation (a pass of mirt_shadow_mask*: no carry whatever the pass count), the counting one where stats_arm gave counters.
static int direct_light_brute(QueryLightFrame &q, const float *origins, int npos, bool safe, bool carry)
{
    int rc;
    if ((rc = query_origin_tables(origins, npos, safe))) return rc;
    q.f.light_tab = g.cur().query.d_light_tab;
    q.f.unsafe = g.cur().query.d_flags;
    void (*const kernel)(QueryLightFrame) = q.mask ? (q.stats ? k_query_direct_light<QUERY_P, false, true, true> : k_query_direct_light<QUERY_P, false, true, false>)
                                                   : (carry ? k_query_direct_light<QUERY_P, true> : k_query_direct_light<QUERY_P, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((q.nhits + QUERY_BLOCK_RAYS - 1) / QUERY_BLOCK_RAYS)), dim3(256), sweep_lds_bytes(), g.stream, q);
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}

// The binned kernel over the cube C (the frame path's, or the queries' own after light_cache_ensure); counters: what stats_arm
// gave the call, the same words for every pass of it.
static int direct_light_binned(QueryLightFrame &q, const LightCache &C, unsigned long long *counters, bool carry)
{
    QueryBinnedFrame b;
    memset(&b, 0, sizeof b);
    b.q = q;
    b.q.f.light_tab = C.d_light_tab;             // (the records the bins do not cover sweep the cube's own origin table)
    b.q.f.unsafe = nullptr;
    b.cube = cube_view(C);
    b.stats = counters;
    const dim3 grid((unsigned)((q.nhits + 256 * QUERY_BIN_P - 1) / (256 * QUERY_BIN_P)));
    if (q.mask) return launch_walk(k_query_direct_light_binned<QUERY_BIN_P, false, false, true>, k_query_direct_light_binned<QUERY_BIN_P, true, false, true>, counters != nullptr, grid, b);
    if (carry) return launch_walk(k_query_direct_light_binned<QUERY_BIN_P, false, true>, k_query_direct_light_binned<QUERY_BIN_P, true, true>, counters != nullptr, grid, b);
    return launch_walk(k_query_direct_light_binned<QUERY_BIN_P, false, false>, k_query_direct_light_binned<QUERY_BIN_P, true, false>, counters != nullptr, grid, b);
}

bool direct_light_auto_bins(int nhits, int npos) { return auto_bins(nhits, npos); }

static int fold_cube_source(size_t pass, int so_far, int source);

// DirectLight over npos positions in passes of at most MIRT_MAX_LIGHTS (light_passes.hpp has the argument).  Up to MIRT_MAX_LIGHTS
// positions are ONE pass on the kernels' plain instantiations, under the rules a query has always had; beyond, the ranges are
// fan_pass_plan's, walked strictly in order on the current stream, every pass with lpos / lcol, origin tables (brute) or cube
// (binned) of its own range and the carry between them.  Binned or brute is decided once, for the whole call: never what lies
// outside the filter's proven range (`safe`: that is the `unsafe` flag the brute kernel is given) or what the sort cannot key --
// one range that does not fit sends every pass to the brute-force kernel.  The cube of pass p: g.qrows.cubes[p % QUERY_LIGHT_CUBES];
// pass 0 reads the frame path's instead when that holds these very positions.
// d_mask (mirt_shadow_mask*): the same passes, plan, rules and cubes with the kernels' MASK instantiations, which write the shadow
// decisions of their range into the mask's planes and carry nothing; the statistics are the kind QUERY_SHADOW_MASK, counted by the
// sweep as well.  Without it every launch is the one this function has always made.
int direct_light_passes(const void *d_hits, int nhits, const mirt_light *lights, int npos, void *d_rgb, int mode, bool auto_rule, bool is_query,
                        float **carry, size_t *carry_cap, void *d_mask)
{
    int rc;
    QueryLightFrame q;
    memset(&q, 0, sizeof q);
    RtFrame &f = q.f;
    f.tris15 = g.d_tris;
    f.n = g.n;
    f.samples = soft_samples();
    q.hits = static_cast<const uint32_t *>(d_hits);
    q.nhits = nhits;
    q.rgb = static_cast<float *>(d_rgb);
    q.mask = static_cast<uint32_t *>(d_mask);
    const bool masking = d_mask != nullptr;
    const int kind = masking ? QUERY_SHADOW_MASK : QUERY_DIRECT_LIGHT;
    // the light positions the shadow rays start from and their share of the light's power, as a frame sets them up
    LightPositions lp;
    lp.origins[0] = lp.origins[1] = lp.origins[2] = 0.0f;
    fill_light_positions(lights, npos, lp.lpos, lp.lcol, lp.origins);
    const bool safe = starts_safe(lp.origins + 3, npos);     // the shadow rays' starts

    std::vector<FanPass> plan;
    bool may_bin;
    if (npos <= MIRT_MAX_LIGHTS) {
        bool fixed_grid = false;
        const int cube_bins = light_cube_bins_for(npos, &fixed_grid);
        plan.push_back({ 0, npos, cube_bins });
        may_bin = safe && npos > 0 && light_keys_fit(npos, cube_bins);
    } else {
        may_bin = fan_pass_plan(npos, g.n, cube_bins_override(), &plan) && safe;
        if (plan.empty())                                    // no cube takes them: the brute-force passes are full ones
            for (int first = 0; first < npos; first += MIRT_MAX_LIGHTS) plan.push_back({ first, std::min(npos - first, (int)MIRT_MAX_LIGHTS), 0 });
    }
    const size_t npass = plan.size();
    const std::initializer_list<CubeChoice> frame_cube = { { &g.lc, 3 } }, none = {};
    float po[(1 + MIRT_MAX_LIGHTS) * 3];
    // (`held`: every pass's cube, that is; a frame does not ask)
    const bool held = may_bin && is_query && passes_held(plan, g.qrows.cubes, frame_cube, none, lp.origins + 3);
    const bool binned = query_bins(may_bin, mode, held, auto_rule);

    if (is_query) stream_begin();
    QueryStats *stats = is_query ? &stats_begin(kind, binned) : nullptr;
    const bool multi = npass > 1 && !masking;
    if (multi && (size_t)nhits > *carry_cap && (rc = dev_grow(carry, carry_cap, (size_t)nhits, (size_t)nhits * LIGHT_CARRY_WORDS, true))) return rc;
    unsigned long long *counters = nullptr;
    if ((binned || masking) && is_query && (rc = stats_arm(kind, &counters))) return rc;     // (once: the passes' kernels add up in the same words)
    if (masking && !binned) q.stats = counters;
    int source_all = 0;
    for (size_t i = 0; i < npass; i++) {
        const FanPass &p = plan[i];
        f.nlights = p.count;
        memcpy(f.lpos, lp.lpos + p.first, sizeof(float) * 3 * p.count);
        memcpy(f.lcol, lp.lcol + p.first, sizeof(float) * 3 * p.count);
        q.first = p.first;
        q.carry = multi ? *carry : nullptr;
        q.pass_flags = (i == 0 ? LIGHT_PASS_FIRST : 0) | (i + 1 == npass ? LIGHT_PASS_LAST : 0);
        fans_pass_origins(lp.origins + 3, p, po);
        if (!binned) {
            if ((rc = direct_light_brute(q, po, p.count, safe, multi))) return rc;
            continue;
        }
        const std::initializer_list<CubeChoice> &foreign = i == 0 ? frame_cube : none;
        LightCache &own = g.qrows.cubes[i % QueryRows::QUERY_LIGHT_CUBES];
        CubeChoice c = held_cube(foreign, own, po, p.count, p.cube_bins);
        if (!c.cube) {                                       // (a build: behind the previous pass's kernel on this stream)
            if (!is_query && !g.cur().ev_used[MIRT_K_BIN]) k_begin(MIRT_K_BIN);
            if ((rc = walk_cube(foreign, own, po, p.count, p.cube_bins, &c))) return rc;
            if (!is_query) k_end(MIRT_K_BIN);
        }
        source_all = fold_cube_source(i, source_all, c.source);
        if (stats) stats_cube(*stats, *c.cube, source_all);
        if ((rc = direct_light_binned(q, *c.cube, counters, multi))) return rc;
    }
    return MIRT_OK;
}

int query_direct_light(const void *d_hits, int nhits, const mirt_light *lights, int nlights, void *d_rgb)
{
    int rc, npos = 0;
    if ((rc = check_query_args(d_hits, nhits, d_rgb, "hit"))) return rc;
    if ((rc = check_lights(lights, nlights, &npos))) return rc;
    if (nhits == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    QueryScratch &S = g.streams[next_si()].query;            // the stream the call will take: its carry
    return direct_light_passes(d_hits, nhits, lights, npos, d_rgb, g.query_mode, auto_bins(nhits, npos), true, &S.d_carry, &S.carry_cap);
}

// ---- shadow masks: DirectLight's shadow decisions per (record, position), and DirectLight from them (mirt_shadow_mask*,
// mirt_direct_light_masked*) ------------------------------------------------------------------------------------------------------
//
// The mask call IS mirt_direct_light's pass loop with the kernels' MASK instantiations (direct_light_passes): the same plan, the same
// binned-or-brute decision from the same rule (auto_bins over records x positions), the same kept cubes g.qrows.cubes[] and the frame
// path's cube in pass 0, so a cube either call built serves the other.  AUTO keeps mirt_direct_light's rule: tools/ray_query_bench.py
// --steps mask measures both calls beside mirt_direct_light_device (profiles/ray_query_bench.txt, section `mask`).
// The masked call casts no ray: one launch of k_query_relight over all positions, whose lpos / lcol travel as one table into the
// stream's query scratch.  It builds no cube, keeps no statistics and does not look at the query mode.

// The checks both calls share, in mirt_direct_light's order; *npos: the call's light positions.  `mask` may be NULL only where the
// call has no word to read or write (no record or no position).
static int check_mask_args(const void *hits, int nhits, const mirt_light *lights, int nlights, const void *mask, const void *out, int *npos)
{
    int rc;
    if ((rc = check_query_args(hits, nhits, out, "hit"))) return rc;
    if ((rc = check_lights(lights, nlights, npos))) return rc;
    if (nhits > 0 && *npos > 0 && !mask) return fail(MIRT_ERR_INVALID_ARGUMENT, "the mask must not be NULL for %d records and %d light positions", nhits, *npos);
    return MIRT_OK;
}

int query_shadow_mask(const void *d_hits, int nhits, const mirt_light *lights, int nlights, void *d_mask)
{
    int rc, npos = 0;
    if ((rc = check_mask_args(d_hits, nhits, lights, nlights, d_mask, d_hits, &npos))) return rc;
    if (nhits == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    if (npos == 0) return MIRT_OK;                           // no plane: nothing is written
    return direct_light_passes(d_hits, nhits, lights, npos, nullptr, g.query_mode, auto_bins(nhits, npos), true, nullptr, nullptr, d_mask);
}

int query_direct_light_masked(const void *d_hits, int nhits, const mirt_light *lights, int nlights, const void *d_mask, void *d_rgb)
{
    int rc, npos = 0;
    if ((rc = check_mask_args(d_hits, nhits, lights, nlights, d_mask, d_rgb, &npos))) return rc;
    if (nhits == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;

    QueryRelightFrame r;
    memset(&r, 0, sizeof r);
    r.q.f.tris15 = g.d_tris;
    r.q.f.n = g.n;
    r.q.f.samples = soft_samples();
    r.q.hits = static_cast<const uint32_t *>(d_hits);
    r.q.nhits = nhits;
    r.q.rgb = static_cast<float *>(d_rgb);
    r.q.mask = static_cast<uint32_t *>(const_cast<void *>(d_mask));      // (read only: k_query_relight)
    r.npos = npos;
    // position, then share of the light's power, six floats a position: what a pass of DirectLight has in f.lpos / f.lcol
    LightPositions lp;
    fill_light_positions(lights, npos, lp.lpos, lp.lcol, nullptr);
    float table[MIRT_MAX_LIGHT_POSITIONS * 6];
    for (int j = 0; j < npos; j++) {
        memcpy(table + 6 * j, lp.lpos[j], 12);
        memcpy(table + 6 * j + 3, lp.lcol[j], 12);
    }

    stream_begin();
    QueryScratch &S = g.cur().query;
    if (!S.d_relight) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&S.d_relight), sizeof table));
    if (npos > 0) HIP_TRY(upload_small(S.d_relight, table, sizeof(float) * 6 * npos, g.stream));
    r.lights = S.d_relight;
    hipLaunchKernelGGL(k_query_relight, dim3((unsigned)((nhits + 255) / 256)), dim3(256), 0, g.stream, r);
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}

// ---- origin fans: ClosestIntersection for many directions from one origin (mirt_intersect_from*) -----------------------------

// AUTO for a fan.  Measured (tools/ray_query_bench.py --steps fan, profiles/ray_query_bench.txt; soup scenes, the rays of a 1080p
// frame in shuffled order, 1 .. 2^20 rays): at n = 2 000 and at n = 100 000 the binned call WITH its cube's build (0.13 / 0.26 ms at
// few rays) is ahead of the sweep (0.34 / 16 ms: one lane walks the whole table) from a single ray on, so from FAN_AUTO_TRIANGLES
// triangles on AUTO bins whatever the ray count.  Below that the sweep was not measured -- its table is short, the build's fixed
// cost is not -- and the frame path's rule stays, with rays x triangles in the place of pixels x triangles: a scene of
// MIRT_BIN_THRESHOLD triangles or more and rays x triangles >= 4e7, UNMEASURED for this use.
constexpr int FAN_AUTO_TRIANGLES = 2000;
static bool auto_bins_fan(int nrays)
{
    return g.n >= auto_bin_threshold() && (g.n >= FAN_AUTO_TRIANGLES || (long long)nrays * g.n >= 40000000LL);
}

// What the frames of both fan calls share: the scene, the caller's directions and records; everything else zero.
QueryFanFrame fan_frame(const void *d_dirs3, int nrays, void *d_hits)
{
    QueryFanFrame q;
    memset(&q, 0, sizeof q);
    q.tris15 = g.d_tris;
    q.n = g.n;
    q.dirs = static_cast<const float *>(d_dirs3);
    q.nrays = nrays;
    q.hits = static_cast<uint32_t *>(d_hits);
    return q;
}

// What a call from one origin does up to its kernel on the stream it takes (mirt_intersect_from*, and order_fans.cpp's ordered form):
// binned or brute, as a DirectLight query decides it -- the cube is the fans' own, whoever else holds one for this point --, the
// statistics of QUERY_FAN begun afresh, and for a binned call the cube, built if need be, its view and table in *frame and the
// counters armed.  *frame is fan_frame's with the origin; a call that does not bin gets nothing more.
int fan_begin(const float *origin, const void *d_dirs3, int nrays, void *d_hits, QueryFanFrame *frame, bool *binned)
{
    int rc;
    QueryFanFrame &q = *frame;
    q = fan_frame(d_dirs3, nrays, d_hits);
    memcpy(q.origin, origin, 12);
    float origins[6] = {};
    memcpy(origins + 3, origin, 12);
    const bool safe = starts_safe(origin, 1);

    bool fixed_grid = false;
    const int cube_bins = light_cube_bins_for(1, &fixed_grid);
    const bool may_bin = safe && light_keys_fit(1, cube_bins);
    const bool held = may_bin && held_cube({}, g.qrows.fan, origins, 1, cube_bins).cube != nullptr;
    *binned = query_bins(may_bin, g.query_mode, held, auto_bins_fan(nrays));

    stream_begin();
    QueryStats &stats = stats_begin(QUERY_FAN, *binned);
    if (!*binned) return MIRT_OK;

    CubeChoice c;
    if ((rc = walk_cube({}, g.qrows.fan, origins, 1, cube_bins, &c))) return rc;
    stats_cube(stats, *c.cube, c.source);
    q.tab = c.cube->d_light_tab;
    q.cube = cube_view(*c.cube);
    return stats_arm(QUERY_FAN, &q.stats);
}

int query_intersect_from(const float *origin, const void *d_dirs3, int nrays, void *d_hits)
{
    int rc;
    if ((rc = check_from_args(origin, d_dirs3, nrays, d_hits))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;

    QueryFanFrame q;
    bool binned = false;
    if ((rc = fan_begin(origin, d_dirs3, nrays, d_hits, &q, &binned))) return rc;
    if (!binned) {
        QueryScratch &S = g.cur().query;
        float origins[6] = {};
        memcpy(origins + 3, origin, 12);
        if ((rc = query_origin_tables(origins, 1, starts_safe(origin, 1)))) return rc;
        q.tab = S.d_light_tab;
        q.unsafe = S.d_flags;
        hipLaunchKernelGGL(k_query_fan<QUERY_P>, dim3((unsigned)((nrays + QUERY_BLOCK_RAYS - 1) / QUERY_BLOCK_RAYS)), dim3(256), sweep_lds_bytes(), g.stream, q);
        HIP_TRY(hipGetLastError());
        return MIRT_OK;
    }
    return launch_walk(k_query_fan_binned<false>, k_query_fan_binned<true>, q.stats != nullptr, dim3((unsigned)((nrays + 255) / 256)), q);
}

// The primary sub-rays of a supersampled frame that shades each record once are such a fan from the camera (rt_frame.cpp,
// ../lights/aa_many_lights.hip): binned or swept as the single fan decides it, with the FRAME's mode in the place of
// mirt_set_query_mode and the frame's sub-ray count in AUTO's rule; the cube is the frames' own (g.qrows.aa_cam).
int aa_camera_cube(const float *cam, int mode, long long subrays, const LightCache **cube)
{
    int rc;
    *cube = nullptr;
    float origins[6] = {};
    memcpy(origins + 3, cam, 12);
    bool fixed_grid = false;
    const int cube_bins = light_cube_bins_for(1, &fixed_grid);
    const bool may_bin = starts_safe(cam, 1) && light_keys_fit(1, cube_bins);
    const bool held = may_bin && held_cube({}, g.qrows.aa_cam, origins, 1, cube_bins).cube != nullptr;
    const int qmode = mode == MIRT_RT_BRUTE ? MIRT_QUERY_BRUTE : (mode == MIRT_RT_BINNED ? MIRT_QUERY_BINNED : MIRT_QUERY_AUTO);
    const bool auto_rule = g.n >= auto_bin_threshold() && (g.n >= FAN_AUTO_TRIANGLES || subrays * g.n >= 40000000LL);   // (auto_bins_fan)
    if (!query_bins(may_bin, qmode, held, auto_rule)) return MIRT_OK;
    CubeChoice c = held_cube({}, g.qrows.aa_cam, origins, 1, cube_bins);
    if (!c.cube) {                                           // (a build: the frame's binning step, as a deferred frame's light cubes)
        if (!g.cur().ev_used[MIRT_K_BIN]) k_begin(MIRT_K_BIN);
        if ((rc = walk_cube({}, g.qrows.aa_cam, origins, 1, cube_bins, &c))) return rc;
        k_end(MIRT_K_BIN);
    }
    *cube = c.cube;
    return MIRT_OK;
}

// ---- origin fans from many origins in one call (mirt_intersect_fans*) ----------------------------------------------------------
//
// The call's origins go into cubes of up to MIRT_MAX_LIGHTS positions each, as the lights of a DirectLight query do, in passes over
// consecutive ranges of the list (cube_plan.hpp: fan_pass_plan); every pass launches k_query_fans_binned over ALL rays, and a lane
// whose origin lies outside the pass's range retires after reading its index.  Every ray belongs to exactly one pass, so records
// never meet; no pass is skipped, because which origins the rays name is device data.  The cube of a pass: the frame path's (g.lc)
// or DirectLight's (g.qrows.cube) when it holds these very positions on this very grid -- read, never written, nor their tracking
// --, else the call's own (pass p: g.qrows.fans[p % QUERY_LIGHT_CUBES]), built now if need be in the stream's LIGHT scratch set; a
// call of up to QUERY_LIGHT_CUBES passes finds every cube held when it is repeated.

// AUTO for a many-origin call: the single fan's rule (auto_bins_fan), which is MEASURED FOR ONE ORIGIN ONLY, and one condition more
// that tools/ray_query_bench.py --steps fans showed (profiles/ray_query_bench.txt, section `fans`; K = 1 .. 128 origins, soup100k and
// the soup of 2000).  This call's brute path is mirt_intersect's, not the fan's sweep: up to MIRT_QUERY_WAVE_RAYS rays it answers a
// wave per ray, and in every cell of at most 4096 rays it was ahead of binning with the builds (n = 2000: 0.03 ms against 0.32 ..
// 0.54 ms; n = 100 000: 0.6 ms against 0.83 .. 2.4 ms).  Beyond that many rays binning with its builds was ahead in every cell at n =
// 100 000 (9 .. 11 ms against 22 .. 681 ms) and in all but two at n = 2000 -- 4 origins x 4096 rays (0.60 against 0.53 ms) and
// 128 origins x 64 rays (four builds: 1.30 against 0.53 ms) --, where AUTO stays behind brute force.
bool auto_bins_fans(int nrays)
{
    return auto_bins_fan(nrays) && (long)nrays > query_wave_rays();
}

// The arguments of a many-origin call alone (order_fans.cpp checks them in front of the library's state), and with that state first
// as the fan calls themselves check them.
int fans_args(const float *origins3, int norigins, const void *origin_of, const void *dirs3, int nrays, const void *hits)
{
    if (norigins < 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "origin count %d is negative", norigins);
    if (nrays < 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "direction count %d is negative", nrays);
    if (nrays > 0 && (!dirs3 || !hits)) return fail(MIRT_ERR_INVALID_ARGUMENT, "direction arrays must not be NULL when the count is > 0");
    if (norigins > 0 && !origins3) return fail(MIRT_ERR_INVALID_ARGUMENT, "origins must not be NULL when their count is > 0");
    if (norigins == 0 && nrays > 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "%d rays but no origin", nrays);
    if (norigins > 1 && !origin_of) return fail(MIRT_ERR_INVALID_ARGUMENT, "origin_of may be NULL only for a single origin, not for %d", norigins);
    return MIRT_OK;
}
static int check_fans_args(const float *origins3, int norigins, const void *origin_of, const void *dirs3, int nrays, const void *hits)
{
    int rc;
    if ((rc = need_init())) return rc;
    return fans_args(origins3, norigins, origin_of, dirs3, nrays, hits);
}

// By definition the call is mirt_intersect on the expanded rays: they are written out on the device (k_query_fans_expand) into
// the stream's query scratch (fans_expand) and go through query_intersect's kernels, whose per-ray filter safety and choice of
// kernel come along.
int fans_expand(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays)
{
    int rc;
    QueryScratch &S = g.cur().query;
    if ((size_t)norigins > S.fan_origins_cap && (rc = dev_grow(&S.d_fan_origins, &S.fan_origins_cap, (size_t)norigins, (size_t)norigins * 3, false))) return rc;
    if ((size_t)nrays > S.fan_rays_cap && (rc = dev_grow(&S.d_fan_rays, &S.fan_rays_cap, (size_t)nrays, (size_t)nrays * RAY_WORDS, false))) return rc;
    HIP_TRY(upload_small(S.d_fan_origins, origins3, sizeof(float) * 3 * (size_t)norigins, g.stream));
    QueryFansExpand x;
    x.origins = S.d_fan_origins;
    x.norigins = norigins;
    x.origin_of = static_cast<const int32_t *>(d_origin_of);
    x.dirs = static_cast<const float *>(d_dirs3);
    x.nrays = nrays;
    x.rays = S.d_fan_rays;
    hipLaunchKernelGGL(k_query_fans_expand, dim3((unsigned)((nrays + 255) / 256)), dim3(256), 0, g.stream, x);
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}
static int fans_brute(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays, void *d_hits)
{
    int rc;
    if ((rc = fans_expand(origins3, norigins, d_origin_of, d_dirs3, nrays))) return rc;
    return intersect_launch(g.cur().query.d_fan_rays, nrays, d_hits);
}

// Binned or brute for a many-origin call, and the pass plan of a binned one.  As the single fan decides it: never what the frame
// path would not bin, whatever the mode -- and the call is one: an origin outside the filter's range (NaN included) among ordinary
// ones sends all of it to the brute-force kernels.  `held`: every pass's cube, that is.
bool fans_binned(const float *origins3, int norigins, int nrays, std::initializer_list<CubeChoice> foreign, std::vector<FanPass> *plan)
{
    const bool may_bin = starts_safe(origins3, norigins) && fan_pass_plan(norigins, g.n, cube_bins_override(), plan);
    const bool held = may_bin && passes_held(*plan, g.qrows.fans, foreign, foreign, origins3);
    return query_bins(may_bin, g.query_mode, held, auto_bins_fans(nrays));
}

// What every pass of a call read, folded over the passes: 1 as soon as a pass built; else what every pass read when that is one
// kind of cube; else 2: all were held.
static int fold_cube_source(size_t pass, int so_far, int source)
{
    return pass == 0 ? source : (so_far == 1 || source == 1 ? 1 : (so_far == source ? source : 2));
}

// The passes of a binned many-origin call on the current stream, in the plan's order: the pass's origins, the cube its walk reads
// (a build: behind the previous pass's kernel on this stream), what the call's statistics say of the cubes so far, the pass's fields
// of the caller's frame -- q is that frame's QueryFansFrame --, then the caller's launch of its walk kernel over the frame.
template <class Launch>
static int fans_passes(const float *origins3, const std::vector<FanPass> &plan, std::initializer_list<CubeChoice> foreign, QueryStats &stats,
                       QueryFansFrame &q, Launch launch)
{
    int rc;
    float po[(1 + MIRT_MAX_LIGHTS) * 3];
    int source_all = 0;
    for (size_t i = 0; i < plan.size(); i++) {
        const FanPass &p = plan[i];
        fans_pass_origins(origins3, p, po);
        CubeChoice c;
        if ((rc = walk_cube(foreign, g.qrows.fans[i % QueryRows::QUERY_LIGHT_CUBES], po, p.count, p.cube_bins, &c))) return rc;
        source_all = fold_cube_source(i, source_all, c.source);
        stats_cube(stats, *c.cube, source_all);
        q.f.tab = c.cube->d_light_tab;
        q.f.cube = cube_view(*c.cube);
        q.origins = c.cube->d_origins;
        q.first = p.first;
        q.count = p.count;
        if ((rc = launch())) return rc;
    }
    return MIRT_OK;
}

int fans_passes_run(const float *origins3, const std::vector<FanPass> &plan, std::initializer_list<CubeChoice> foreign, QueryStats &stats,
                    QueryFansFrame &q, const std::function<int()> &launch)
{
    return fans_passes(origins3, plan, foreign, stats, q, [&] { return launch(); });
}

int query_intersect_fans(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays, void *d_hits)
{
    int rc;
    if ((rc = check_fans_args(origins3, norigins, d_origin_of, d_dirs3, nrays, d_hits))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;

    std::vector<FanPass> plan;
    const std::initializer_list<CubeChoice> foreign = { { &g.lc, 3 }, { &g.qrows.cubes[0], 4 } };
    const bool binned = fans_binned(origins3, norigins, nrays, foreign, &plan);

    stream_begin();
    QueryStats &stats = stats_begin(QUERY_FAN, binned);
    if (!binned) return fans_brute(origins3, norigins, d_origin_of, d_dirs3, nrays, d_hits);

    QueryFansFrame q;
    memset(&q, 0, sizeof q);
    q.f = fan_frame(d_dirs3, nrays, d_hits);
    q.origin_of = static_cast<const int32_t *>(d_origin_of);
    if ((rc = stats_arm(QUERY_FAN, &q.f.stats))) return rc;          // (once: the passes' kernels add up in the same words)
    const dim3 grid((unsigned)((nrays + 255) / 256));
    return fans_passes(origins3, plan, foreign, stats, q, [&] { return launch_walk(k_query_fans_binned<false>, k_query_fans_binned<true>, q.f.stats != nullptr, grid, q); });
}

// ---- occlusion queries: any-hit rays (mirt_occluded*) ---------------------------------------------------------------------------
//
// One byte per ray: whether some accepted triangle is nearer than the ray's limit.  Arbitrary rays sweep the scene's rows
// (k_query_occluded*, the kernel chosen as for mirt_intersect*: launch_sweep); rays that share origins walk the many-origin fans' cubes
// (k_query_occluded_fans_binned) -- the same pass plan, the same kept cubes g.qrows.fans[] and the same foreign cubes as
// mirt_intersect_fans*, so a cube either call built serves the other.  The statistics are a kind of their own (QUERY_OCCLUDED):
// every call of either form begins them afresh, and no call touches the fans' or DirectLight's.

// The brute-force kernels for nrays > 0 rays on the current stream.
int occluded_launch(const void *d_rays, int nrays, const void *d_limit, void *d_occluded)
{
    int rc;
    if ((rc = query_rows())) return rc;
    const QueryOccludedFrame o = { rows_frame(d_rays, nrays, nullptr), static_cast<const float *>(d_limit), static_cast<uint8_t *>(d_occluded) };
    return launch_sweep(k_query_occluded_wave, k_query_occluded<QUERY_P>, nrays, o);
}

int query_occluded(const void *d_rays, int nrays, const void *d_max_distance, void *d_occluded)
{
    int rc;
    if ((rc = check_query_args(d_rays, nrays, d_occluded, "ray"))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    stream_begin();
    if (g.ray_grid) {                                        // (a call the grid answers is reported by mirt_get_ray_grid_stats alone:
        bool done = false;                                   //  the occlusion statistics keep the last call that swept or walked a cube)
        if ((rc = ray_grid_occluded(d_rays, nrays, d_max_distance, d_occluded, &done)) || done) return rc;
    }
    stats_begin(QUERY_OCCLUDED, false);
    return occluded_launch(d_rays, nrays, d_max_distance, d_occluded);
}

// AUTO for the many-origin form is auto_bins_fans' rule unchanged (fans_binned).  The rule was measured for closest hits; the
// sweep of this call (tools/ray_query_bench.py --steps occluded, profiles/ray_query_bench.txt, section `occluded`; K = 1, 4, 32
// origins, 1 .. 2^20 rays, 2000 and 100 000 triangles, with and without limits) puts the crossing in the same place: brute force
// ahead of binning with the builds in all 42 cells of at most 4096 rays, binning with the builds ahead beyond except at 2000
// triangles and 4 origins (16384 / 65536 rays: 0.50 / 0.53 against 0.47 / 0.49 ms), the cell mirt_intersect_fans* loses too.
int query_occluded_fans(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays, const void *d_max_distance,
                        void *d_occluded)
{
    int rc;
    if ((rc = check_fans_args(origins3, norigins, d_origin_of, d_dirs3, nrays, d_occluded))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;

    std::vector<FanPass> plan;
    const std::initializer_list<CubeChoice> foreign = { { &g.lc, 3 }, { &g.qrows.cubes[0], 4 } };
    const bool binned = fans_binned(origins3, norigins, nrays, foreign, &plan);

    stream_begin();
    QueryStats &stats = stats_begin(QUERY_OCCLUDED, binned);
    if (!binned) {
        // mirt_occluded on the expanded rays; a ray whose index lies outside the list becomes one no triangle accepts: its byte is 0
        if ((rc = fans_expand(origins3, norigins, d_origin_of, d_dirs3, nrays))) return rc;
        return occluded_launch(g.cur().query.d_fan_rays, nrays, d_max_distance, d_occluded);
    }

    QueryOccludedFansFrame q;
    memset(&q, 0, sizeof q);
    q.f.f = fan_frame(d_dirs3, nrays, nullptr);
    q.f.origin_of = static_cast<const int32_t *>(d_origin_of);
    q.norigins = norigins;
    q.limit = static_cast<const float *>(d_max_distance);
    q.occluded = static_cast<uint8_t *>(d_occluded);
    if ((rc = stats_arm(QUERY_OCCLUDED, &q.f.f.stats))) return rc;    // (once: the passes' kernels add up in the same words)
    const dim3 grid((unsigned)((nrays + 255) / 256));
    // (plan[0].first == 0: the pass that writes the strays' 0)
    return fans_passes(origins3, plan, foreign, stats, q.f, [&] {
        return launch_walk(k_query_occluded_fans_binned<false>, k_query_occluded_fans_binned<true>, q.f.f.stats != nullptr, grid, q);
    });
}

int query_set_mode(int mode)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (mode != MIRT_QUERY_AUTO && mode != MIRT_QUERY_BRUTE && mode != MIRT_QUERY_BINNED)
        return fail(MIRT_ERR_INVALID_ARGUMENT, "unknown query mode %d", mode);
    g.query_mode = mode;
    return MIRT_OK;
}

// ---- host buffers: staged through library-owned device arrays, complete on return ----

int query_staging(size_t count)
{
    int rc;
    QueryRows &Q = g.qrows;
    if (count <= Q.cap) return MIRT_OK;
    Q.cap = 0;
    if ((rc = dev_realloc_bytes(&Q.d_rays, count * sizeof(mirt_ray)))) return rc;
    if ((rc = dev_realloc_bytes(&Q.d_hits, count * sizeof(mirt_hit)))) return rc;
    if ((rc = dev_realloc_bytes(&Q.d_rgb, count * 3 * sizeof(float)))) return rc;
    if ((rc = dev_realloc_bytes(&Q.d_dirs, count * 3 * sizeof(float)))) return rc;
    if ((rc = dev_realloc_bytes(&Q.d_origin_of, count * sizeof(int32_t)))) return rc;
    if ((rc = dev_realloc_bytes(&Q.d_limits, count * sizeof(float)))) return rc;
    if ((rc = dev_realloc_bytes(&Q.d_occluded, count))) return rc;
    Q.cap = count;
    return MIRT_OK;
}

// (the host-buffer wrapper with_host_arrays: capi.hpp)

int query_intersect_host(const mirt_ray *rays, int nrays, mirt_hit *hits)
{
    QueryRows &Q = g.qrows;
    const HostArray a[] = { { (void *)rays, &QueryRows::d_rays, (size_t)nrays * sizeof(mirt_ray), true, false },
                            { hits, &QueryRows::d_hits, (size_t)nrays * sizeof(mirt_hit), true, true } };
    return with_host_arrays(check_query_args(rays, nrays, hits, "ray"), nrays, a, [&] { return query_intersect(Q.d_rays, nrays, Q.d_hits); });
}

int query_direct_light_host(const mirt_hit *hits, int nhits, const mirt_light *lights, int nlights, float *out_rgb)
{
    int npos = 0, checked = check_query_args(hits, nhits, out_rgb, "hit");
    if (!checked) checked = check_lights(lights, nlights, &npos);
    QueryRows &Q = g.qrows;
    const HostArray a[] = { { (void *)hits, &QueryRows::d_hits, (size_t)nhits * sizeof(mirt_hit), true, false },
                            { out_rgb, &QueryRows::d_rgb, (size_t)nhits * 3 * sizeof(float), false, true } };
    return with_host_arrays(checked, nhits, a, [&] { return query_direct_light(Q.d_hits, nhits, lights, nlights, Q.d_rgb); });
}

// The mask's staging array is its own and grows by its own measure -- up to 32 bytes a record, which the other arrays' callers
// should not pay for --, once the checks have passed and there is something to stage.
static int mask_staging(int checked, int nhits, size_t words)
{
    QueryRows &Q = g.qrows;
    if (checked || nhits == 0 || g.n <= 0 || words <= Q.mask_cap) return MIRT_OK;
    Q.mask_cap = 0;
    const int rc = dev_realloc_bytes(&Q.d_mask, words * sizeof(uint32_t));
    if (!rc) Q.mask_cap = words;
    return rc;
}

int query_shadow_mask_host(const mirt_hit *hits, int nhits, const mirt_light *lights, int nlights, uint32_t *mask)
{
    int rc, npos = 0;
    const int checked = check_mask_args(hits, nhits, lights, nlights, mask, hits, &npos);
    const size_t words = (size_t)light_mask_words(npos) * (size_t)(nhits > 0 ? nhits : 0);
    if ((rc = mask_staging(checked, nhits, words))) return rc;
    QueryRows &Q = g.qrows;
    const HostArray a[] = { { (void *)hits, &QueryRows::d_hits, (size_t)nhits * sizeof(mirt_hit), true, false },
                            { mask, &QueryRows::d_mask, words * sizeof(uint32_t), false, words != 0 } };
    return with_host_arrays(checked, nhits, a, [&] { return query_shadow_mask(Q.d_hits, nhits, lights, nlights, Q.d_mask); });
}

int query_direct_light_masked_host(const mirt_hit *hits, int nhits, const mirt_light *lights, int nlights, const uint32_t *mask, float *out_rgb)
{
    int rc, npos = 0;
    const int checked = check_mask_args(hits, nhits, lights, nlights, mask, out_rgb, &npos);
    const size_t words = (size_t)light_mask_words(npos) * (size_t)(nhits > 0 ? nhits : 0);
    if ((rc = mask_staging(checked, nhits, words))) return rc;
    QueryRows &Q = g.qrows;
    const HostArray a[] = { { (void *)hits, &QueryRows::d_hits, (size_t)nhits * sizeof(mirt_hit), true, false },
                            { (void *)mask, &QueryRows::d_mask, words * sizeof(uint32_t), words != 0, false },
                            { out_rgb, &QueryRows::d_rgb, (size_t)nhits * 3 * sizeof(float), false, true } };
    return with_host_arrays(checked, nhits, a, [&] { return query_direct_light_masked(Q.d_hits, nhits, lights, nlights, Q.d_mask, Q.d_rgb); });
}

int query_intersect_from_host(const float *origin, const float *dirs3, int nrays, mirt_hit *hits)
{
    QueryRows &Q = g.qrows;
    const HostArray a[] = { { (void *)dirs3, &QueryRows::d_dirs, (size_t)nrays * 3 * sizeof(float), true, false },
                            { hits, &QueryRows::d_hits, (size_t)nrays * sizeof(mirt_hit), true, true } };
    return with_host_arrays(check_from_args(origin, dirs3, nrays, hits), nrays, a, [&] { return query_intersect_from(origin, Q.d_dirs, nrays, Q.d_hits); });
}

// The host form looks at every index before anything touches the device; the device form cannot (its kernels leave such a ray's
// record unwritten).
int fans_index_args(int norigins, const int32_t *origin_of, int nrays)
{
    if (origin_of)
        for (int i = 0; i < nrays; i++)
            if (origin_of[i] < 0 || origin_of[i] >= norigins)
                return fail(MIRT_ERR_INVALID_ARGUMENT, "origin_of[%d] = %d is outside [0, %d)", i, (int)origin_of[i], norigins);
    return MIRT_OK;
}
static int check_fans_host_args(const float *origins3, int norigins, const int32_t *origin_of, const float *dirs3, int nrays, const void *hits)
{
    int rc;
    if ((rc = check_fans_args(origins3, norigins, origin_of, dirs3, nrays, hits))) return rc;
    return fans_index_args(norigins, origin_of, nrays);
}

int query_intersect_fans_host(const float *origins3, int norigins, const int32_t *origin_of, const float *dirs3, int nrays, mirt_hit *hits)
{
    QueryRows &Q = g.qrows;
    const HostArray a[] = { { (void *)dirs3, &QueryRows::d_dirs, (size_t)nrays * 3 * sizeof(float), true, false },
                            { hits, &QueryRows::d_hits, (size_t)nrays * sizeof(mirt_hit), true, true },
                            { (void *)origin_of, &QueryRows::d_origin_of, (size_t)nrays * sizeof(int32_t), origin_of != nullptr, false } };
    return with_host_arrays(check_fans_host_args(origins3, norigins, origin_of, dirs3, nrays, hits), nrays, a,
                            [&] { return query_intersect_fans(origins3, norigins, origin_of ? Q.d_origin_of : nullptr, Q.d_dirs, nrays, Q.d_hits); });
}

// (a NULL max_distance stays NULL: every limit is +inf)
int query_occluded_host(const mirt_ray *rays, int nrays, const float *max_distance, uint8_t *occluded)
{
    QueryRows &Q = g.qrows;
    const HostArray a[] = { { (void *)rays, &QueryRows::d_rays, (size_t)nrays * sizeof(mirt_ray), true, false },
                            { (void *)max_distance, &QueryRows::d_limits, (size_t)nrays * sizeof(float), max_distance != nullptr, false },
                            { occluded, &QueryRows::d_occluded, (size_t)nrays, false, true } };
    return with_host_arrays(check_query_args(rays, nrays, occluded, "ray"), nrays, a,
                            [&] { return query_occluded(Q.d_rays, nrays, max_distance ? Q.d_limits : nullptr, Q.d_occluded); });
}

int query_occluded_fans_host(const float *origins3, int norigins, const int32_t *origin_of, const float *dirs3, int nrays, const float *max_distance,
                             uint8_t *occluded)
{
    QueryRows &Q = g.qrows;
    const HostArray a[] = { { (void *)dirs3, &QueryRows::d_dirs, (size_t)nrays * 3 * sizeof(float), true, false },
                            { (void *)origin_of, &QueryRows::d_origin_of, (size_t)nrays * sizeof(int32_t), origin_of != nullptr, false },
                            { (void *)max_distance, &QueryRows::d_limits, (size_t)nrays * sizeof(float), max_distance != nullptr, false },
                            { occluded, &QueryRows::d_occluded, (size_t)nrays, false, true } };
    return with_host_arrays(check_fans_host_args(origins3, norigins, origin_of, dirs3, nrays, occluded), nrays, a, [&] {
        return query_occluded_fans(origins3, norigins, origin_of ? Q.d_origin_of : nullptr, Q.d_dirs, nrays, max_distance ? Q.d_limits : nullptr, Q.d_occluded);
    });
}

}  // namespace mirt

extern "C" int mirt_intersect(const mirt_ray *rays, int nrays, mirt_hit *hits) { return mirt::query_intersect_host(rays, nrays, hits); }
extern "C" int mirt_intersect_device(const void *d_rays, int nrays, void *d_hits) { return mirt::query_intersect(d_rays, nrays, d_hits); }
extern "C" int mirt_direct_light(const mirt_hit *hits, int nhits, const mirt_light *lights, int nlights, float *out_rgb) { return mirt::query_direct_light_host(hits, nhits, lights, nlights, out_rgb); }
extern "C" int mirt_direct_light_device(const void *d_hits, int nhits, const mirt_light *lights, int nlights, void *d_rgb) { return mirt::query_direct_light(d_hits, nhits, lights, nlights, d_rgb); }
extern "C" int mirt_shadow_mask(const mirt_hit *hits, int nhits, const mirt_light *lights, int nlights, uint32_t *mask) { return mirt::query_shadow_mask_host(hits, nhits, lights, nlights, mask); }
extern "C" int mirt_shadow_mask_device(const void *d_hits, int nhits, const mirt_light *lights, int nlights, void *d_mask) { return mirt::query_shadow_mask(d_hits, nhits, lights, nlights, d_mask); }
extern "C" int mirt_direct_light_masked(const mirt_hit *hits, int nhits, const mirt_light *lights, int nlights, const uint32_t *mask, float *out_rgb) { return mirt::query_direct_light_masked_host(hits, nhits, lights, nlights, mask, out_rgb); }
extern "C" int mirt_direct_light_masked_device(const void *d_hits, int nhits, const mirt_light *lights, int nlights, const void *d_mask, void *d_rgb) { return mirt::query_direct_light_masked(d_hits, nhits, lights, nlights, d_mask, d_rgb); }
extern "C" int mirt_get_shadow_mask_stats(mirt_query_stats *out) { return mirt::query_get_stats(mirt::QUERY_SHADOW_MASK, out); }
extern "C" int mirt_occluded(const mirt_ray *rays, int nrays, const float *max_distance, uint8_t *occluded) { return mirt::query_occluded_host(rays, nrays, max_distance, occluded); }
extern "C" int mirt_occluded_device(const void *d_rays, int nrays, const void *d_max_distance, void *d_occluded) { return mirt::query_occluded(d_rays, nrays, d_max_distance, d_occluded); }
extern "C" int mirt_occluded_fans(const float *origins3, int norigins, const int32_t *origin_of, const float *dirs3, int nrays, const float *max_distance, uint8_t *occluded) { return mirt::query_occluded_fans_host(origins3, norigins, origin_of, dirs3, nrays, max_distance, occluded); }
extern "C" int mirt_occluded_fans_device(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays, const void *d_max_distance, void *d_occluded) { return mirt::query_occluded_fans(origins3, norigins, d_origin_of, d_dirs3, nrays, d_max_distance, d_occluded); }
extern "C" int mirt_get_occlusion_stats(mirt_query_stats *out) { return mirt::query_get_stats(mirt::QUERY_OCCLUDED, out); }
extern "C" int mirt_intersect_fans(const float *origins3, int norigins, const int32_t *origin_of, const float *dirs3, int nrays, mirt_hit *hits) { return mirt::query_intersect_fans_host(origins3, norigins, origin_of, dirs3, nrays, hits); }
extern "C" int mirt_intersect_fans_device(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays, void *d_hits) { return mirt::query_intersect_fans(origins3, norigins, d_origin_of, d_dirs3, nrays, d_hits); }
extern "C" int mirt_intersect_from(const float origin[3], const float *dirs3, int nrays, mirt_hit *hits) { return mirt::query_intersect_from_host(origin, dirs3, nrays, hits); }
extern "C" int mirt_intersect_from_device(const float origin[3], const void *d_dirs3, int nrays, void *d_hits) { return mirt::query_intersect_from(origin, d_dirs3, nrays, d_hits); }
extern "C" int mirt_get_fan_stats(mirt_query_stats *out) { return mirt::query_get_stats(mirt::QUERY_FAN, out); }
extern "C" int mirt_set_query_mode(int mode) { return mirt::query_set_mode(mode); }
extern "C" int mirt_get_query_stats(mirt_query_stats *out) { return mirt::query_get_stats(mirt::QUERY_DIRECT_LIGHT, out); }
