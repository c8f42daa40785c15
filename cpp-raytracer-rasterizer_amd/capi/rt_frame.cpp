// rt_frame.cpp -- a ray-traced frame: its parameter block, the choice of path (tile kernel, small-scene kernel, origin tables +
// wave / brute kernel, binned), and the launches of the paths that are not binned (binned.cpp holds those).
#include "capi.hpp"

namespace mirt {

// The camera ray family negD = -(R0*(x - W/2) + R1*(y - H/2) + R2*f) as a bin frame: (u, v) = pixel (x, y), bins =
// 8x8-pixel tiles; also carries the inverse map for the bounding boxes (rt_binned.hpp).
BinFrameDesc make_camera_frame(const mirt_view *view, int y0, int y1, int aa)
{
    const int W = view->width, H = view->height;
    BinFrameDesc c;
    memset(&c, 0, sizeof c);
    {
        const float *R = view->rot;                       // column-major: column j = R[3j..3j+2]
        const float hw = (float)W / 2.0f, hh = (float)H / 2.0f;
        for (int i = 0; i < 3; i++) {
            c.Pu[i] = -R[0 + i];
            c.Pv[i] = -R[3 + i];
            c.P0[i] = -(R[6 + i] * view->focal - R[0 + i] * hw - R[3 + i] * hh);
        }
        float dm = 0.0f;
        for (int i = 0; i < 3; i++)
            dm = fmaxf(dm, fabsf(R[0 + i]) * (hw + 1.0f) + fabsf(R[3 + i]) * (hh + 1.0f) + fabsf(R[6 + i]) * fabsf(view->focal));
        c.dmax = dm;
        // inverse map for the bounding boxes: h = R^-1 (P - S) = lambda * (x - W/2, y - H/2, f), so with g = S - P
        //   w = -(R^-1 row 2 . g) / f,  u = (-(R^-1 row 0 . g) + (W/2) f w / f ... ) -> rows below; computed in double
        {
            double M[9], inv[9];
            for (int i = 0; i < 9; i++) M[i] = R[i];
#define MM(cc, rr) M[(cc) * 3 + (rr)]
            const double det = MM(0, 0) * (MM(1, 1) * MM(2, 2) - MM(2, 1) * MM(1, 2)) - MM(1, 0) * (MM(0, 1) * MM(2, 2) - MM(2, 1) * MM(0, 2)) +
                               MM(2, 0) * (MM(0, 1) * MM(1, 2) - MM(1, 1) * MM(0, 2));
            // inv is row-major here: inv[r*3+c] = (R^-1)(r, c)
            inv[0] = (MM(1, 1) * MM(2, 2) - MM(2, 1) * MM(1, 2)) / det; inv[1] = -(MM(1, 0) * MM(2, 2) - MM(2, 0) * MM(1, 2)) / det; inv[2] = (MM(1, 0) * MM(2, 1) - MM(2, 0) * MM(1, 1)) / det;
            inv[3] = -(MM(0, 1) * MM(2, 2) - MM(2, 1) * MM(0, 2)) / det; inv[4] = (MM(0, 0) * MM(2, 2) - MM(2, 0) * MM(0, 2)) / det; inv[5] = -(MM(0, 0) * MM(2, 1) - MM(2, 0) * MM(0, 1)) / det;
            inv[6] = (MM(0, 1) * MM(1, 2) - MM(1, 1) * MM(0, 2)) / det; inv[7] = -(MM(0, 0) * MM(1, 2) - MM(1, 0) * MM(0, 2)) / det; inv[8] = (MM(0, 0) * MM(1, 1) - MM(1, 0) * MM(0, 1)) / det;
#undef MM
            const bool ok = std::isfinite(det) && det != 0.0 && view->focal != 0.0f;
            for (int i = 0; i < 3; i++) {
                const double rwd = ok ? -inv[6 + i] / (double)view->focal : 0.0;       // w = h.z / f, h = -R^-1 g
                c.rw[i] = (float)rwd;
                c.ru[i] = (float)(ok ? -inv[0 + i] + (double)hw * rwd : 0.0);          // u*w = h.x + (W/2) w
                c.rv[i] = (float)(ok ? -inv[3 + i] + (double)hh * rwd : 0.0);
            }
        }
        memcpy(c.S, view->pos, 12);
        c.ulo = 0.0f; c.vlo = 0.0f; c.du = (float)BIN_TILE; c.dv = (float)BIN_TILE;
        // bin i covers the rays of pixels 8i .. 8i+7: exactly their centres, or with supersampling half a pixel around them
        // (at 4, 6, 7 and 8 samples the chain of sub-ray coordinates ends up to a few ulp beyond the half pixel; the edge-function
        // margin covers that 20 times over: tests/test_aa_reach.py)
        c.pad_lo = aa > 1 ? -0.5f : 0.0f; c.pad_hi = aa > 1 ? -0.5f : -1.0f;
        c.nbu = (W + BIN_TILE - 1) / BIN_TILE; c.nbv = (H + BIN_TILE - 1) / BIN_TILE;
        c.j0 = y0 / BIN_TILE; c.j1 = (y1 + BIN_TILE - 1) / BIN_TILE;
        c.base = 0; c.tab = 0;
    }
    return c;
}

int check_lights(const mirt_light *lights, int nlights, int *light_positions)
{
    if (nlights < 0 || nlights > MIRT_MAX_LIGHTS) return fail(MIRT_ERR_INVALID_ARGUMENT, "nlights %d out of range [0,%d]", nlights, MIRT_MAX_LIGHTS);
    if (nlights > 0 && !lights) return fail(MIRT_ERR_INVALID_ARGUMENT, "lights must not be NULL when nlights > 0");
    const int samples = soft_samples();
    *light_positions = nlights * samples;
    if (*light_positions > MIRT_MAX_LIGHT_POSITIONS)
        return fail(MIRT_ERR_INVALID_ARGUMENT, "%d lights x %d soft-shadow samples exceed %d light positions", nlights, samples, MIRT_MAX_LIGHT_POSITIONS);
    if (samples > 1 && *light_positions > g.soft_npos)
        return fail(MIRT_ERR_INVALID_ARGUMENT, "%d lights x %d soft-shadow samples exceed the %d jittered positions set: %d jittered positions needed (mirt_set_soft_shadows)",
                    nlights, samples, g.soft_npos, *light_positions);
    return MIRT_OK;
}

int many_lights_min()
{
    static const int v = (int)env_int("MIRT_MANY_LIGHTS_MIN", MIRT_MAX_LIGHTS + 1);
    return v;
}

int aa_defer_min()
{
    static const int v = (int)env_int("MIRT_AA_DEFER_MIN", MIRT_MAX_LIGHTS + 1);
    return v;
}

// Whether a frame of so many light positions shades each carried record once (aa_record_once_frame): supersampling on, the opt-in
// on (mirt_set_supersampled_many_lights), and at least MIRT_AA_DEFER_MIN positions.
static bool aa_record_once(int light_positions)
{
    return g.aa_many_lights && g.aa > 1 && light_positions >= aa_defer_min();
}

// Whether a frame of so many light positions is deferred (rt_enqueue): always beyond what RtFrame carries, and from
// MIRT_MANY_LIGHTS_MIN positions on when that is set lower -- but never a supersampled frame the fused kernels can render.
static bool frame_deferred(int light_positions)
{
    const int aa = g.aa > 1 ? g.aa : 1;
    return light_positions > MIRT_MAX_LIGHTS || (aa <= 1 && light_positions >= many_lights_min());
}

void fill_light_positions(const mirt_light *lights, int npos, float (*lpos)[3], float (*lcol)[3], float *origins)
{
    const int samples = soft_samples();
    for (int j = 0; j < npos; j++) {
        const mirt_light &l = lights[j / samples];
        const float *pos = samples > 1 ? g.soft_pos + 3 * j : l.pos;
        if (lpos) memcpy(lpos[j], pos, 12);
        if (origins) memcpy(origins + 3 * (j + 1), pos, 12);
        // uniform per light, so the division happens once here (host float division is the same IEEE operation the kernels
        // would run per pixel)
        if (lcol) for (int c = 0; c < 3; c++) lcol[j][c] = (l.color[c] * l.intensity) / (float)samples;
    }
}

// The frame's parameter block, apart from what its stream supplies (hit counters, origin tables); `origins` receives the camera
// and the light positions the shadow rays start from (1 + f.nlights rows of 3).
static void make_rt_frame(RtFrame &f, float *origins, const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                          int y0, int y1, int row_origin, void *d_xrgb, int pitch_bytes, void *d_rgb, void *d_index, void *d_fd, void *d_dist, void *d_pos)
{
    memset(&f, 0, sizeof f);
    f.tris15 = g.d_tris;
    f.n = g.n;
    memcpy(f.cam, view->pos, sizeof f.cam);
    memcpy(f.rot, view->rot, sizeof f.rot);
    f.focal = view->focal;
    f.W = view->width;
    f.H = view->height;
    const int npos = nlights * soft_samples();
    f.nlights = npos;
    f.samples = soft_samples();
    f.aa = g.aa > 1 ? g.aa : 1;
    memcpy(origins, view->pos, 12);
    fill_light_positions(lights, npos, f.lpos, f.lcol, origins);
    f.lights_in_range = 1;
    for (int j = 0; j < npos; j++) f.lights_in_range &= light_colour_in_range(f.lcol[j]) ? 1 : 0;
    memcpy(f.indirect, indirect, 12);
    f.y0 = y0; f.y1 = y1; f.row_origin = row_origin;
    f.xrgb = static_cast<uint32_t *>(d_xrgb);
    f.pitch_words = pitch_bytes / 4;
    f.rgb = static_cast<float *>(d_rgb);
    f.index = static_cast<int32_t *>(d_index);
    f.fd = static_cast<float *>(d_fd);
    f.dist = static_cast<float *>(d_dist);
    f.pos = static_cast<float *>(d_pos);
    f.focal_plane = g.dof_focal;
}

static bool finite_below(const float *p, int n, float lim)
{
    for (int i = 0; i < n; i++) if (!(fabsf(p[i]) < lim)) return false;
    return true;
}

// The pre-reject filter is proven for finite, moderate operands only (rt_common.hpp); anything else (absurd coordinates, NaN/Inf)
// renders through the exact-only path.  Ray directions of the primary rays are bounded by 3 * max|rot| * max(W, H, |focal|).
// `origins`: the camera and the npos light positions.
static bool operands_safe(const mirt_view *view, const float *origins, int npos)
{
    float rmax = 0.0f;
    for (int i = 0; i < 9; i++) rmax = fmaxf(rmax, fabsf(view->rot[i]));
    const float dmax = 3.0f * rmax * fmaxf(fmaxf((float)view->width, (float)view->height), fabsf(view->focal));
    return g.scene_finite && finite_below(view->rot, 9, 1.0e6f) && (dmax < 1.0e6f) &&
           finite_below(origins, 3 * (1 + npos), 1.0e8f);      // camera and light positions
}

// MIRT_RT_AUTO bins when the scene is beyond the tile kernel (65 triangles or more) and the brute-force work, pixels x
// triangles, is above ~4e7: binning + sorting costs ~40 us whatever the scene, brute force ~7.5e-10 ms per pixel-triangle
// (tools/threshold_sweep.py at 1080p: 65 triangles 0.099 vs 0.043 ms, 300: 0.47 vs 0.079, 800: 1.13 vs 0.097).
int auto_bin_threshold()
{
    static const int v = (int)env_int("MIRT_BIN_THRESHOLD", 65);
    return v;
}
static bool mode_bins(const mirt_view *view, int mode, int rows)
{
    return (mode == MIRT_RT_BINNED) ||
           (mode == MIRT_RT_AUTO && g.n >= auto_bin_threshold() && (long long)view->width * rows > 4096 &&
            (long long)view->width * rows * g.n >= 40000000LL);
}

bool rt_bins_whole_frame(const mirt_view *view, const mirt_light *lights, int nlights, int mode)
{
    const int samples = soft_samples(), npos = nlights * samples;
    // (check_lights' conditions, without its messages: the question is asked, not a frame)
    if (!view || nlights < 0 || nlights > MIRT_MAX_LIGHTS || (nlights && !lights) || npos > MIRT_MAX_LIGHT_POSITIONS || (samples > 1 && npos > g.soft_npos)) return false;
    if (npos > MIRT_MAX_LIGHTS && g.aa > 1) return false;    // (rt_enqueue refuses the frame, or shades each record once: no tile pass)
    if (aa_record_once(npos)) return false;
    // a deferred frame: the answer is its primary pass's, which has no light
    const int fused = frame_deferred(npos) ? 0 : npos;
    float origins[(1 + MIRT_MAX_LIGHTS) * 3];
    memcpy(origins, view->pos, 12);
    fill_light_positions(lights, fused, nullptr, nullptr, origins);
    return mode_bins(view, mode, view->height) && operands_safe(view, origins, fused) && frame_fits_binning(view->width, view->height);
}

// The frames that are not binned.  Scenes of at most 64 triangles (the reference's Cornell box has 30): per-tile candidate
// masks, one lane per triangle (rt_tile.hip), when the operands are inside the filter's proven range; other small scenes: one
// launch, every table built in LDS by the workgroup itself -- no origin-table kernel, no global loads inside the loops; the
// rest: the stream's origin tables (k_prep_origin), then a wave per ray (few rays, many triangles) or the brute-force kernel.
static int rt_dispatch_brute(RtFrame &f, const mirt_view *view, OriginTables &S, const float *origins, int nlights, bool safe, bool tile_path, size_t tile_lds)
{
    StreamState &ss = g.cur();
    const int rows = f.y1 - f.y0;
    if (tile_path) {
        RtTileFrame tf;
        memset(&tf, 0, sizeof tf);
        tf.f = f;
        tf.cam = make_camera_frame(view, f.y0, f.y1, g.aa);
        // a wave owns a 16 x 8-pixel tile, two pixels per lane (packed FP32, rt_tile.hip); workgroups of 4 waves, one workgroup
        // per 4 tiles.  Tile cost varies several-fold (candidates, shadowed or lit), and the hardware's dynamic workgroup dispatch
        // balances that better than any static assignment (measured on the Cornell box at 1080p: 40.5 us with one tile per wave,
        // 46 us with a resident grid striding over the tiles, 49 us with 3 tiles per wave).
        const int tw = 16, th = 8, wpb = 4;
        tf.tiles_x = (view->width + tw - 1) / tw;
        tf.tiles_y = (rows + th - 1) / th;
        const long long ntiles = (long long)tf.tiles_x * tf.tiles_y;
        const unsigned blocks = (unsigned)((ntiles + wpb - 1) / wpb);
        if (!ss.hits_clean[ss.hits_tog]) HIP_TRY(hipMemsetAsync(g.d_hits, 0, HIT_BYTES, g.stream));
        ss.hits_clean[ss.hits_tog] = false;
        g.pending_counted = true;
        tf.clear_hits = ss.d_hits[ss.hits_tog ^ 1];      // zeroed by this launch for the next frame on this stream: no memset node per frame
        ss.hits_clean[ss.hits_tog ^ 1] = true;
        // Tables: built once per frame by k_tile_tables when the frame has enough workgroups to make rebuilding them in
        // each one the larger cost; small frames are bound by the launch rate and keep the single launch.
        tf.tables = blocks >= 1024u ? ss.d_tile_tab : nullptr;
        if (tf.tables) {
            k_begin(MIRT_K_PREP);
            hipLaunchKernelGGL(k_tile_tables, dim3(1), dim3(64), 0, g.stream, tf);
            k_end(MIRT_K_PREP);
        }
        k_begin(MIRT_K_TRACE);
        if (f.aa > 1) hipLaunchKernelGGL((k_rt_tile2<16, true>), dim3(blocks), dim3(64 * wpb), tile_lds, g.stream, tf);
        else hipLaunchKernelGGL((k_rt_tile2<16, false>), dim3(blocks), dim3(64 * wpb), tile_lds, g.stream, tf);
        k_end(MIRT_K_TRACE);
        HIP_TRY(hipGetLastError());
        return MIRT_OK;
    }

    const size_t small_lds = 16 + (size_t)g.n * sizeof(OriginRow) * (2 + nlights);
    if (small_lds <= 48 * 1024) {
        HIP_TRY(hipMemsetAsync(g.d_hits, 0, HIT_BYTES, g.stream));
        ss.hits_clean[ss.hits_tog] = false;
        k_begin(MIRT_K_TRACE);
        // (two rays per lane, packed FP32 filter: 188 -> 163 ms on the 100 k soup against one)
        hipLaunchKernelGGL(k_rt_small<2>, dim3((view->width + 127) / 128, (rows + 3) / 4), dim3(256), small_lds, g.stream, f, safe ? 0 : 1);
        k_end(MIRT_K_TRACE);
        HIP_TRY(hipGetLastError());
        return MIRT_OK;
    }

    const uint32_t flags_init[4] = { safe ? 0u : 1u, 0u, 0u, 0u };
    HIP_TRY(upload_small(S.d_flags, flags_init, sizeof flags_init, g.stream));
    ss.cam.kept.forget();                        // (k_prep_origin below overwrites the camera rows a kept binning pass would count on)
    ss.hits_clean[ss.hits_tog] = false;
    HIP_TRY(upload_small(S.d_origins, origins, sizeof(float) * 3 * (1 + nlights), g.stream));

    k_begin(MIRT_K_PREP);
    hipLaunchKernelGGL(k_prep_origin, dim3((g.n + 255) / 256, 1 + nlights), dim3(256), 0, g.stream,
                       g.d_tris, g.n, S.d_origins, V3(0.0f, 0.0f, 0.0f), 0, S.d_cam_tab, S.d_light_tab, S.d_flags, g.d_hits, (uint32_t *)nullptr);
    k_end(MIRT_K_PREP);

    k_begin(MIRT_K_TRACE);
    if (g.aa <= 1 && (long long)view->width * rows <= 4096 && g.n >= 1024) {
        // few rays, many triangles: one wave per ray, lanes over triangles, wavefront min-t reduce
        const long long nrays = (long long)view->width * rows;
        hipLaunchKernelGGL(k_rt_wave, dim3((unsigned)((nrays + 3) / 4)), dim3(256), 0, g.stream, f);
    } else {
        hipLaunchKernelGGL(k_rt_brute<2>, dim3((view->width + 127) / 128, (rows + 3) / 4), dim3(256), sweep_lds_bytes(), g.stream, f);
    }
    k_end(MIRT_K_TRACE);
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}

// The light of a deferred frame, behind its primary pass on the frame's stream (../lights/many_lights.hip): the planes that pass
// left in f become one hit record per pixel of the band, DirectLight runs over the records in passes of at most MIRT_MAX_LIGHTS
// positions (query.cpp: direct_light_passes -- the frame's mode decides between its kernels, mirt_set_query_mode and the queries'
// statistics stay out of it), and the resolve writes pixelColours and the surface's words.  All of it is bracketed as the frame's
// trace step, the cube builds of binned passes as its binning step.
static int deferred_lights(const RtFrame &f, const mirt_light *lights, int npos, int mode)
{
    int rc;
    ManyLightsScratch &M = g.cur().many;
    const int pixels = f.W * (f.y1 - f.y0);
    ManyLightsFrame m;
    memset(&m, 0, sizeof m);
    m.W = f.W; m.H = f.H; m.y0 = f.y0; m.y1 = f.y1; m.row_origin = f.row_origin;
    m.index = f.index; m.dist = f.dist; m.pos = f.pos;
    m.records = M.d_records;
    m.direct = M.d_direct;
    m.tris15 = f.tris15;
    m.n = f.n;
    memcpy(m.indirect, f.indirect, 12);
    m.xrgb = f.xrgb; m.pitch_words = f.pitch_words; m.rgb = f.rgb;
    const dim3 grid((unsigned)((pixels + 255) / 256));
    if (!g.cur().ev_used[MIRT_K_TRACE]) k_begin(MIRT_K_TRACE);
    hipLaunchKernelGGL(k_frame_records, grid, dim3(256), 0, g.stream, m);
    HIP_TRY(hipGetLastError());
    const int qmode = mode == MIRT_RT_BRUTE ? MIRT_QUERY_BRUTE : (mode == MIRT_RT_BINNED ? MIRT_QUERY_BINNED : MIRT_QUERY_AUTO);
    size_t carry_cap = M.cap_px;                             // (ensure sized it for these pixels)
    if ((rc = direct_light_passes(M.d_records, pixels, lights, npos, M.d_direct, qmode, direct_light_auto_bins(pixels, npos), false, &M.d_carry, &carry_cap))) return rc;
    hipLaunchKernelGGL(k_frame_resolve, grid, dim3(256), 0, g.stream, m);
    HIP_TRY(hipGetLastError());
    k_end(MIRT_K_TRACE);                                     // (the end of the primary pass's bracket moves behind the resolve)
    return MIRT_OK;
}

// A supersampled frame that shades each carried record once (../lights/aa_versions.hpp has the argument, aa_many_lights.hip the
// kernels, aa_plan.hpp the chunks): the band in chunks of rows, per chunk the list's fill (0xFF: index -1, which DirectLight answers
// with zeros and never traces), k_aa_primary -- through the cube around the camera, or sweeping the camera's origin table --,
// DirectLight over the whole capacity of the list in passes (query.cpp: direct_light_passes, as deferred_lights calls it) and
// k_aa_resolve, all on the frame's stream with no read-back.  AUTO's rule for the passes is decided once, from the band's pixels.
// The chunks are the frame's trace step, the cube builds its binning step.
static int aa_record_once_frame(const mirt_view *view, const mirt_light *lights, int npos, const float *indirect, int mode,
                                int y0, int y1, int row_origin, void *d_xrgb, int pitch_bytes, void *d_rgb, void *d_index, void *d_fd,
                                void *d_dist, void *d_pos)
{
    int rc;
    static const long long budget_mb = env_int("MIRT_AA_DEFER_SCRATCH_MB", AA_DEFER_SCRATCH_DEFAULT_MB);
    static const int forced_rows = (int)env_int("MIRT_AA_DEFER_ROWS", 0);
    const int W = view->width, aa = g.aa;
    call_begin();
    g.pending_is_rt = true;
    g.pending_primary = (uint64_t)W * (uint64_t)(y1 - y0) * (uint64_t)(aa * aa);
    g.pending_nlights = npos;
    g.stats.mode_used = MIRT_RT_BRUTE;
    g.pending_empty = (y1 == y0);
    g.pending_counted = false;
    if (y1 == y0) { call_end(); return MIRT_OK; }
    StreamState &ss = g.cur();
    ss.hits_tog ^= 1;
    g.d_hits = ss.d_hits[ss.hits_tog];
    HIP_TRY(hipMemsetAsync(g.d_hits, 0, HIT_BYTES, g.stream));
    ss.hits_clean[ss.hits_tog] = false;

    const int rows_per_chunk = aa_chunk_rows(W, y1 - y0, aa, std::max(budget_mb, 0ll) << 20, forced_rows);
    const size_t chunk_px = (size_t)W * rows_per_chunk, cap = aa_chunk_records(W, rows_per_chunk, aa);
    AaScratch &A = ss.aa;
    if ((rc = A.ensure(chunk_px, cap))) return rc;
    HIP_TRY(hipMemsetAsync(A.d_stats, 0, 16, g.stream));
    g.aa_stats_stream = g.stream;
    g.aa_stats_dev = A.d_stats;

    AaFrame a;
    memset(&a, 0, sizeof a);
    a.tris15 = g.d_tris;
    a.n = g.n;
    memcpy(a.cam, view->pos, sizeof a.cam);
    memcpy(a.rot, view->rot, sizeof a.rot);
    a.focal = view->focal;
    a.W = W; a.H = view->height; a.aa = aa;
    a.row_origin = row_origin;
    a.index = static_cast<int32_t *>(d_index);
    a.fd = static_cast<float *>(d_fd);
    a.focal_plane = g.dof_focal;
    a.dist = static_cast<float *>(d_dist);
    a.pos = static_cast<float *>(d_pos);
    a.hit_count = g.d_hits;
    a.records = A.d_records; a.cursor = A.d_cursor; a.slots = A.d_slots; a.counts = A.d_counts; a.nver = A.d_nver;
    a.direct = A.d_direct;
    memcpy(a.indirect, indirect, 12);
    a.xrgb = static_cast<uint32_t *>(d_xrgb);
    a.pitch_words = pitch_bytes / 4;
    a.rgb = static_cast<float *>(d_rgb);
    a.stats = A.d_stats;

    // the primary sub-rays: through the camera's cube, or sweeping its origin table (built as for any brute-force frame)
    const LightCache *cube = nullptr;
    if ((rc = aa_camera_cube(view->pos, mode, (long long)g.pending_primary, &cube))) return rc;
    if (cube) {
        a.tab = cube->d_light_tab;
        a.cube = cube_view(*cube);
        g.stats.mode_used = MIRT_RT_BINNED;
    } else {
        OriginTables &S = ss.tabs;
        if ((rc = S.ensure_cam_rows())) return rc;
        if (!S.d_origins) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&S.d_origins), sizeof(float) * 3 * (1 + MIRT_MAX_LIGHTS)));
        if (!S.d_flags) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&S.d_flags), 16));
        const uint32_t flags_init[4] = { operands_safe(view, view->pos, 0) ? 0u : 1u, 0u, 0u, 0u };
        HIP_TRY(upload_small(S.d_flags, flags_init, sizeof flags_init, g.stream));
        ss.cam.kept.forget();                    // (k_prep_origin below overwrites the camera rows a kept binning pass would count on)
        HIP_TRY(upload_small(S.d_origins, view->pos, sizeof(float) * 3, g.stream));
        k_begin(MIRT_K_PREP);
        hipLaunchKernelGGL(k_prep_origin, dim3((g.n + 255) / 256, 1), dim3(256), 0, g.stream,
                           g.d_tris, g.n, S.d_origins, V3(0.0f, 0.0f, 0.0f), 0, S.d_cam_tab, S.d_light_tab, S.d_flags, (unsigned long long *)nullptr, (uint32_t *)nullptr);
        k_end(MIRT_K_PREP);
        HIP_TRY(hipGetLastError());
        a.tab = S.d_cam_tab;
        a.unsafe = S.d_flags;
    }

    const int qmode = mode == MIRT_RT_BRUTE ? MIRT_QUERY_BRUTE : (mode == MIRT_RT_BINNED ? MIRT_QUERY_BINNED : MIRT_QUERY_AUTO);
    const long long band_px = (long long)W * (y1 - y0);
    const bool auto_rule = direct_light_auto_bins((int)std::min<long long>(band_px, 0x7fffffffLL), npos);
    const int nchunks = aa_chunk_count(y0, y1, rows_per_chunk);
    if (!ss.ev_used[MIRT_K_TRACE]) k_begin(MIRT_K_TRACE);
    for (int c = 0; c < nchunks; c++) {
        aa_chunk_of(y0, y1, rows_per_chunk, c, &a.y0, &a.y1);
        const size_t px = (size_t)W * (a.y1 - a.y0), records = aa_chunk_records(W, a.y1 - a.y0, aa);
        const dim3 grid((unsigned)((px + 255) / 256));
        HIP_TRY(hipMemsetAsync(A.d_records, 0xFF, records * HIT_WORDS * sizeof(uint32_t), g.stream));
        HIP_TRY(hipMemsetAsync(A.d_cursor, 0, 4, g.stream));
        if (cube) hipLaunchKernelGGL(k_aa_primary<true>, grid, dim3(256), 0, g.stream, a);
        else hipLaunchKernelGGL(k_aa_primary<false>, grid, dim3(256), sweep_lds_bytes(), g.stream, a);
        HIP_TRY(hipGetLastError());
        size_t carry_cap = A.cap_rec;                        // (ensure sized it for these records)
        if ((rc = direct_light_passes(A.d_records, (int)records, lights, npos, A.d_direct, qmode, auto_rule, false, &A.d_carry, &carry_cap))) return rc;
        hipLaunchKernelGGL(k_aa_resolve, grid, dim3(256), 0, g.stream, a);
        HIP_TRY(hipGetLastError());
    }
    k_end(MIRT_K_TRACE);
    call_end();
    return MIRT_OK;
}

int rt_enqueue(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect, int mode,
               int y0, int y1, int row_origin, void *d_xrgb, int pitch_bytes, void *d_rgb, void *d_index, void *d_fd,
               void *d_dist, void *d_pos)
{
    int rc;
    if ((rc = check_frame_args(view, lights, nlights, indirect, d_xrgb, pitch_bytes, true, y0, y1))) return rc;
    if (mode != MIRT_RT_AUTO && mode != MIRT_RT_BRUTE && mode != MIRT_RT_BINNED) return fail(MIRT_ERR_INVALID_ARGUMENT, "unknown mode %d", mode);
    int light_positions = 0;                                 // shadow-ray origins
    if ((rc = check_lights(lights, nlights, &light_positions))) return rc;

    // More positions than RtFrame carries: the frame is deferred (deferred_lights) -- its primary pass below renders with no light.
    // Supersampling shades the record a pixel carries at each of its aa x aa sub-rays (raytracer.cpp:580-594), which one record per
    // pixel cannot hold.
    // With mirt_set_supersampled_many_lights on, such a frame shades each record the pixel carries once instead (aa_record_once_frame).
    const bool deferred = frame_deferred(light_positions);
    if (aa_record_once(light_positions))
        return aa_record_once_frame(view, lights, light_positions, indirect, mode, y0, y1, row_origin, d_xrgb, pitch_bytes, d_rgb, d_index, d_fd, d_dist, d_pos);
    if (light_positions > MIRT_MAX_LIGHTS && g.aa > 1)
        return fail(MIRT_ERR_INVALID_ARGUMENT, "supersampling (mirt_set_antialiasing %d) cannot be combined with %d light positions: more than %d are rendered with one record per pixel",
                    g.aa, light_positions, MIRT_MAX_LIGHTS);

    RtFrame f;
    float origins[(1 + MIRT_MAX_LIGHTS) * 3];
    make_rt_frame(f, origins, view, lights, deferred ? 0 : nlights, indirect, y0, y1, row_origin, d_xrgb, pitch_bytes, d_rgb, d_index, d_fd, d_dist, d_pos);
    nlights = deferred ? 0 : light_positions;    // from here on "lights" means the light positions of the fused kernels
    const bool safe = operands_safe(view, origins, nlights);

    // ---- mode: brute force for small scenes, binned otherwise; unsafe operands always render exact brute ----
    bool binned = mode_bins(view, mode, y1 - y0);
    if (!safe) binned = false;
    if (binned && !frame_fits_binning(view->width, view->height)) {
        // more 8 x 8-pixel tiles than one sort pass has keys (a frame beyond ~23 000 x 23 000 pixels)
        if (mode == MIRT_RT_BINNED) return fail(MIRT_ERR_INVALID_ARGUMENT, "frame %dx%d has more tiles than the binned path can key; use MIRT_RT_AUTO or row bands of a smaller frame", view->width, view->height);
        binned = false;
    }
    const size_t tile_lds = (size_t)g.n * 16 * (12 + 3 * nlights);
    const bool tile_path = !binned && safe && g.n <= 64 && tile_lds <= 64 * 1024;

    // A frame reads the scene and writes the caller's planes plus its stream's own tables, counters and depth-of-field
    // planes, so frames may overlap (call_begin).
    call_begin();
    g.pending_is_rt = true;
    g.pending_primary = (uint64_t)view->width * (uint64_t)(y1 - y0) * (uint64_t)((g.aa > 1 ? g.aa : 1) * (g.aa > 1 ? g.aa : 1));
    g.pending_nlights = light_positions;
    g.stats.mode_used = MIRT_RT_BRUTE;
    g.pending_empty = (y1 == y0);
    g.pending_counted = false;
    if (y1 == y0) { call_end(); return MIRT_OK; }
    // hit counters: the stream's two buffers in turn (the tile kernel clears the one the stream's next frame will use)
    StreamState &ss = g.cur();
    ss.hits_tog ^= 1;
    g.d_hits = ss.d_hits[ss.hits_tog];
    f.hit_count = g.d_hits;
    OriginTables &S = ss.tabs;
    if (!tile_path) {                            // origin tables of this stream, sized for the scene and the light positions
        if ((rc = S.ensure_cam_rows())) return rc;
        if (!binned && (nlights > S.light_tab_lights || S.light_tab_n != g.n)) {   // (binned frames read the shared light cache)
            if ((rc = dev_grow(&S.d_light_tab, &S.light_tab_lights, nlights, (size_t)nlights * g.n, false))) return rc;
            S.light_tab_n = g.n;
        }
        if (!S.d_origins) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&S.d_origins), sizeof(float) * 3 * (1 + MIRT_MAX_LIGHTS)));
        if (!S.d_flags) { HIP_TRY(hipMalloc(reinterpret_cast<void **>(&S.d_flags), 16)); HIP_TRY(hipMemsetAsync(S.d_flags, 0, 16, g.stream)); }
    }
    f.cam_tab = S.d_cam_tab;
    f.light_tab = S.d_light_tab;
    f.unsafe = S.d_flags;
    if (deferred) {
        // the planes the records are made from: the caller's, or the stream's own where the caller asked for none (the kernels
        // index them with full-frame pixel numbers: the bases are shifted so that row y0 is the first stored)
        ManyLightsScratch &M = ss.many;
        if ((rc = M.ensure((size_t)view->width * (size_t)(y1 - y0)))) return rc;
        const ptrdiff_t shift = (ptrdiff_t)y0 * view->width;
        if (!f.index) f.index = M.d_index - shift;
        if (!f.dist) f.dist = M.d_dist - shift;
        if (!f.pos) f.pos = M.d_pos - 3 * shift;
    }

    if (binned) {
        BinnedPass bp;
        if ((rc = binned_pass(view, ss, origins, nlights, y0, y1, &bp)) || (rc = binned_trace(f, ss, bp))) return rc;
    } else if ((rc = rt_dispatch_brute(f, view, S, origins, nlights, safe, tile_path, tile_lds))) {
        return rc;
    }
    if (deferred && (rc = deferred_lights(f, lights, light_positions, mode))) return rc;
    call_end();
    return MIRT_OK;
}

}  // namespace mirt

extern "C" int mirt_set_supersampled_many_lights(int on)
{
    int rc;
    if ((rc = mirt::need_init())) return rc;
    mirt::g.aa_many_lights = on != 0;
    return MIRT_OK;
}

extern "C" int mirt_get_supersample_stats(uint64_t *hit_subrays, uint64_t *records_shaded)
{
    using namespace mirt;
    int rc;
    if ((rc = need_init())) return rc;
    if (!hit_subrays || !records_shaded) return fail(MIRT_ERR_INVALID_ARGUMENT, "hit_subrays / records_shaded must not be NULL");
    unsigned long long c[2] = { 0ull, 0ull };
    if (g.aa_stats_dev) {
        HIP_TRY(hipStreamSynchronize(g.aa_stats_stream));
        HIP_TRY(hipMemcpy(c, g.aa_stats_dev, sizeof c, hipMemcpyDeviceToHost));
    }
    *hit_subrays = c[0];
    *records_shaded = c[1];
    return MIRT_OK;
}
