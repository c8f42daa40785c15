// binned.cpp -- the binned ray tracer's host side: binning passes (selection, pairs, sort, offsets), the light-cube tables (the
// shared cache, or a frame's own pass for lights that move), the tile order, and the trace kernel over them.
#include "capi.hpp"

namespace mirt {

// ---- binned ray tracing ---------------------------------------------------------------------------------------------

int PairList::ensure(size_t cap)
{
    int r;
    if ((r = dev_realloc(&d_entries, cap)) || (r = dev_realloc(&d_pair_keys, cap)) || (r = dev_realloc(&d_pair_vals, cap)) ||
        (r = dev_realloc(&d_sorted_keys, cap)) || (r = dev_realloc(&d_tmp_vals, cap))) { cap_entries = 0; return r; }
    cap_entries = (uint32_t)cap;
    return MIRT_OK;
}

// (BIN_MAX_KEYS, the most sort keys one binning pass may use: cube_plan.hpp)

void PairList::poll()
{
    if (count_pending && hipEventQuery(ev_count) == hipSuccess) {
        known_pairs = *h_count; have_known = true; count_pending = false;
    }
    (void)hipGetLastError();                                 // (hipErrorNotReady of the query is not an error)
}

// (the event that tells a later frame the count has landed is recorded BEHIND the frame's trace kernel: an event record between
// two kernels of the chain is a barrier packet of its own, ~5 us of the single frame's latency)
int PairList::record_count()
{
    if (!count_event_due) return MIRT_OK;
    count_event_due = false;
    HIP_TRY(hipEventRecord(ev_count, g.stream));
    count_pending = true;
    return MIRT_OK;
}

// The one decision about the pass a stream holds.  When NOTHING a pass depends on has changed since the stream's last one -- the
// view stands still while a light key, a toggle or nothing at all asks for a frame (raytracer.cpp:385-537 set isUpdated without
// touching cameraPos / yaw) -- the stream still holds that pass's tables and the frame starts at the trace kernel
// (MIRT_BIN_REUSE=0: never); the rules: pass_plan.hpp.
PassPlan KeptPass::plan_for(uint64_t key, int mode, PairList &P) const
{
    static const bool reuse_off = env_int("MIRT_BIN_REUSE", 1) == 0;
    P.poll();
    return kept_pass_plan(bin_key_valid, bin_key == key, P.have_known, P.known_pairs > P.cap_used, last_bin_mode == mode, reuse_off);
}

// One binning pass on g.stream: (key, triangle) pairs of `bs`' frames into the pair list S, ordered by key into S.d_entries /
// S.d_sorted_keys, offsets into bin_off.  `counter` (device, zeroed by the caller's previous kernel) receives the pair
// count.  The list is sized from a count only the device knows: it is read back (4 bytes + one sync of this stream) and the
// pass repeated if the list was too small, and *npairs is the count.
// A pass that may not read back (`may_guess`) sizes the list from the count an earlier pass published and publishes its own;
// a list that turns out too small makes the frame's kernels take the brute-force path (k_rt_trace2) and the NEXT pass grow it.
int bin_pass(PairList &S, BinSet bs, const OriginRow *cam_tab, const OriginRow *light_tab, uint32_t *counter, uint32_t *bin_off,
             uint32_t *npairs, bool may_guess = false)
{
    int rc;
    S.count_event_due = false;
    S.poll();                                                // a count an earlier frame left behind?
    const bool guess = may_guess && S.have_known;
    if (!S.d_entries || !S.cap_entries) {
        // first capacity of the pair list (grown on demand below); MIRT_BIN_INITIAL_PAIRS lets a test start small
        static const size_t initial = [] { const long v = env_int("MIRT_BIN_INITIAL_PAIRS", 0); return v > 0 ? (size_t)v : (size_t)1 << 20; }();
        if ((rc = S.ensure(initial))) return rc;
    }
    if (bs.nbins > BIN_MAX_KEYS) return fail(MIRT_ERR_INVALID_ARGUMENT, "binning: %u sort keys exceed the %u the bucket sort holds", bs.nbins, BIN_MAX_KEYS);
    // workgroups striding over the (256-triangle chunk, frame) work items: 8 per CU (52 KiB of LDS and 512 threads each, 3 resident; 1 M
    // triangles at 8K: 4.06 -> 3.53 ms per frame against 3 per CU)
    bs.chunk_tris = 256;                                // (64 measured slower on the 100 k soup: 86 vs 74 us for the whole binning, more flushes)
    const dim3 bin_grid((unsigned)std::min<long long>((long long)((g.n + bs.chunk_tris - 1) / bs.chunk_tris) * bs.nframes, (long long)g.cu_count * 8));
    bs.counters = counter;
    // order the pairs by key with the two-level counting sort (bin_bucket_sort.hip: k_bin_pairs counts the pairs per bucket,
    // two more launches sort)
    const uint32_t nbuckets = bucket_sort_buckets(bs.nbins);
    if (nbuckets + 1 > S.cap_buckets) {
        if ((rc = dev_grow(&S.d_bucket, &S.cap_buckets, nbuckets + 1, (size_t)3 * (nbuckets + 1), false))) return rc;
        HIP_TRY(hipMemsetAsync(S.d_bucket, 0, sizeof(uint32_t) * 3 * (nbuckets + 1), g.stream));
        S.bucket_dirty = false;
    }
    uint32_t *bcnt = S.d_bucket, *bbase = S.d_bucket + S.cap_buckets, *bcur = S.d_bucket + 2 * (size_t)S.cap_buckets;
    bs.bucket_cnt = bcnt; bs.nbuckets = nbuckets; bs.bucket_shift = bucket_sort_shift(bs.nbins);
    const size_t bin_lds = (size_t)nbuckets * sizeof(uint32_t);
    {   // k_bin_pairs: ~52 KB of static LDS + up to 32 KB of bucket counters: past the 64 KB a launch may use by default
        static const bool once = [] {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bin_pairs<512>), hipFuncAttributeMaxDynamicSharedMemorySize, 48 * 1024);
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bin_pairs<256>), hipFuncAttributeMaxDynamicSharedMemorySize, 48 * 1024);
            return true; }();
        (void)once;
    }
    // workgroups of 256 threads where the frame's kernels overlap with its neighbours' -- three or four frames in flight, a scene small
    // enough for that to matter --, of 512 for the large scenes and for the frame that runs alone, whose latency they serve (rt_binned.hip)
    static const int bin_wg_env = (int)env_int("MIRT_BIN_WG", 0);
    const int bin_wg = (bin_wg_env == 256 || bin_wg_env == 512) ? bin_wg_env : ((g.n < 400000 && g.in_flight >= 3) ? 256 : 512);
    // a guessed list: room for half as many pairs again as the last frame seen produced; growing needs this stream idle (rare)
    if (guess && pairs_wanted(S.known_pairs) > S.cap_entries) {
        HIP_TRY(hipStreamSynchronize(g.stream));
        if ((rc = S.ensure(pairs_grown(pairs_wanted(S.known_pairs))))) return rc;
    }
    bool publish_count = false;
    for (int attempt = 0; attempt < 2; attempt++) {
        // MIRT_TEST_PAIR_CAP (tests only): a guessed list pretends to be this small, so that the overflow path runs
        static const uint32_t test_cap = [] { const long v = env_int("MIRT_TEST_PAIR_CAP", 0); return v > 0 ? (uint32_t)v : 0u; }();
        S.cap_used = (guess && test_cap && test_cap < S.cap_entries) ? test_cap : S.cap_entries;
        BinPairs pairs = { S.d_pair_keys, S.d_pair_vals, S.cap_used };
        bs.entries = S.d_entries; bs.cap_entries = S.cap_used;
        if (attempt) HIP_TRY(hipMemsetAsync(counter, 0, 4, g.stream));
        if (attempt || S.bucket_dirty) HIP_TRY(hipMemsetAsync(S.d_bucket, 0, sizeof(uint32_t) * 3 * (size_t)S.cap_buckets, g.stream));
        S.bucket_dirty = true;                               // bucket counts pending until k_bs_local has consumed them
        if (bin_wg == 256) hipLaunchKernelGGL(k_bin_pairs<256>, bin_grid, dim3(256), bin_lds, g.stream, g.d_tris, cam_tab, light_tab, g.n, bs, pairs);
        else hipLaunchKernelGGL(k_bin_pairs<512>, bin_grid, dim3(512), bin_lds, g.stream, g.d_tris, cam_tab, light_tab, g.n, bs, pairs);
        if (guess) {
            // no sync: k_bs_scatter stores the count into a pinned word behind the kernel and a later frame picks it up
            if (!S.h_count) {
                HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&S.h_count), 64, hipHostMallocDefault));
                HIP_TRY(hipEventCreateWithFlags(&S.ev_count, hipEventDisableTiming));
            }
            if (!S.count_pending) publish_count = true;
            *npairs = S.known_pairs;
            break;
        }
        uint32_t total = 0;
        HIP_TRY(hipStreamSynchronize(g.stream));
        HIP_TRY(hipMemcpy(&total, counter, 4, hipMemcpyDeviceToHost));
        *npairs = total;
        S.known_pairs = total; S.have_known = true;
        S.count_pending = false;                             // (a count still on its way belongs to an earlier pass, maybe of another kind)
        if (total <= S.cap_entries) break;
        if (attempt == 1) return fail(MIRT_ERR_HIP, "binning produced %u pairs twice with room for %u", total, S.cap_entries);
        if ((rc = S.ensure(pairs_after_readback(total)))) return rc;
    }
#ifdef MIRT_BIN_STATS
    {
        uint32_t c[16];
        (void)hipMemcpy(c, counter, 64, hipMemcpyDeviceToHost);
        fprintf(stderr, "[mirt bin stats] flattened units=%u max per work item=%u direct items=%u | huge: box valid=%u no box=%u (camera frame %u) waves in the joint test=%u\n", c[8], c[9], c[10], c[11], c[12], c[14], c[15]);
        fprintf(stderr, "[mirt bin stats] tris=%d frames=%d  pairs=%u  bins=%u | large items walked=%u level-1 rounds=%u level-2 steps=%u pairs=%u max steps/item=%u items>100 steps=%u\n",
                g.n, bs.nframes, *npairs, bs.nbins, c[2], c[3], c[4], c[5], c[6], c[7]);
        (void)hipMemset(counter + 2, 0, 56);
    }
#endif
    uint32_t *count_out = nullptr;
    if (publish_count) HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&count_out), S.h_count, 0));
    HIP_TRY(bucket_sort_pairs(S.d_pair_keys, S.d_pair_vals, counter, S.cap_used, *npairs, bs.nbins, S.d_sorted_keys, S.d_tmp_vals,
                              bcnt, bbase, bcur, bin_off, S.d_entries, g.cu_count, g.stream, count_out));
    S.bucket_dirty = false;                                  // k_bs_local leaves the counts and cursors zero
    S.count_event_due = publish_count;                       // (record_count, behind the frame's trace kernel)
    return MIRT_OK;
}

// Key of what the light-cube bins depend on: the scene and the light positions.
uint64_t light_key_of(const float *origins, int nlights)
{
    return Fnv(g.scene_version).mix(origins + 3, sizeof(float) * 3 * nlights).mix(&nlights, 4).mix(&g.n, 4).h;
}

// (shell_range, fill_light_frames and the shell counts' rules: pass_plan.hpp)
int light_shells_for(int nlights, int cube_bins, uint32_t keys_in_front)
{
    static const int env = (int)env_int("MIRT_LIGHT_SHELLS", 0);
    return light_shells_rule(nlights, cube_bins, keys_in_front, env);
}

// Room for the face lists of `nlights` light cubes (k_select_faces) in a stream's light pass; the stream must be idle when they grow.
int ensure_face_lists(LightPass &S, int nlights)
{
    int rc;
    // the light pass's counters and the face lists' lengths in ONE block (a pass zeroes it with one fill): words 0..127 as in the
    // camera's block, 128.. the face counts
    if ((rc = S.ensure_counters(LIGHT_COUNTER_BYTES))) return rc;
    S.d_face_counts = S.d_bin_counters + 128;
    const size_t want = (size_t)6 * (size_t)nlights * (size_t)g.n;
    if (want > S.cap_face_sel && (rc = dev_grow(&S.d_face_sel, &S.cap_face_sel, want, want, true))) return rc;
    return MIRT_OK;
}

// The build chain of `nlights` light cubes on g.stream in the light pass S, from the descriptors and origins the caller has
// uploaded: the lights' origin rows into light_tab and per face the triangles it can see (k_select_faces), then the binning pass
// over those lists -- nkeys keys, offsets into bin_off, the pair count into `counter` (zeroed by the caller) and *npairs.
static int cube_bin_chain(LightPass &S, const BinFrameDesc *d_frames, const float *d_origins, int nlights, uint32_t nkeys, OriginRow *light_tab,
                          uint32_t *bin_off, uint32_t *counter, uint32_t *npairs, bool may_guess)
{
    hipLaunchKernelGGL(k_select_faces, dim3((unsigned)std::min<long long>(((long long)g.n + 1023) / 1024, (long long)g.cu_count), nlights), dim3(1024), 0, g.stream,
                       g.d_tris, g.n, d_origins, d_frames, light_tab, S.d_face_sel, (uint32_t)g.n, S.d_face_counts);
    BinSet bs;
    memset(&bs, 0, sizeof bs);
    bs.frames = d_frames; bs.nframes = 6 * nlights; bs.nbins = nkeys; bs.bin_off = bin_off;
    bs.face_lists = S.d_face_sel; bs.face_counts = S.d_face_counts; bs.face_stride = (uint32_t)g.n;
    return bin_pass(S.pairs, bs, nullptr, light_tab, counter, bin_off, npairs, may_guess);
}

// The SHARED light-cube bins and their expanded rows, for lights that stand still: built on g.stream as a barrier call -- the
// frames of both streams read the tables -- whenever the scene, a light position or the grid differs from what is held.  (Lights
// that just moved do not come here: binned_pass bins their cubes together with the camera frame, on the frame's own stream.)
// C: the frame path's shared cube (g.lc) or the queries' (g.qrows.cube); either is read by the work of every stream.
// shadowed: the cube also gets its covered words (LightCache::d_shadowed) -- the frame path's cube; the queries' cubes have no use for them.
int light_cache_ensure(LightCache &C, LightPass &S, const float *origins, int nlights, int cube_bins, bool *built, bool shadowed)
{
    int rc;
    const uint64_t key = light_key_of(origins, nlights);
    if (built) *built = false;
    if (C.holds(key, cube_bins)) return MIRT_OK;
    if (built) *built = true;
    C.valid = false;
    for (int o = 0; o < g.in_flight; o++)                  // frames of the other streams may still read the old tables
        if (o != g.si) {
            HIP_TRY(hipEventRecord(g.streams[o].ev_order, g.streams[o].stream));
            HIP_TRY(hipStreamWaitEvent(g.stream, g.streams[o].ev_order, 0));
        }
    const int shells = light_shells_for(nlights, cube_bins, 0u);
    const uint32_t per_light = 6u * (uint32_t)(cube_bins * cube_bins) * (uint32_t)shells, nkeys = per_light * (uint32_t)nlights;
    const size_t tab_rows = (size_t)nlights * g.n;
    if (tab_rows > C.cap_tab && (rc = dev_grow(&C.d_light_tab, &C.cap_tab, tab_rows, tab_rows, false))) return rc;
    if (nkeys + 1 > C.cap_bins && (rc = dev_grow(&C.d_off, &C.cap_bins, nkeys + 1, (size_t)nkeys + 1, false))) return rc;
    if (!C.d_frames) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&C.d_frames), sizeof(BinFrameDesc) * 6 * MIRT_MAX_LIGHTS));
    if (!C.d_origins) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&C.d_origins), sizeof(float) * 3 * (1 + MIRT_MAX_LIGHTS)));
    if (!C.d_counter) { HIP_TRY(hipMalloc(reinterpret_cast<void **>(&C.d_counter), 512)); HIP_TRY(hipMemsetAsync(C.d_counter, 0, 512, g.stream)); }   // (k_prep_origin zeroes words 0 and 16..79 of a pass's counter block)   // (ON the stream: see zero-fill note at S.d_bin_counters)
    C.nbins = nkeys;
    C.nrows = 0;
    C.shells = shells;
    C.nlights = nlights; C.n = g.n;
    C.has_shadowed = false;
    if (shadowed && g.n > 0) {                               // (no scene: nothing to allocate or fill, and has_shadowed stays false below)
        // zero on the way: a cube without positions or without a single pair leaves every word clear
        if ((size_t)g.n > C.cap_shadowed && (rc = dev_grow(&C.d_shadowed, &C.cap_shadowed, (size_t)g.n, (size_t)SHADOWED_HEAD + (size_t)g.n, false))) return rc;
        HIP_TRY(hipMemsetAsync(C.d_shadowed, 0, sizeof(uint32_t) * ((size_t)SHADOWED_HEAD + (size_t)g.n), g.stream));
    }
    if (nlights > 0) {
        BinFrameDesc frames[6 * MIRT_MAX_LIGHTS];
        fill_light_frames(frames, origins, nlights, cube_bins, shells, 0u, g.bbox_lo, g.bbox_hi);
        HIP_TRY(upload_small(C.d_frames, frames, sizeof(BinFrameDesc) * 6 * nlights, g.stream));
        HIP_TRY(upload_small(C.d_origins, origins, sizeof(float) * 3 * (1 + nlights), g.stream));
        // the face lists' lengths and the build's pair counter are zeroed on the way
        if ((rc = ensure_face_lists(S, nlights))) return rc;
        HIP_TRY(hipMemsetAsync(S.d_face_counts, 0, sizeof(uint32_t) * 6 * nlights, g.stream));
        HIP_TRY(hipMemsetAsync(C.d_counter, 0, 512, g.stream));
        uint32_t npairs = 0;                                 // (read back: a build never guesses)
        if ((rc = cube_bin_chain(S, C.d_frames, C.d_origins, nlights, nkeys, C.d_light_tab, C.d_off, C.d_counter, &npairs, false))) return rc;
        if (npairs > C.cap_rows) {
            const size_t rows = (size_t)npairs + npairs / 8 + 1024;
            C.cap_rows = 0;
            if ((rc = dev_realloc(&C.d_rows, rows)) || (rc = dev_realloc(&C.d_row_tri, rows))) return rc;
            C.cap_rows = (uint32_t)rows;
        }
        C.nrows = npairs;
        if (npairs)
            hipLaunchKernelGGL(k_expand_light_rows, dim3((unsigned)std::min<uint32_t>((npairs + 255) / 256, 4096u)), dim3(256), 0, g.stream,
                               C.d_off, S.pairs.d_entries, nlights, per_light, C.d_light_tab, g.n, C.d_rows, (const uint32_t *)nullptr, 0u, C.d_row_tri);
        // ... and which triangles one of those rows hides whole from a position (rt_trace.hip): one thread per (triangle, position)
        if (npairs && shadowed)
            hipLaunchKernelGGL(k_shadowed_table, dim3((unsigned)((g.n + 255) / 256), (unsigned)nlights), dim3(256), 0, g.stream,
                               g.d_tris, g.n, C.d_origins, C.d_light_tab, C.d_off, C.d_rows, C.d_frames, cube_bins, shells, C.d_shadowed + SHADOWED_HEAD);
        HIP_TRY(hipGetLastError());
        S.kept = KeptPass();                                 // the stream's pair list now holds the build, a pass of no kind a frame runs
    } else {
        HIP_TRY(hipMemsetAsync(C.d_off, 0, 4, g.stream));
    }
    if (g.in_flight > 1) {                                   // later frames of the other streams wait for the build
        HIP_TRY(hipEventRecord(g.cur().ev_order, g.stream));
        for (int o = 0; o < g.in_flight; o++)
            if (o != g.si) HIP_TRY(hipStreamWaitEvent(g.streams[o].stream, g.cur().ev_order, 0));
    }
    C.key = key;
    C.cube_bins = cube_bins;
    C.has_shadowed = shadowed && g.n > 0;
    C.valid = true;
    return MIRT_OK;
}

// The grid of a light cube: finer grids shorten the shadow lists; the bins are built once per (scene, lights), not per frame, so what
// they cost is memory (48 bytes per (bin, triangle) pair) and ~1 ms of build for 100 k triangles.  Measured on the 100 k soup at 1080p
// (round 2's trace kernel, lists not yet ordered by depth): 64: 153 us, 128: 125 us, 256: 105 us.  MIRT_CUBE_BINS=64|128|256 fixes
// the grid (and keeps every frame on the shared cache).
// (the arithmetic: cube_plan.hpp, cube_bins_rule and cube_keys_fit)
int cube_bins_override()
{
    static const int cube_override = (int)env_int("MIRT_CUBE_BINS", 0);
    return cube_override;
}

int light_cube_bins_for(int nlights, bool *fixed_grid)
{
    return cube_bins_rule(g.n, nlights, cube_bins_override(), fixed_grid);
}

bool light_keys_fit(int nlights, int cube_bins)
{
    return cube_keys_fit(nlights, cube_bins);
}

// A binned frame: camera origin rows, camera-tile bins, trace.  The light-cube bins come from the shared cache when the lights
// stand still -- the only per-frame binning is then the camera's -- or, for lights that moved within the last
// LIGHT_STABLE_FRAMES frames, from this frame's own pass: their cubes (CUBE_BINS_MIN bins per side) are binned TOGETHER with the
// camera frame into the stream's pair list and expanded into the stream's rows.  Nothing of that is shared, so a moving light
// needs no barrier between the streams and no host sync (the list is sized like the camera's: from an earlier frame's count).
// The reference moves the light with keys as readily as the camera (raytracer.cpp:152-162).
constexpr int LIGHT_STABLE_FRAMES = 4;

// The cubes of lights that MOVE, binned by the frame itself (64 x 64 bins per face): a pass of its own in the stream's light
// scratch set L -- the lights' origin rows and per-face selection lists (k_select_faces), pairs, sort, expanded rows --, apart from
// the camera's pass, so that each is kept while only the other one's inputs change: a light key with the camera at rest
// (raytracer.cpp:152-162, 385-537) re-bins the cubes and nothing else; the camera moving under lights that have not settled into the
// shared cube yet re-bins the camera frame and nothing else.  *kept: the pass was not run.
int transient_light_pass(LightPass &L, const float *origins, int nlights, int cube_bins, int tshells, uint32_t per_light, uint64_t lkey, bool *kept,
                         unsigned long long *zero_hits /* nullable: the frame's hit counters, zeroed by the pass's first launch when it runs */)
{
    int rc;
    const uint64_t key = Fnv(g.scene_version).mix(&lkey, 8).mix(&cube_bins, 4).mix(&tshells, 4).mix(&g.n, 4).mix(&nlights, 4).h;
    const PassPlan plan = L.kept.plan_for(key, nlights, L.pairs);
    *kept = plan.reuse;
    if (plan.reuse) return MIRT_OK;
    if ((rc = ensure_face_lists(L, nlights))) return rc;
    if (nlights > L.light_tab_lights || L.light_tab_n != g.n) {
        if ((rc = dev_grow(&L.d_light_tab, &L.light_tab_lights, nlights, (size_t)nlights * g.n, true))) return rc;
        L.light_tab_n = g.n;
    }
    const uint32_t nkeys = per_light * (uint32_t)nlights;
    if (nkeys + 1 > L.cap_bins && (rc = dev_grow(&L.d_bin_off, &L.cap_bins, nkeys + 1, (size_t)nkeys + 1, true))) return rc;
    // frame descriptors of the cubes and the origins in ONE buffer, one upload: [6 * nlights descriptors | (1 + nlights) x 3 floats]
    if (!L.d_frames) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&L.d_frames), sizeof(BinFrameDesc) * (6 * MIRT_MAX_LIGHTS) + sizeof(float) * 3 * (1 + MIRT_MAX_LIGHTS)));
    struct { BinFrameDesc frames[6 * MIRT_MAX_LIGHTS]; float origins[3 * (1 + MIRT_MAX_LIGHTS)]; } up;
    static_assert(sizeof(BinFrameDesc) % 4 == 0, "descriptors are uploaded as words");
    fill_light_frames(up.frames, origins, nlights, cube_bins, tshells, 0u, g.bbox_lo, g.bbox_hi);
    float *d_origins = reinterpret_cast<float *>(L.d_frames + 6 * nlights);
    memcpy(reinterpret_cast<char *>(up.frames + 6 * nlights), origins, sizeof(float) * 3 * (1 + nlights));      // (right behind the descriptors in use)
    // (the same launch zeroes the pass's pair counter and the face lists' lengths)
    const ZeroJob zj = { L.d_bin_counters, (int)(LIGHT_COUNTER_BYTES / 4), reinterpret_cast<uint32_t *>(zero_hits), zero_hits ? 2 * HIT_SHARDS * HIT_SHARD_STRIDE : 0 };
    HIP_TRY(upload_small(L.d_frames, &up, sizeof(BinFrameDesc) * 6 * nlights + sizeof(float) * 3 * (1 + nlights), g.stream, &zj));
    if ((rc = cube_bin_chain(L, L.d_frames, d_origins, nlights, nkeys, L.d_light_tab, L.d_bin_off, L.d_bin_counters, &L.kept.bin_entries, plan.may_guess))) return rc;
    L.kept.keep(key, nlights);
    // one row per pair at most; grown with the pair list (rare)
    if (L.cap_light_rows < L.pairs.cap_entries && (rc = dev_grow(&L.d_light_rows, &L.cap_light_rows, L.pairs.cap_entries, (size_t)L.pairs.cap_entries, true))) return rc;
    const uint32_t expect = std::max<uint32_t>(L.kept.bin_entries, 1u);
    hipLaunchKernelGGL(k_expand_light_rows, dim3((unsigned)std::min<uint32_t>((expect + 255) / 256, 4096u)), dim3(256), 0, g.stream,
                       L.d_bin_off, L.pairs.d_entries, nlights, per_light, L.d_light_tab, g.n, L.d_light_rows, L.d_bin_counters, L.pairs.cap_used, (uint32_t *)nullptr);
    return MIRT_OK;
}

// ---- the camera pass's set-up, shared by a binned frame and a histogram-only pass ----

int OriginTables::ensure_cam_rows() { return cam_tab_n == g.n ? MIRT_OK : dev_grow(&d_cam_tab, &cam_tab_n, g.n, (size_t)g.n, false); }

// Zero-fill ON the stream that uses the buffer: hipMemset runs on the null stream, which the library's non-blocking streams
// are not ordered with -- with several processes on one device (three ranks rehearsing a sharded run) such a fill has been seen
// to land AFTER the first kernels of g.stream had started counting, which cut the pair count short (a light cube built from
// it kept wrong shadows until the lights moved; a camera pass failed with "produced N pairs twice").
int BinPass::ensure_counters(size_t bytes)
{
    if (!d_bin_counters) { HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_bin_counters), bytes)); HIP_TRY(hipMemsetAsync(d_bin_counters, 0, bytes, g.stream)); }
    return MIRT_OK;
}

int CameraPass::ensure_sel()
{
    if (sel_n == g.n) return MIRT_OK;
    kept.forget();
    return dev_grow(&d_sel, &sel_n, g.n, (size_t)g.n, true);
}

SelectOut CameraPass::select_out(const OriginTables &T, int count_word) const
{
    SelectOut so;
    memset(&so, 0, sizeof so);
    so.cam_tab = T.d_cam_tab; so.sel = d_sel;
    so.sel_count = d_bin_counters + count_word; so.sel_count_next = d_bin_counters + (count_word ^ 1);
    return so;
}

// k_prep_select on g.stream: one workgroup of 1024 threads per CU -- a workgroup reserves its slice of the list with ONE atomic
// (rt_binned.hip)
static void launch_prep_select(const BinFrameDesc &frame, const SelectOut &so)
{
    const unsigned sel_grid = (unsigned)std::min<long long>(((long long)g.n + 1023) / 1024, (long long)g.cu_count);
    if (sel_grid) hipLaunchKernelGGL(k_prep_select, dim3(sel_grid), dim3(1024), 0, g.stream, g.d_tris, g.n, frame, so);
}

// The binning pass of a binned frame, up to the trace kernel: the light-cube tables (the shared cache, or this frame's own pass on
// the side stream), then the camera's selection, binning and tile order -- or nothing at all when the stream still holds the pass.
int binned_pass(const mirt_view *view, StreamState &ss, const float *origins, int nlights, int y0, int y1, BinnedPass *bp)
{
    int rc;
    CameraPass &S = ss.cam;
    LightPass &L = ss.lt;
    g.stats.mode_used = MIRT_RT_BINNED;
    g.stats_sel_count = nullptr;
    // light-cube resolution: bins per face side (light_cube_bins_for)
    bool fixed_grid = false;
    const int fine_bins = light_cube_bins_for(nlights, &fixed_grid);

    const uint64_t lkey = light_key_of(origins, nlights);
    if (g.lc.track_key == lkey) g.lc.stable++;
    else { g.lc.track_key = lkey; g.lc.stable = 0; }
    const bool transient = nlights > 0 && !fixed_grid && !g.lc.holds(lkey, fine_bins) && g.lc.stable < LIGHT_STABLE_FRAMES;

    k_begin(MIRT_K_BIN);
    if (!transient && (rc = light_cache_ensure(g.lc, L, origins, nlights, fine_bins, nullptr, true))) return rc;   // (in the light pass's scratch: the camera's tables stay)
    const int cube_bins = transient ? CUBE_BINS_MIN : fine_bins;

    BinSet bs;
    memset(&bs, 0, sizeof bs);
    bs.frame0 = make_camera_frame(view, y0, y1, g.aa);
    bs.frames = nullptr; bs.nframes = 1;
    // (a tile-pair record carries its tile's column and row in 16 bits each: rt_trace.hip)
    if (bs.frame0.nbu > 0xFFFF || bs.frame0.nbv > 0xFFFF) return fail(MIRT_ERR_INVALID_ARGUMENT, "binned frame of %d x %d tiles", bs.frame0.nbu, bs.frame0.nbv);
    // The camera's sort keys are LOCAL to the rows the call renders: tile (i, j) of a band that starts at tile row j0 has bin
    // (j - j0) * nbu + i (the frame's `base` is -j0 * nbu, modulo 2^32), so a band of a sharded frame sorts an eighth of the keys
    // -- buckets an eighth as wide, spread over all the sort's workgroups -- and writes an eighth of the offsets.  (With the whole
    // frame's key space a band's pairs sat in an eighth of the buckets: k_bs_local took 94 us for a middle band of the 1 M-triangle
    // frame at 8K against 112 us for the whole frame.)  The kernels that index the offsets by the frame's tile number get the
    // array's base shifted accordingly (cam_off below).
    const int band_tile_rows = bs.frame0.j1 - bs.frame0.j0;
    const uint32_t key_shift_tiles = (uint32_t)bs.frame0.j0 * (uint32_t)bs.frame0.nbu;
    bs.frame0.base = 0u - key_shift_tiles;
    {
        // depth shells: the tiles' lists come out of the sort roughly front to back (key = bin * shells + shell of the
        // candidate's `near` bound, uniform steps between the nearest and the farthest point of the scene's box)
        static const int shells_env = (int)env_int("MIRT_CAM_SHELLS", 0);
        const int ns = camera_shells_rule((long long)bs.frame0.nbu * band_tile_rows, shells_env);
        double dn = 0.0, df = 0.0;
        const bool okr = shell_range(view->pos, g.bbox_lo, g.bbox_hi, &dn, &df);
        bs.frame0.nshell = okr ? ns : 1;
        bs.frame0.shell_d0 = (float)dn;
        bs.frame0.shell_iw = okr ? (float)(ns / (df - dn)) : 0.0f;
    }
    const uint32_t cam_keys = (uint32_t)bs.frame0.nbu * (uint32_t)band_tile_rows * (uint32_t)bs.frame0.nshell;
    // this frame's own light cubes (moving lights) are a pass of their own, with keys of their own (below)
    const int tshells = transient ? light_shells_for(nlights, cube_bins, 0u) : 1;
    const uint32_t per_light = 6u * (uint32_t)(cube_bins * cube_bins) * (uint32_t)tshells;
    bs.nbins = cam_keys;
    if (bs.nbins + 1 > S.cap_bins) {                         // (a frame of this stream may still read the old array)
        if ((rc = dev_grow(&S.d_bin_off, &S.cap_bins, bs.nbins + 1, (size_t)bs.nbins + 1, true))) return rc;
        S.kept.forget();
    }
    if ((rc = S.ensure_counters(512)) || (rc = S.ensure_sel())) return rc;
    bs.bin_off = S.d_bin_off;

    const uint64_t key = Fnv(g.scene_version).mix(view, sizeof *view).mix(&y0, 4).mix(&y1, 4).mix(&g.n, 4).mix(&g.aa, 4).h;
    const int bin_mode = 0;                                  // (the camera's pass bins the camera frame alone)
    ss.hits_clean[ss.hits_tog] = false;
    if (!S.d_frames) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&S.d_frames), sizeof(BinFrameDesc) * (1 + 6 * MIRT_MAX_LIGHTS)));
    // The pair count is read back (4 bytes + one sync of this stream) only when the inputs that determine it changed AND no
    // count of an earlier pass of the same kind is at hand; and the stream may still hold the whole pass (KeptPass::plan_for).
    const PassPlan plan = S.kept.plan_for(key, bin_mode, S.pairs);
    const uint32_t pairs_x = (uint32_t)((bs.frame0.nbu + 1) / 2);
    uint32_t group_rows[ORDER_GROUPS] = { 0 };
    for (int j = bs.frame0.j0; j < bs.frame0.j1; j++) group_rows[((uint32_t)j >> ORDER_STRIPE_SHIFT) & (ORDER_GROUPS - 1)]++;
    const uint32_t order_seg = pairs_x * *std::max_element(group_rows, group_rows + ORDER_GROUPS);
    const uint32_t *cam_off = S.d_bin_off - (size_t)key_shift_tiles * (size_t)bs.frame0.nshell;   // indexed by the FRAME's tile number
    // The cubes of lights that moved within the last frames: a pass of their own (transient_light_pass), kept while the lights stand
    // still.  When the camera's pass runs as well, the light pass goes FIRST and onto the stream's side stream: the two chains
    // share nothing until the trace kernel and are each bound by the latency of their launches, so side by side they take the longer
    // one's time instead of the sum (one frame in flight, camera and light moving: 0.268 ms one after the other, see
    // profiles/r04_moving_light.txt for the figure side by side).  The side stream starts behind everything the main stream has
    // queued (the previous frame's trace kernel reads the tables the pass rewrites) and is joined in front of this frame's.
    bool lights_kept = false, forked = false;
    if (transient) {
        static const bool side_off = env_int("MIRT_LIGHT_SIDE_STREAM", 1) == 0;
        hipStream_t main_stream = g.stream;
        forked = !plan.reuse && !side_off;
        if (forked) {
            HIP_TRY(hipEventRecord(ss.ev_fork, main_stream));
            HIP_TRY(hipStreamWaitEvent(ss.aux, ss.ev_fork, 0));
            g.stream = ss.aux;
        }
        // (with the camera's pass kept nothing else runs in front of the trace kernel: the light pass's first launch zeroes the hit counters too)
        rc = transient_light_pass(L, origins, nlights, cube_bins, tshells, per_light, lkey, &lights_kept, plan.reuse ? g.d_hits : nullptr);
        g.stream = main_stream;
        if (rc) return rc;
        if (forked) HIP_TRY(hipEventRecord(ss.ev_join, ss.aux));
    }
    if (plan.reuse) {
        // (the first kernel of a pass zeroes the frame's hit counters on the way; here nothing runs in front of the trace kernel --
        // unless the light pass has just run and done it)
        if (!(transient && !lights_kept)) HIP_TRY(hipMemsetAsync(g.d_hits, 0, HIT_BYTES, g.stream));
        g.stats.bins_reused = 1;
    } else {
        // first kernel of the frame: the camera's origin rows for the triangles the rows of this call can see, and their list
        // (k_prep_select); it also zeroes the hit counters and the pass's counters
        S.sel_parity ^= 1;
        SelectOut so = S.select_out(ss.tabs, SEL_COUNT0 + S.sel_parity);
        so.zero_hits = g.d_hits; so.zero_counter = S.d_bin_counters;
        if ((rc = hist_prepare(ss.hist, bs.frame0, &so))) return rc;
        launch_prep_select(bs.frame0, so);
        if ((rc = hist_publish(ss.hist))) return rc;
        bs.sel = S.d_sel; bs.sel_count = so.sel_count;
        g.stats_sel_count = so.sel_count;
        if ((rc = bin_pass(S.pairs, bs, ss.tabs.d_cam_tab, nullptr, S.d_bin_counters, S.d_bin_off, &S.kept.bin_entries, plan.may_guess))) return rc;
        S.kept.keep(key, bin_mode);
        // the order the trace kernel's waves take the tile pairs in: per XCD group (pairs of tile rows dealt round-robin), longest
        // lists first
        if (order_seg > S.cap_order && (rc = dev_grow(&S.d_order, &S.cap_order, order_seg, (size_t)ORDER_GROUPS * ORDER_CLASSES * order_seg, true))) return rc;
        hipLaunchKernelGGL(k_tile_order, dim3((pairs_x + 63) / 64, (unsigned)(bs.frame0.j1 - bs.frame0.j0)), dim3(64), 0, g.stream, cam_off, bs.frame0.nshell,
                           bs.frame0.nbu, bs.frame0.j0, bs.frame0.j1, S.d_bin_counters, S.pairs.cap_used, S.d_order, order_seg);
    }
    if (forked) HIP_TRY(hipStreamWaitEvent(g.stream, ss.ev_join, 0));
    k_end(MIRT_K_BIN);

    bp->cam_off = cam_off;
    bp->tiles_x = bs.frame0.nbu;
    bp->cam_shells = bs.frame0.nshell;
    bp->shell_d0 = bs.frame0.shell_d0; bp->shell_iw = bs.frame0.shell_iw;
    bp->order_seg = order_seg;
    // the light tables: this frame's own pass with its count, or the shared cube's, which are complete by construction -- the trace
    // kernel reads the count with its other counters, without a branch, so it gets a word that is there and a cap no count exceeds
    bp->cube = transient ? cube_view(L, cube_bins, tshells) : cube_view(g.lc);
    bp->light_tab = transient ? L.d_light_tab : g.lc.d_light_tab;
    // The shared cube's covered words (a pixel on a covered triangle has no shadow ray, rt_trace.hip) arrive as that word: the head of
    // their block reads zero.  A frame's own cubes have none; MIRT_TR_SHADOWED=0 hands none over either.
    static const int shadowed_env = (int)env_int("MIRT_TR_SHADOWED", 1);
    bp->shadowed = !transient && shadowed_env != 0 && g.lc.has_shadowed;
    bp->light_pair_count = transient ? L.d_bin_counters : bp->shadowed ? g.lc.d_shadowed : S.d_bin_counters;
    bp->light_pair_cap = transient ? L.pairs.cap_used : 0xFFFFFFFFu;
    return MIRT_OK;
}

// k_prep_select over a frame of no rows, for its histogram of the whole frame, filed like a binned pass's.  It still writes the
// origin rows and the indices of the triangles it cannot rule out into the stream's tables -- the pass the stream held is gone --
// and counts them into words of its own (HIST_SEL_COUNT, zeroed first), so that the selection count of the stream's last binned
// frame, which mirt_get_stats reads, stays what it was.
int hist_only_pass(const mirt_view *view)
{
    int rc;
    g.stream = g.cur().stream;
    StreamState &ss = g.cur();
    CameraPass &S = ss.cam;
    if ((rc = ss.tabs.ensure_cam_rows()) || (rc = S.ensure_sel()) || (rc = S.ensure_counters(512))) return rc;
    S.kept.forget();
    const BinFrameDesc fr = make_camera_frame(view, 0, 0, g.aa);
    SelectOut so = S.select_out(ss.tabs, HIST_SEL_COUNT);
    if ((rc = hist_prepare(ss.hist, fr, &so))) return rc;
    if (!g.hist_armed) return MIRT_OK;
    HIP_TRY(hipMemsetAsync(so.sel_count, 0, 4, g.stream));
    launch_prep_select(fr, so);
    HIP_TRY(hipGetLastError());
    return hist_publish(ss.hist);
}

// The trace kernel of a binned frame over the tables binned_pass left: the camera's in the stream's tables and camera pass, the
// light cubes' as bp's view shows them.
int binned_trace(const RtFrame &f, StreamState &ss, const BinnedPass &bp)
{
    int rc;
    CameraPass &S = ss.cam;
    RtTraceFrame tf;
    memset(&tf, 0, sizeof tf);
    tf.f = f;
    tf.f.cam_tab = ss.tabs.d_cam_tab;
    // (a frame whose pair list overflowed walks the origin tables themselves: every triangle for every ray)
    tf.f.light_tab = bp.light_tab;
    tf.f.unsafe = nullptr;
    tf.cam_off = bp.cam_off;
    tf.cam_entries = S.pairs.d_entries;
    tf.sel = S.d_sel; tf.sel_count = S.d_bin_counters + SEL_COUNT0 + S.sel_parity;
    // geometry rows staged with every candidate while the scene's tables fit the caches, fetched by the exact stage beyond (rt_trace.hip);
    // MIRT_LAZY_GEO=0|1 fixes the choice
    static const int lazy_env = (int)env_int("MIRT_LAZY_GEO", -1);
    const bool lazy_geo = lazy_env >= 0 ? (lazy_env != 0) : (g.n >= 400000);
    tf.geo = g.d_geo;
    tf.shade = g.d_shade;
    tf.light_off = bp.cube.light_off;
    tf.light_rows = bp.cube.light_rows;
    tf.light_tri = bp.cube.light_tri;
    tf.light_frames = bp.cube.light_frames;
    tf.tiles_x = bp.tiles_x;
    tf.cube_bins = bp.cube.cube_bins;
    tf.cam_shells = bp.cam_shells;
    tf.light_shells = bp.cube.shells;
    tf.shell_d0 = bp.shell_d0; tf.shell_iw = bp.shell_iw;
    // a tile's list ends at the depth shell of the tile's farthest record (rt_trace.hip); MIRT_TR_LIST_END=0 walks every list to its end
    static const int list_end_env = (int)env_int("MIRT_TR_LIST_END", 1);
    // (what is uniform per launch -- planes asked for, one sample per light, these two settings -- in one word: csrc/rt_trace_frame.hpp)
    tf.flags = trace_frame_flags(tf.f, lazy_geo, list_end_env != 0, bp.shadowed);
    tf.pair_count = S.d_bin_counters;
    tf.pair_cap = S.pairs.cap_used;
    tf.light_pair_count = bp.light_pair_count;
    tf.light_pair_cap = bp.light_pair_cap;
    // one wave per pair of 8 x 8 tiles
    tf.order = S.d_order; tf.order_count = S.d_bin_counters + 16; tf.order_seg = bp.order_seg;
    // (waves never synchronise with each other: one-wave workgroups are the finest scheduling unit; 84 / 87 / 89 us with 1 / 2 / 4)
    const dim3 tgrid(ORDER_GROUPS * bp.order_seg);          // (workgroup id % 8 = XCD group, id / 8 = the wave among the group's)
    static_assert(TR_WG_WAVES == 1, "the kernel is compiled for one-wave workgroups: 64 threads and one LDS slice per launch below");
    const size_t lds = rt_trace_lds_bytes(1);
    k_begin(MIRT_K_TRACE);
    // (the kernel's own statistics -- tests, candidates, steps, drains -- only for frames rendered with profiling on: rt_trace.hip)
    g.pending_counted = g.profiling;
    if (f.aa > 1) {
        if (g.profiling) hipLaunchKernelGGL((k_rt_trace2<true, true>), tgrid, dim3(64), lds, g.stream, tf);
        else hipLaunchKernelGGL((k_rt_trace2<true, false>), tgrid, dim3(64), lds, g.stream, tf);
    } else {
        // five waves per SIMD (the instantiation held to 96 VGPRs: 92 now) for the large scenes and for the frame that runs alone, four (94 VGPRs) for
        // the small scenes' frames in flight: rt_trace.hip says why; MIRT_TR_WAVES5=0|1 fixes the choice
        static const int waves5_env = (int)env_int("MIRT_TR_WAVES5", -1);
        const bool waves5 = waves5_env >= 0 ? (waves5_env != 0) : (g.n >= 400000 || g.in_flight <= 2);
        if (g.profiling) hipLaunchKernelGGL((k_rt_trace2<false, true>), tgrid, dim3(64), lds, g.stream, tf);
        else if (waves5) hipLaunchKernelGGL((k_rt_trace2<false, false, 5>), tgrid, dim3(64), lds, g.stream, tf);
        else hipLaunchKernelGGL((k_rt_trace2<false, false>), tgrid, dim3(64), lds, g.stream, tf);
    }
    k_end(MIRT_K_TRACE);
    HIP_TRY(hipGetLastError());
    return (rc = S.pairs.record_count()) ? rc : ss.lt.pairs.record_count();
}

}  // namespace mirt

// The shared cube's covered words for one light position, a byte per triangle (1: the frames cast no shadow ray from that triangle
// towards that position).  Waits for everything in flight; an error when no shared cube with the words is held -- before the first
// binned frame, after a scene change or a light move until the cube is back -- or when it holds other positions or triangles.
extern "C" int mirt_get_shadowed(int position, uint8_t *out, int n)
{
    using namespace mirt;
    int rc;
    if ((rc = need_init())) return rc;
    if (!out || n < 0 || position < 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "get shadowed: position %d, %d triangles", position, n);
    const LightCache &C = g.lc;
    if (!C.valid || !C.has_shadowed) return fail(MIRT_ERR_INVALID_ARGUMENT, "get shadowed: no shared light cube is held (render binned frames under lights that stand still first)");
    if (position >= C.nlights || n != C.n) return fail(MIRT_ERR_INVALID_ARGUMENT, "get shadowed: position %d of %d, %d of %d triangles", position, C.nlights, n, C.n);
    HIP_TRY(sync_all());
    std::vector<uint32_t> words((size_t)n);
    if (n) HIP_TRY(hipMemcpy(words.data(), C.d_shadowed + SHADOWED_HEAD, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
    for (int t = 0; t < n; t++) out[t] = (uint8_t)((words[(size_t)t] >> position) & 1u);
    return MIRT_OK;
}
