// state.cpp -- the library's state (capi.hpp): what each part of it owns and gives back (create / release; a buffer is freed
// by the struct that holds its pointer), and what every device call does with it: the argument checks, the stream it takes, its
// start and its end.
#include "capi.hpp"

namespace mirt {

int dev_realloc_bytes(void **p, size_t bytes)
{
    if (*p) { (void)hipFree(*p); *p = nullptr; }
    if (bytes == 0) return MIRT_OK;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { *p = nullptr; return fail(MIRT_ERR_OUT_OF_MEMORY, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e)); }
    return MIRT_OK;
}

int check_frame_args(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect, const void *xrgb, int pitch_bytes,
                     bool need_scene, int y0, int y1)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (!view || !indirect) return fail(MIRT_ERR_INVALID_ARGUMENT, "view / indirect must not be NULL");
    if (view->width < 1 || view->height < 1 || view->width > 32768 || view->height > 32768)
        return fail(MIRT_ERR_INVALID_ARGUMENT, "frame size %dx%d out of range [1,32768]", view->width, view->height);
    if (nlights < 0 || nlights > MIRT_MAX_LIGHTS) return fail(MIRT_ERR_INVALID_ARGUMENT, "nlights %d out of range [0,%d]", nlights, MIRT_MAX_LIGHTS);
    if (nlights > 0 && !lights) return fail(MIRT_ERR_INVALID_ARGUMENT, "lights must not be NULL when nlights > 0");
    if (need_scene && g.n <= 0) return fail(MIRT_ERR_NO_SCENE, "no scene uploaded (mirt_scene_upload)");
    if (!xrgb) return fail(MIRT_ERR_INVALID_ARGUMENT, "xrgb output must not be NULL");
    if (y0 < 0 || y1 > view->height || y0 > y1) return fail(MIRT_ERR_INVALID_ARGUMENT, "row band [%d,%d) outside [0,%d)", y0, y1, view->height);
    if (pitch_bytes < view->width * 4 || (pitch_bytes & 3)) return fail(MIRT_ERR_INVALID_ARGUMENT, "pitch %d bytes too small for width %d or not a multiple of 4", pitch_bytes, view->width);
    return MIRT_OK;
}

// Waits for every call enqueued so far (all streams).
hipError_t sync_all()
{
    hipError_t e = hipSuccess;
    for (const StreamState &ss : g.streams)
        if (ss.stream) { const hipError_t r = hipStreamSynchronize(ss.stream); if (r != hipSuccess) e = r; }
    for (const StreamState &ss : g.streams)
        if (ss.aux) { const hipError_t r = hipStreamSynchronize(ss.aux); if (r != hipSuccess) e = r; }
    if (g.comm_stream) { const hipError_t r = hipStreamSynchronize(g.comm_stream); if (r != hipSuccess) e = r; }
    return e;
}

// The stream the NEXT device call will take: calls take the in_flight streams in turn.
int next_si() { return g.in_flight > 1 ? (g.si + 1) % g.in_flight : 0; }

// Every device call starts here.  With several frames in flight consecutive calls take the streams in turn, so frame i+1 is
// dispatched -- and its kernels run, where the device has room -- while frame i still drains: no dispatch gap, no idle tail,
// and the latency-bound chains of consecutive frames (binning, sort, trace; vertex, edges, fragments, resolve) fill each
// other's gaps.  A frame reads the scene and writes the caller's planes plus its OWN stream's state (origin tables, bins,
// raster keys, depth-of-field planes, counters), so frames need no ordering among themselves; frames i and i + in_flight,
// which a caller cycling through in_flight sets of planes gives the same planes, share a stream.
void stream_begin()
{
    g.si = next_si();
    g.stream = g.cur().stream;
    g.frame_no++;
    (void)hipGetLastError();                     // drop a stale error of another HIP user in this thread (torch polls events:
                                                 // hipErrorNotReady) so that the launch checks below report our own launches only
}
void call_begin()
{
    stream_begin();
    StreamState &ss = g.cur();
    memset(&g.stats, 0, sizeof g.stats);
    g.stats_sel_count = nullptr;
    g.ev_cur = g.si;
    memset(ss.ev_used, 0, sizeof ss.ev_used);
    // the call's own start / end events only when profiling is on: an event record costs ~2.7 us of host time, a quarter of
    // a 500 x 500 Cornell frame (12.9 -> 7.x us per frame without the two of them)
    ss.call_timed = g.profiling;
    if (ss.call_timed) (void)hipEventRecord(ss.ev[EV_CALL0], g.stream);
}
void call_end() { if (g.cur().call_timed) (void)hipEventRecord(g.cur().ev[EV_CALL1], g.stream); g.stats_stream = g.stream; g.stats_pending = true; }

// ---- what the state owns ----------------------------------------------------------------------------------------
// (a buffer is freed by the struct that holds its pointer)

static void dev_free(std::initializer_list<void *> ptrs) { for (void *p : ptrs) if (p) (void)hipFree(p); }

void OriginTables::release() { dev_free({ d_cam_tab, d_light_tab, d_origins, d_flags }); *this = OriginTables(); }

void PairList::release()
{
    dev_free({ d_entries, d_pair_keys, d_pair_vals, d_sorted_keys, d_tmp_vals, d_bucket });
    if (h_count) (void)hipHostFree(h_count);
    if (ev_count) (void)hipEventDestroy(ev_count);
    *this = PairList();
}

void CameraPass::release() { pairs.release(); dev_free({ d_bin_off, d_bin_counters, d_frames, d_sel, d_order }); *this = CameraPass(); }

// (d_face_counts lies inside d_bin_counters' block)
void LightPass::release() { pairs.release(); dev_free({ d_bin_off, d_bin_counters, d_frames, d_face_sel, d_light_tab, d_light_rows }); *this = LightPass(); }

void CostHist::release()
{
    dev_free({ d_hist });
    if (h_hist) (void)hipHostFree(h_hist);
    for (hipEvent_t e : ev_hist) if (e) (void)hipEventDestroy(e);
    *this = CostHist();
}

void QueryScratch::release()
{
    dev_free({ d_light_tab, d_origins, d_flags, d_stats[QUERY_DIRECT_LIGHT], d_stats[QUERY_FAN], d_stats[QUERY_OCCLUDED], d_stats[QUERY_SHADOW_MASK], d_stats[QUERY_ALONG], d_fan_origins, d_fan_rays, d_carry,
               d_relight, d_order_after });
    *this = QueryScratch();
}

int ManyLightsScratch::ensure(size_t px)
{
    int rc;
    if (px <= cap_px) return MIRT_OK;
    HIP_TRY(hipStreamSynchronize(g.stream));     // an earlier frame of the stream may still read the old buffers
    cap_px = 0;
    if ((rc = dev_realloc(&d_records, px * HIT_WORDS)) || (rc = dev_realloc(&d_direct, px * 3)) || (rc = dev_realloc(&d_carry, px * LIGHT_CARRY_WORDS)) ||
        (rc = dev_realloc(&d_index, px)) || (rc = dev_realloc(&d_dist, px)) || (rc = dev_realloc(&d_pos, px * 3))) return rc;
    cap_px = px;
    return MIRT_OK;
}

void ManyLightsScratch::release()
{
    dev_free({ d_records, d_direct, d_carry, d_index, d_dist, d_pos });
    *this = ManyLightsScratch();
}

int AaScratch::ensure(size_t px, size_t rec)
{
    int rc;
    if (!d_cursor) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_cursor), 16));
    if (!d_stats) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_stats), 16));
    if (px <= cap_px && rec <= cap_rec) return MIRT_OK;
    HIP_TRY(hipStreamSynchronize(g.stream));     // an earlier frame of the stream may still read the old buffers
    px = std::max(px, cap_px); rec = std::max(rec, cap_rec);
    cap_px = cap_rec = 0;
    if ((rc = dev_realloc(&d_records, rec * HIT_WORDS)) || (rc = dev_realloc(&d_direct, rec * 3)) || (rc = dev_realloc(&d_carry, rec * LIGHT_CARRY_WORDS)) ||
        (rc = dev_realloc(&d_slots, rec)) || (rc = dev_realloc(&d_counts, rec)) || (rc = dev_realloc(&d_nver, px))) return rc;
    cap_px = px; cap_rec = rec;
    return MIRT_OK;
}

void AaScratch::release()
{
    dev_free({ d_records, d_direct, d_carry, d_slots, d_counts, d_nver, d_cursor, d_stats });
    *this = AaScratch();
}

void QueryRows::release()
{
    dev_free({ d_rows, d_max, d_rays, d_hits, d_rgb, d_dirs, d_origin_of, d_limits, d_occluded, d_mask, d_order_after, d_order_counts, d_order_hits });
    if (ev_built) (void)hipEventDestroy(ev_built);
    for (LightCache &c : cubes) c.release();
    fan.release();
    aa_cam.release();
    for (LightCache &c : fans) c.release();
    along.release();
    for (AlongsGroup &a : alongs) a.release();
    alongs_build.release();
    grid.release();
    *this = QueryRows();
}

void AlongCache::release()
{
    dev_free({ d_off, d_rows, d_aux, d_near, d_counters, d_keys, d_vals, d_tmp_keys, d_tmp_vals, d_entries, d_bucket });
    *this = AlongCache();
}

void RayGridCache::release()
{
    dev_free({ d_off, d_rows, d_counters, d_keys, d_vals, d_tmp_keys, d_tmp_vals, d_entries, d_bucket });
    for (unsigned long long *p : d_stats) dev_free({ p });
    *this = RayGridCache();
}

void AlongsGroup::release()
{
    dev_free({ d_descs, d_dirs, d_off, d_rows, d_aux });
    *this = AlongsGroup();
}

void AlongsBuild::release()
{
    dev_free({ d_near, d_counters, d_keys, d_vals, d_tmp_keys, d_tmp_vals, d_entries, d_bucket });
    *this = AlongsBuild();
}

void LightCache::release() { dev_free({ d_light_tab, d_frames, d_off, d_rows, d_row_tri, d_origins, d_counter, d_shadowed }); *this = LightCache(); }

int StreamState::create()
{
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&ev_order, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ev_cull_read, hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithFlags(&aux, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    return MIRT_OK;
}

void StreamState::release()
{
    tabs.release();
    cam.release();
    lt.release();
    hist.release();
    raster_scratch_free(raster);
    query.release();
    many.release();
    aa.release();
    dof.release();
    dev_free({ d_hits[0], d_hits[1], d_tile_tab, d_async });
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : { ev_order, ev_cull_read, ev_fork, ev_join }) if (e) (void)hipEventDestroy(e);
    if (aux) (void)hipStreamDestroy(aux);
    if (stream) (void)hipStreamDestroy(stream);
    *this = StreamState();
}

}  // namespace mirt
