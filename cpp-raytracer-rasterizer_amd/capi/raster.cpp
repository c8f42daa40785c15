// raster.cpp -- a rasterised frame: its parameter block, the hand-over of the cull flags between the streams' copies, and the
// launch chain (raster_kernels.hip: launch_raster).
#include "capi.hpp"

namespace mirt {

// Orders a WRITE into cull-flag copy `dst`, about to be queued on stream `st`, behind every copy OUT of it that another stream
// still has pending (a rasterised frame that brought the latest flags over to its own copy): a bit per copy and stream says
// which streams have read `dst` since the last writer waited; a stream's event is re-recorded behind each of its reads, and a
// stream runs in order, so waiting for its latest record covers the earlier ones.  Both writers come here: the cull kernel
// (mirt_cull_device) and the hand-over copy of raster_enqueue -- with three or four frames in flight the latter can overwrite a
// copy that a lagging stream is still reading (advisor finding of round 3).
int cull_copy_wait_readers(int dst, hipStream_t st)
{
    for (int r = 0; r < MAX_FLIGHT; r++) {
        StreamState &reader = g.streams[r];
        if ((reader.cull_read_src >> dst & 1u) && r != dst) {
            HIP_TRY(hipStreamWaitEvent(st, reader.ev_cull_read, 0));
            reader.cull_read_src &= ~(1u << dst);
        }
    }
    return MIRT_OK;
}

int raster_enqueue(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                   int y0, int y1, int row_origin, void *d_xrgb, int pitch_bytes, void *d_rgb, void *d_zinv,
                   void *d_index, void *d_fd)
{
    int rc;
    if ((rc = check_frame_args(view, lights, nlights, indirect, d_xrgb, pitch_bytes, true, y0, y1))) return rc;

    // A rasteriser frame touches the scene (read only) and its stream's own scratch and depth-of-field planes, so frames
    // may overlap (call_begin).
    call_begin();
    StreamState &ss = g.cur();
    if (ss.culled_ver != g.streams[g.culled_latest].culled_ver) {
        // the most recent cull flags sit in another stream's copy (mirt_cull_device wrote them for the call it expected next,
        // and a ray-traced frame took that turn): bring them over, ordered after the cull kernel
        const int from = g.culled_latest;
        HIP_TRY(hipStreamWaitEvent(g.stream, g.streams[from].ev_order, 0));
        if ((rc = cull_copy_wait_readers(g.si, g.stream))) return rc;   // ... and after any stream still copying OUT of this stream's copy
        HIP_TRY(hipMemcpyAsync(g.d_culled + (size_t)g.si * g.n, g.d_culled + (size_t)from * g.n, (size_t)g.n, hipMemcpyDeviceToDevice, g.stream));
        ss.culled_ver = g.streams[from].culled_ver;
        HIP_TRY(hipEventRecord(ss.ev_cull_read, g.stream));            // (a later cull step into copy `from` must not overtake this read)
        ss.cull_read_src |= 1u << from;
    }
    g.pending_is_rt = false;
    if (y1 == y0) { call_end(); return MIRT_OK; }

    RasterFrame f;
    memset(&f, 0, sizeof f);
    f.tris15 = g.d_tris;
    f.culled = g.d_culled + (size_t)g.si * g.n;
    f.n = g.n;
    memcpy(f.cam, view->pos, 12);
    memcpy(f.rot, view->rot, 36);
    mat3_inverse(view->rot, f.invrot);        // glm::inverse(cameraRot), hoisted out of PixelShader (rasteriser.cpp:559)
    f.focal = view->focal;
    f.W = view->width; f.H = view->height;
    f.nlights = nlights;
    for (int k = 0; k < nlights; k++) {
        memcpy(f.lpos[k], lights[k].pos, 12);
        for (int c = 0; c < 3; c++) f.lcol[k][c] = lights[k].color[c] * lights[k].intensity;   // rasteriser.cpp:576
    }
    f.lights_in_range = 1;
    for (int k = 0; k < nlights; k++) f.lights_in_range &= light_colour_in_range(f.lcol[k]) ? 1 : 0;
    memcpy(f.indirect, indirect, 12);
    f.y0 = y0; f.y1 = y1; f.row_origin = row_origin;
    f.xrgb = static_cast<uint32_t *>(d_xrgb);
    f.pitch_words = pitch_bytes / 4;
    f.rgb = static_cast<float *>(d_rgb);
    f.zinv = static_cast<float *>(d_zinv);
    f.index = static_cast<int32_t *>(d_index);
    f.fd = static_cast<float *>(d_fd);
    f.focal_plane = g.dof_focal;
    if ((rc = raster_scratch_ensure(ss.raster, g.n, view->width, y1 - y0))) return fail(rc, "raster scratch allocation failed");
    g.raster_since_sync = true;
    {
        static const int edge_env = (int)env_int("MIRT_EDGE_SEGMENTS", -1);
        f.edge_segments = edge_env >= 0 ? edge_env : (g.in_flight <= 2 ? 1 : 0);       // (2: tests -- a spoilt prediction in every chain)
    }
    if ((rc = launch_raster(f, ss.raster, g.scene_version * 0x9E3779B97F4A7C15ull + g.cull_version, g.stream, g.profiling ? &ss.ev[EV_K0] : nullptr,
                            g.profiling ? ss.ev_used : nullptr)))
        return fail(rc, "rasteriser launch failed: %s", hipGetErrorString(hipGetLastError()));
    call_end();
    return MIRT_OK;
}

}  // namespace mirt
