// delivery.cpp -- how a frame reaches the caller beyond the device planes: staging planes and registered host surfaces for the
// host-buffer entry points, the planes of asynchronous frames, and the depth-of-field resolve (capi.hpp: deliver_host,
// deliver_async, render_with_dof).
#include "capi.hpp"

namespace mirt {

int ensure_staging(size_t px, const HostPlane *planes, int nplanes)
{
    // All staging planes share ONE capacity (g.cap_px pixels): a plane that is first needed by a small frame must
    // still be big enough for every frame size the other planes were already grown to.
    if (px > g.cap_px) {
        for (void **p : { &g.d_xrgb, &g.d_rgb, &g.d_index, &g.d_zinv, &g.d_pos }) { if (*p) (void)hipFree(*p); *p = nullptr; }
        g.cap_px = px;
    }
    int rc;
    if (!g.d_xrgb && (rc = dev_realloc_bytes(&g.d_xrgb, g.cap_px * 4))) return rc;
    for (int i = 0; i < nplanes; i++)
        if (planes[i].host && !*planes[i].staging && (rc = dev_realloc_bytes(planes[i].staging, g.cap_px * planes[i].bpp))) return rc;
    return MIRT_OK;
}

// The device alias of a host pointer inside a registered surface (rows [0, H) of `pitch` bytes must fit), or NULL.
char *registered_alias(const void *host, size_t pitch, int H)
{
    const char *p = static_cast<const char *>(host);
    for (const Ctx::HostSurface &r : g.surf)
        if (r.host && p >= r.host && p + pitch * (size_t)H <= r.host + r.bytes) return r.dev + (p - r.host);
    return nullptr;
}

// How a frame reaches a REGISTERED host surface: 0 (default) = device staging plane + one DMA copy into the pinned surface,
// 1 = the render kernels store their XRGB words straight into the mapped surface (no staging plane, no copy; the stores cross
// the link while the frame is still being computed).  MIRT_HOST_PATH=direct|dma.  Measured on the MI355X box (bench.py
// host_path): 1080p ray tracer 0.226 (dma) / 0.230 (direct) / 0.224 ms (unregistered, pageable) per frame, 4K rasteriser
// 0.71 (pageable) / 0.90 ms (direct) -- the runtime's own staging of pageable copies already runs at the rate the link gives
// here (37-46 GB/s), so registering buys nothing on this machine and direct stores lose to the DMA engine on large frames.
bool host_direct()
{
    static const bool direct = env_is("MIRT_HOST_PATH", "direct");
    return direct;
}

int copy_plane_interior(void *dst, int dst_pitch, const void *src, int src_pitch, int W, int H)
{
    // rows 1..H-2, columns 1..W-2 only: the reference never writes the 1-pixel border (raytracer.cpp:618-620)
    if (W < 3 || H < 3) return MIRT_OK;
    HIP_TRY(hipMemcpy2DAsync(static_cast<char *>(dst) + dst_pitch + 4, dst_pitch,
                             static_cast<const char *>(src) + src_pitch + 4, src_pitch,
                             (size_t)(W - 2) * 4, H - 2, hipMemcpyDeviceToHost, g.stream));
    return MIRT_OK;
}

// One XRGB plane per stream for the asynchronous entry points -- the frame that reuses a plane is queued on the stream whose copy
// engine read it last, so the render is ordered after that copy whatever other calls came in between.
int async_plane(size_t px, void **plane)
{
    if (px > g.async_cap_px) {
        HIP_TRY(sync_all());                                 // frames in flight may still read the planes
        for (StreamState &ss : g.streams) { if (ss.d_async) (void)hipFree(ss.d_async); ss.d_async = nullptr; }
        g.async_cap_px = 0;
        for (StreamState &ss : g.streams)
            if (dev_realloc_bytes(&ss.d_async, px * 4)) return fail(MIRT_ERR_OUT_OF_MEMORY, "hipMalloc(%zu bytes) for an asynchronous frame", px * 4);
        g.async_cap_px = px;
    }
    *plane = g.streams[next_si()].d_async;                   // the plane of the stream this frame is about to take
    return MIRT_OK;
}

int async_target(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect, uint32_t *out_xrgb, int pitch_bytes, char **alias)
{
    int rc;
    if ((rc = check_frame_args(view, lights, nlights, indirect, out_xrgb, pitch_bytes))) return rc;
    *alias = registered_alias(out_xrgb, (size_t)pitch_bytes, view->height);
    if (!*alias) return fail(MIRT_ERR_INVALID_ARGUMENT, "an asynchronous frame needs a surface registered with mirt_surface_register (pageable memory cannot take a stream-ordered copy)");
    return MIRT_OK;
}

int DofPlanes::ensure(size_t px)
{
    if (px <= cap_px) return MIRT_OK;
    release();
    if (dev_realloc(&rgb, px * 3) || dev_realloc(&fd, px) || dev_realloc(&xrgb, px) || dev_realloc(&index, px) || dev_realloc(&zinv, px))
        return fail(MIRT_ERR_OUT_OF_MEMORY, "depth-of-field planes (%zu pixels)", px);
    cap_px = px;
    return MIRT_OK;
}

void DofPlanes::release()
{
    for (void *p : { (void *)rgb, (void *)fd, (void *)xrgb, (void *)index, (void *)zinv }) if (p) (void)hipFree(p);
    *this = DofPlanes();
}

// The blur of rows [y0, y1) -- rendered with their halo [ry0, ry1) into D -- into the caller's surface, and the band's rows of the
// other planes the caller asked for (render_with_dof).
int dof_resolve(const DofPlanes &D, const mirt_view *view, int y0, int y1, int row_origin, int ry0, int ry1, void *d_xrgb, int pitch_bytes,
                void *user_rgb, void *user_index, void *user_zinv, bool clear_border)
{
    if (y1 <= y0) return MIRT_OK;
    const int W = view->width;
    const ptrdiff_t shift = (ptrdiff_t)ry0 * W;
    StreamState &ss = g.cur();
    DofFrame d;
    d.rgb = D.rgb - 3 * shift; d.fd = D.fd - shift; d.W = W; d.H = view->height; d.K = g.dof_k;
    d.y0 = y0; d.y1 = y1; d.row_origin = row_origin; d.ry0 = ry0; d.ry1 = ry1;
    d.xrgb = static_cast<uint32_t *>(d_xrgb); d.pitch_words = pitch_bytes / 4; d.clear_border = clear_border ? 1 : 0;
    k_begin(MIRT_K_DOF);
    launch_dof(d, g.stream);
    k_end(MIRT_K_DOF);
    HIP_TRY(hipGetLastError());
    const size_t rows = (size_t)(y1 - y0), off = (size_t)(y0 - ry0) * W, uoff = (size_t)y0 * W;
    if (user_rgb) HIP_TRY(hipMemcpyAsync((float *)user_rgb + 3 * uoff, D.rgb + 3 * off, rows * W * 12, hipMemcpyDeviceToDevice, g.stream));
    if (user_index) HIP_TRY(hipMemcpyAsync((int32_t *)user_index + uoff, D.index + off, rows * W * 4, hipMemcpyDeviceToDevice, g.stream));
    if (user_zinv) HIP_TRY(hipMemcpyAsync((float *)user_zinv + uoff, D.zinv + off, rows * W * 4, hipMemcpyDeviceToDevice, g.stream));
    if (ss.call_timed) (void)hipEventRecord(ss.ev[EV_CALL1], g.stream);   // the call ends after the blur
    return MIRT_OK;
}

}  // namespace mirt
