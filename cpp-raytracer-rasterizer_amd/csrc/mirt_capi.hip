// mirt_capi.hip -- the C-ABI of include/mirt.h on top of the HIP kernels: the library's lifetime, settings, statistics and
// every extern "C" entry point but the ray queries' (../capi/query.cpp).  The orchestration behind them -- ray-traced and rasterised frames, binning, delivery, sharded
// frames -- lives in ../capi/ (capi.hpp: the state, one StreamState per frame in flight).  No CPU fallback: without a gfx950
// device every compute entry point returns MIRT_ERR_NO_DEVICE.
#include "../capi/capi.hpp"

#include <unistd.h>

namespace mirt {

char g_err[512] = "no error";
Ctx g;

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

namespace {

// Small parameter blocks for the device (frame descriptors, ray origins): the words travel in the KERNEL ARGUMENTS of a one-
// workgroup kernel, which the launch copies before it returns -- ordered on the stream like any kernel and independent of when
// the runtime reads a pageable or stack source (hipMemcpyAsync from such memory leaves that to its staging policy).
struct UploadChunk { uint32_t w[768]; };
__global__ __launch_bounds__(256) void k_upload_words(const UploadChunk c, uint32_t *__restrict__ dst, int nwords)
{
    for (int i = threadIdx.x; i < nwords; i += 256) dst[i] = c.w[i];
}
// ... and, in the same launch, up to two regions to zero (a pass's counters, the frame's hit counters): a fill of its own is a launch
// of its own, ~3 us of a single frame's latency each.
__global__ __launch_bounds__(256) void k_upload_words_zero(const UploadChunk c, uint32_t *__restrict__ dst, int nwords, const ZeroJob z)
{
    for (int i = threadIdx.x; i < nwords; i += 256) dst[i] = c.w[i];
    for (int i = threadIdx.x; i < z.na; i += 256) z.a[i] = 0u;
    for (int i = threadIdx.x; i < z.nb; i += 256) z.b[i] = 0u;
}

// The cost histogram of a pass leaves the device behind k_prep_select: its words go to a pinned copy the host reads later
// (weighted partition), and the device words are zero again for the next pass.
__global__ __launch_bounds__(SEL_HIST_MAX) void k_hist_out(uint32_t *__restrict__ hist, uint32_t *__restrict__ host_copy)
{
    host_copy[threadIdx.x] = hist[threadIdx.x];
    hist[threadIdx.x] = 0u;
}

}  // namespace

hipError_t upload_small(void *dst, const void *src, size_t bytes, hipStream_t stream, const ZeroJob *zero)
{
    if (zero) {
        // (the zero job rides on the first chunk)
        const uint32_t *w0 = static_cast<const uint32_t *>(src);
        UploadChunk c0;
        const int n0 = (int)std::min<size_t>(768, bytes / 4);
        memcpy(c0.w, w0, (size_t)n0 * 4);
        hipLaunchKernelGGL(k_upload_words_zero, dim3(1), dim3(256), 0, stream, c0, static_cast<uint32_t *>(dst), n0, *zero);
        if (bytes / 4 <= 768) return hipGetLastError();
        return upload_small(static_cast<uint32_t *>(dst) + 768, w0 + 768, bytes - 768 * 4, stream, nullptr);
    }
    const uint32_t *w = static_cast<const uint32_t *>(src);
    uint32_t *d = static_cast<uint32_t *>(dst);
    for (size_t off = 0, nw = bytes / 4; off < nw; off += 768) {
        UploadChunk c;
        const int n = (int)std::min<size_t>(768, nw - off);
        memcpy(c.w, w + off, (size_t)n * 4);
        hipLaunchKernelGGL(k_upload_words, dim3(1), dim3(256), 0, stream, c, d + off, n);
    }
    return hipGetLastError();
}

// k_hist_out on `stream`: the device words of a cost histogram to a pinned copy, and zero again (hist_publish).
void hist_out(uint32_t *hist, uint32_t *host_copy, hipStream_t stream)
{
    hipLaunchKernelGGL(k_hist_out, dim3(1), dim3(SEL_HIST_MAX), 0, stream, hist, host_copy);
}

int need_init()
{
    if (!g.init) return fail(MIRT_ERR_NOT_INITIALISED, "mirt_init has not been called (or failed)");
    return MIRT_OK;
}

}  // namespace mirt

using namespace mirt;

// ---- lifetime ----------------------------------------------------------------------------------------

extern "C" int mirt_abi_version(void) { return MIRT_ABI_VERSION; }
extern "C" const char *mirt_last_error(void) { return g_err; }

extern "C" int mirt_init(int device)
{
    int rc;
    if (g.init) {
        if (g.device == device) return MIRT_OK;
        mirt_shutdown();
    }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(MIRT_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU path", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= count) return fail(MIRT_ERR_INVALID_ARGUMENT, "device %d out of range [0,%d)", device, count);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MIRT_ERR_NO_DEVICE, "device %d is %s; the kernels in this library are built for gfx950 (MI355X) only", device, prop.gcnArchName);
    HIP_TRY(hipSetDevice(device));
    g.cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    for (StreamState &ss : g.streams)
        if ((rc = ss.create())) return rc;
    // ... and what their frames write, only once every stream exists: the fills below run on the null stream, and the order in
    // which the streams and the null stream come into being decides which hardware queues they share (with the fills between
    // the streams' creation, four frames in flight of host/frame_rate ran at about half their rate)
    for (StreamState &ss : g.streams)
        for (hipEvent_t &e : ss.ev) HIP_TRY(hipEventCreate(&e));
    for (int t = 0; t < 2; t++)
        for (StreamState &ss : g.streams) {
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ss.d_hits[t]), HIT_BYTES));
            HIP_TRY(hipMemset(ss.d_hits[t], 0, HIT_BYTES));   // (mirt_init ends with a device sync)
            ss.hits_clean[t] = true;
        }
    for (StreamState &ss : g.streams)
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ss.d_tile_tab), sizeof(float4) * 64 * (12 + 3 * MIRT_MAX_LIGHTS)));
    g.stream = g.streams[0].stream;
    g.in_flight = 1;
    g.frame_no = 0;
    g.si = 0;
    g.ev_cur = 0;
    g.d_hits = g.streams[0].d_hits[0];
    g.device = device;
    HIP_TRY(hipDeviceSynchronize());             // the null-stream fills above have landed before any stream of ours runs
    g.init = true;
    return MIRT_OK;
}

extern "C" void mirt_shutdown(void)
{
    if (!g.init) return;
    (void)hipSetDevice(g.device);
    (void)sync_all();                            // nothing in flight on any stream (frames, side streams, a gather) reads what is freed below
    comm_destroy(g.comm);
    for (StreamState &ss : g.streams) ss.release();
    g.lc.release();
    g.qrows.release();
    scene_forget_objects();
    for (void *p : { (void *)g.d_tris, (void *)g.d_culled, (void *)g.d_geo, (void *)g.d_shade, (void *)g.d_scene_bounds, (void *)g.d_scene_stage, g.d_xrgb, g.d_rgb, g.d_index, g.d_zinv, g.d_pos,
                     (void *)g.d_band[0], (void *)g.d_band[1] })
        if (p) (void)hipFree(p);
    for (Ctx::HostSurface &r : g.surf) if (r.host) (void)hipHostUnregister(r.host);
    for (hipEvent_t e : { g.ev_rendered, g.ev_sent[0], g.ev_sent[1] }) if (e) (void)hipEventDestroy(e);
    if (g.comm_stream) (void)hipStreamDestroy(g.comm_stream);
    g = Ctx();
}

extern "C" int mirt_set_profiling(int on)
{
    int rc;
    if ((rc = need_init())) return rc;
    g.profiling = on != 0;
    return MIRT_OK;
}

extern "C" int mirt_sync(void)
{
    int rc;
    if ((rc = need_init())) return rc;
    HIP_TRY(sync_all());
    // A rasteriser frame whose row tables were sized from a cached count reports a table that turned out too small in
    // counters[1] (it would have dropped the rows of the triangles that did not fit): surface it here, where the caller
    // waits for its frames, instead of presenting such a frame silently.
    if (g.raster_since_sync) {
        g.raster_since_sync = false;
        for (StreamState &ss : g.streams)
            if (RasterScratch &R = ss.raster; R.counters) {
                uint32_t c[2] = { 0, 0 };
                HIP_TRY(hipMemcpy(c, R.counters, sizeof c, hipMemcpyDeviceToHost));
                if (c[1]) {
                    R.sizing_valid = false;
                    return fail(MIRT_ERR_HIP, "rasteriser: the row tables (%zu rows) were too small for a frame; its sizing cache is dropped, render the frame again", R.cap_rows);
                }
            }
    }
    return MIRT_OK;
}

extern "C" void *mirt_stream(void) { return g.init ? (void *)g.stream : nullptr; }

extern "C" int mirt_set_frames_in_flight(int frames)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (frames < 1 || frames > MAX_FLIGHT) return fail(MIRT_ERR_INVALID_ARGUMENT, "frames in flight must be 1 .. %d, not %d", MAX_FLIGHT, frames);
    HIP_TRY(sync_all());
    if (g.d_culled && g.n > 0) {                 // every stream's copy of the cull flags starts from the most recent ones
        for (int h = 0; h < MAX_FLIGHT; h++)
            if (h != g.culled_latest) {
                HIP_TRY(hipMemcpy(g.d_culled + (size_t)h * g.n, g.d_culled + (size_t)g.culled_latest * g.n, (size_t)g.n, hipMemcpyDeviceToDevice));
                g.streams[h].culled_ver = g.streams[g.culled_latest].culled_ver;
            }
        HIP_TRY(hipDeviceSynchronize());         // (null-stream copies: landed before a frame on one of our streams reads the flags)
    }
    g.in_flight = frames;
    g.si = frames - 1;                           // the first call takes streams[0]
    g.stream = g.streams[0].stream;
    return MIRT_OK;
}

// ---- host surfaces ------------------------------------------------------------------------------------

extern "C" int mirt_surface_register(void *pixels, size_t bytes)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (!pixels || bytes == 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "surface must not be NULL / empty");
    for (Ctx::HostSurface &r : g.surf)
        if (r.host == pixels && r.bytes == bytes) return MIRT_OK;
    Ctx::HostSurface *slot = nullptr;
    for (Ctx::HostSurface &r : g.surf) if (!r.host) { slot = &r; break; }
    if (!slot) return fail(MIRT_ERR_INVALID_ARGUMENT, "at most %d surfaces can be registered at a time", (int)(sizeof g.surf / sizeof g.surf[0]));
    hipError_t e = hipHostRegister(pixels, bytes, hipHostRegisterMapped | hipHostRegisterPortable);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(MIRT_ERR_HIP, "hipHostRegister(%zu bytes): %s", bytes, hipGetErrorString(e)); }
    void *dev = nullptr;
    e = hipHostGetDevicePointer(&dev, pixels, 0);
    if (e != hipSuccess || !dev) { (void)hipHostUnregister(pixels); (void)hipGetLastError(); return fail(MIRT_ERR_HIP, "hipHostGetDevicePointer: %s", hipGetErrorString(e)); }
    slot->host = static_cast<char *>(pixels); slot->dev = static_cast<char *>(dev); slot->bytes = bytes;
    return MIRT_OK;
}

extern "C" int mirt_surface_unregister(void *pixels)
{
    int rc;
    if ((rc = need_init())) return rc;
    for (Ctx::HostSurface &r : g.surf)
        if (r.host && r.host == pixels) {
            HIP_TRY(sync_all());
            (void)hipHostUnregister(r.host);
            r = Ctx::HostSurface();
            return MIRT_OK;
        }
    return fail(MIRT_ERR_INVALID_ARGUMENT, "surface %p is not registered", pixels);
}

// ---- scene ------------------------------------------------------------------------------------------

extern "C" int mirt_scene_upload(const float *tris15, const uint8_t *culled, int n)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (!tris15 || n < 1) return fail(MIRT_ERR_INVALID_ARGUMENT, "scene needs at least one triangle (n = %d)", n);
    HIP_TRY(sync_all());
    g.n = 0;
    scene_forget_objects();                      // (their ranges were checked against the old scene)
    if ((rc = dev_realloc(&g.d_tris, (size_t)n * 15))) return rc;
    if ((rc = dev_realloc(&g.d_culled, (size_t)MAX_FLIGHT * n))) return rc;
    HIP_TRY(hipMemcpy(g.d_tris, tris15, (size_t)n * 15 * sizeof(float), hipMemcpyHostToDevice));
    for (int h = 0; h < MAX_FLIGHT; h++) {
        if (culled) HIP_TRY(hipMemcpy(g.d_culled + (size_t)h * n, culled, (size_t)n, hipMemcpyHostToDevice));
        else HIP_TRY(hipMemset(g.d_culled + (size_t)h * n, 0, (size_t)n));
    }
    if ((rc = dev_realloc(&g.d_geo, (size_t)n))) return rc;
    if ((rc = dev_realloc(&g.d_shade, (size_t)n))) return rc;
    // the copies and fills above ran on the null stream, which the library's non-blocking streams are not ordered with (and a
    // copy from pageable memory may return once the source has been staged): everything has landed before a kernel reads it
    HIP_TRY(hipDeviceSynchronize());
    hipLaunchKernelGGL(k_geo_table, dim3((n + 255) / 256), dim3(256), 0, g.stream, g.d_tris, n, g.d_geo, g.d_shade);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g.stream));
    g.scene_finite = true;
    for (size_t i = 0; i < (size_t)n * 15 && g.scene_finite; i++)
        if (!(fabsf(tris15[i]) < 1.0e8f)) g.scene_finite = false;   // generous: |coord| < 1e8 keeps cross products < 1e18
    for (int c = 0; c < 3; c++) { g.bbox_lo[c] = INFINITY; g.bbox_hi[c] = -INFINITY; }
    for (size_t t = 0; t < (size_t)n; t++)
        for (int v = 0; v < 9; v++) {
            const float x = tris15[t * 15 + v];
            g.bbox_lo[v % 3] = fminf(g.bbox_lo[v % 3], x); g.bbox_hi[v % 3] = fmaxf(g.bbox_hi[v % 3], x);
        }
    g.n = n;
    scene_commit(true);                          // (capi/scene.cpp: shared with the device forms)
    return MIRT_OK;
}

// ---- device-resident scenes (../capi/scene.cpp; the kernels: ../scene/scene_kernels.hip) ---------------------------------

extern "C" int mirt_scene_upload_device(const void *d_tris15, const void *d_culled, int n) { return scene_upload_device(d_tris15, d_culled, n); }
extern "C" int mirt_scene_update_device(int first, int count, const void *d_tris15) { return scene_update_device(first, count, d_tris15); }
extern "C" int mirt_scene_update(int first, int count, const float *tris15) { return scene_update_host(first, count, tris15); }
extern "C" int mirt_scene_transform(int first, int count, const float rot9[9], const float translate3[3])
{
    return scene_transform(first, count, rot9, translate3);
}
extern "C" int mirt_scene_download(int first, int count, float *tris15) { return scene_download(first, count, tris15); }
extern "C" int mirt_scene_info(struct mirt_scene_info *out) { return scene_info(out); }
extern "C" int mirt_scene_set_objects(const mirt_object *objects, int nobjects, const float *rest15, int nrest)
{
    return scene_set_objects(objects, nobjects, rest15, nrest);
}
extern "C" int mirt_scene_pose(const int32_t *which, int count, const float *xforms12) { return scene_pose(which, count, xforms12); }

extern "C" int mirt_scene_set_culled(const uint8_t *culled, int n)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (g.n <= 0) return fail(MIRT_ERR_NO_SCENE, "no scene uploaded (mirt_scene_upload)");
    if (n != g.n) return fail(MIRT_ERR_INVALID_ARGUMENT, "cull array has %d entries, scene has %d triangles", n, g.n);
    HIP_TRY(sync_all());
    g.cull_calls++;
    for (int h = 0; h < MAX_FLIGHT; h++) {
        if (culled) HIP_TRY(hipMemcpyAsync(g.d_culled + (size_t)h * n, culled, (size_t)n, hipMemcpyHostToDevice, g.stream));
        else HIP_TRY(hipMemsetAsync(g.d_culled + (size_t)h * n, 0, (size_t)n, g.stream));
        g.streams[h].culled_ver = g.cull_calls;
    }
    HIP_TRY(hipStreamSynchronize(g.stream));
    g.cull_version++;
    return MIRT_OK;
}

// The cull step on the device, for the uploaded scene: no host copy of the flags in either direction.
extern "C" int mirt_cull_device(const mirt_view *view, int flags)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (!view) return fail(MIRT_ERR_INVALID_ARGUMENT, "view must not be NULL");
    if (g.n <= 0) return fail(MIRT_ERR_NO_SCENE, "no scene uploaded (mirt_scene_upload)");
    if (view->width <= 0 || view->height <= 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "frame %d x %d", view->width, view->height);
    CullParams cp;
    cull_setup(view, flags, &cp);
    // The flags belong to the NEXT rasterised frame (the reference culls in Update(), right before Draw()): with several frames
    // in flight they go into the copy of d_culled that belongs to the stream the next call will take, on that stream, in order
    // in front of it -- the frames still running on the other streams keep their own flags, nothing waits for anything.  Should
    // the next rasterised frame land on another stream after all (a ray-traced frame came in between), raster_enqueue brings
    // the flags over (culled_ver tells).
    const int half = next_si();
    hipStream_t st = g.streams[half].stream;
    (void)hipGetLastError();                     // drop a stale error of another HIP user in this thread (see call_begin)
    if ((rc = cull_copy_wait_readers(half, st))) return rc;   // a frame of another stream may still be copying this copy's previous flags
    hipLaunchKernelGGL(k_cull, dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, st, g.d_tris, g.n, cp, g.d_culled + (size_t)half * g.n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(g.streams[half].ev_order, st));
    g.culled_latest = half;
    g.streams[half].culled_ver = ++g.cull_calls;
    g.cull_version++;
    return MIRT_OK;
}

extern "C" int mirt_scene_get_culled(uint8_t *culled, int n)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (g.n <= 0) return fail(MIRT_ERR_NO_SCENE, "no scene uploaded (mirt_scene_upload)");
    if (!culled || n != g.n) return fail(MIRT_ERR_INVALID_ARGUMENT, "cull array has %d entries, scene has %d triangles", n, g.n);
    HIP_TRY(sync_all());
    HIP_TRY(hipMemcpy(culled, g.d_culled + (size_t)g.culled_latest * g.n, (size_t)n, hipMemcpyDeviceToHost));
    return MIRT_OK;
}

extern "C" int mirt_scene_size(void) { return g.init ? g.n : 0; }

extern "C" int mirt_set_depth_of_field(int kernel_size, float focal_length)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (kernel_size > 64) return fail(MIRT_ERR_INVALID_ARGUMENT, "DOF kernel size %d exceeds 64 (the reference uses 8)", kernel_size);
    g.dof_k = kernel_size > 1 ? kernel_size : 0;
    g.dof_focal = focal_length;
    return MIRT_OK;
}

extern "C" int mirt_set_antialiasing(int samples)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (samples > 8) return fail(MIRT_ERR_INVALID_ARGUMENT, "AA samples %d exceed 8 (the reference uses 3)", samples);
    g.aa = samples > 1 ? samples : 1;
    return MIRT_OK;
}

extern "C" int mirt_set_soft_shadows(int samples, const float *positions, int npositions)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (samples <= 1) { g.soft_samples = 1; g.soft_npos = 0; return MIRT_OK; }
    if (samples > MIRT_MAX_LIGHT_POSITIONS) return fail(MIRT_ERR_INVALID_ARGUMENT, "samples %d exceeds %d", samples, MIRT_MAX_LIGHT_POSITIONS);
    if (!positions || npositions < samples || npositions > MIRT_MAX_LIGHT_POSITIONS)
        return fail(MIRT_ERR_INVALID_ARGUMENT, "need between %d and %d jittered positions (more would exceed the limit), got %d", samples, MIRT_MAX_LIGHT_POSITIONS, npositions);
    memcpy(g.soft_pos, positions, sizeof(float) * 3 * (size_t)npositions);
    g.soft_samples = samples;
    g.soft_npos = npositions;
    return MIRT_OK;
}

// ---- ray tracer -------------------------------------------------------------------------------------

extern "C" int mirt_raytrace_device_ex(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                                       int mode, int y0, int y1, int row_origin, void *d_xrgb, int pitch_bytes,
                                       void *d_rgb, void *d_index, void *d_distance, void *d_position)
{
    if (g.init && g.dof_k > 1)
        return render_with_dof(view, lights, nlights, indirect, y0, y1, row_origin, d_xrgb, pitch_bytes, d_rgb, d_index, nullptr, false,
                               [&](int ry0, int ry1, void *x, void *rgb, void *fd, void *idx, void *) {
                                   return rt_enqueue(view, lights, nlights, indirect, mode, ry0, ry1, ry0, x, view->width * 4, rgb, idx, fd,
                                                     d_distance, d_position);
                               });
    return rt_enqueue(view, lights, nlights, indirect, mode, y0, y1, row_origin, d_xrgb, pitch_bytes, d_rgb, d_index, nullptr,
                      d_distance, d_position);
}

extern "C" int mirt_raytrace_device(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                                    int mode, int y0, int y1, int row_origin, void *d_xrgb, int pitch_bytes,
                                    void *d_rgb, void *d_index)
{
    return mirt_raytrace_device_ex(view, lights, nlights, indirect, mode, y0, y1, row_origin, d_xrgb, pitch_bytes, d_rgb, d_index,
                                   nullptr, nullptr);
}

extern "C" int mirt_raytrace(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                             int mode, uint32_t *out_xrgb, int pitch_bytes, float *out_rgb, int32_t *out_index)
{
    return mirt_raytrace_ex(view, lights, nlights, indirect, mode, out_xrgb, pitch_bytes, out_rgb, out_index, nullptr, nullptr);
}

extern "C" int mirt_raytrace_ex(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                                int mode, uint32_t *out_xrgb, int pitch_bytes, float *out_rgb, int32_t *out_index,
                                float *out_distance, float *out_position)
{
    // closestIntersections[].distance shares the depth staging plane of the rasteriser entry point; .position gets its own
    const HostPlane planes[] = { { out_rgb, &g.d_rgb, 12 }, { out_index, &g.d_index, 4 }, { out_distance, &g.d_zinv, 4 }, { out_position, &g.d_pos, 12 } };
    return deliver_host(view, lights, nlights, indirect, out_xrgb, pitch_bytes, false, planes, [&](void *x, int pitch, void *const *d) {
        return mirt_raytrace_device_ex(view, lights, nlights, indirect, mode, 0, view->height, 0, x, pitch, d[0], d[1], d[2], d[3]);
    });
}

extern "C" int mirt_raytrace_async(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                                   int mode, uint32_t *out_xrgb, int pitch_bytes)
{
    return deliver_async(view, lights, nlights, indirect, out_xrgb, pitch_bytes, false, [&](void *x, int pitch) {
        return mirt_raytrace_device_ex(view, lights, nlights, indirect, mode, 0, view->height, 0, x, pitch, nullptr, nullptr, nullptr, nullptr);
    });
}

// (the ray queries' entry points -- mirt_intersect*, mirt_direct_light*, mirt_occluded* and the rest: the tail of ../capi/query.cpp)

// ---- rasteriser -------------------------------------------------------------------------------------

extern "C" int mirt_rasterise_device(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                                     int y0, int y1, int row_origin, void *d_xrgb, int pitch_bytes, void *d_rgb,
                                     void *d_zinv, void *d_index)
{
    if (g.init && g.dof_k > 1)
        return render_with_dof(view, lights, nlights, indirect, y0, y1, row_origin, d_xrgb, pitch_bytes, d_rgb, d_index, d_zinv, true,
                               [&](int ry0, int ry1, void *x, void *rgb, void *fd, void *idx, void *zinv) {
                                   return raster_enqueue(view, lights, nlights, indirect, ry0, ry1, ry0, x, view->width * 4, rgb, zinv, idx, fd);
                               });
    return raster_enqueue(view, lights, nlights, indirect, y0, y1, row_origin, d_xrgb, pitch_bytes, d_rgb, d_zinv, d_index);
}

// (the rasteriser's Update() paints the whole surface, rasteriser.cpp:190: every word is written)
extern "C" int mirt_rasterise(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                              uint32_t *out_xrgb, int pitch_bytes, float *out_rgb, float *out_zinv, int32_t *out_index)
{
    const HostPlane planes[] = { { out_rgb, &g.d_rgb, 12 }, { out_zinv, &g.d_zinv, 4 }, { out_index, &g.d_index, 4 } };
    return deliver_host(view, lights, nlights, indirect, out_xrgb, pitch_bytes, true, planes, [&](void *x, int pitch, void *const *d) {
        return mirt_rasterise_device(view, lights, nlights, indirect, 0, view->height, 0, x, pitch, d[0], d[1], d[2]);
    });
}

extern "C" int mirt_rasterise_async(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                                    uint32_t *out_xrgb, int pitch_bytes)
{
    return deliver_async(view, lights, nlights, indirect, out_xrgb, pitch_bytes, true, [&](void *x, int pitch) {
        return mirt_rasterise_device(view, lights, nlights, indirect, 0, view->height, 0, x, pitch, nullptr, nullptr, nullptr);
    });
}

// ---- statistics -------------------------------------------------------------------------------------

extern "C" int mirt_get_stats(mirt_stats *out)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (!out) return fail(MIRT_ERR_INVALID_ARGUMENT, "out must not be NULL");
    if (g.stats_pending) {
        const StreamState &ls = g.streams[g.ev_cur];                 // the last call's events
        HIP_TRY(hipStreamSynchronize(g.stats_stream));               // the stream the last call ran on
        float ms = 0.0f;
        g.stats.gpu_ms = 0.0f;
        if (ls.call_timed && hipEventElapsedTime(&ms, ls.ev[EV_CALL0], ls.ev[EV_CALL1]) == hipSuccess) g.stats.gpu_ms = ms;
        for (int k = 0; k < 8; k++) {
            g.stats.kernel_ms[k] = 0.0f;
            if (g.profiling && ls.ev_used[k] && hipEventElapsedTime(&ms, ls.ev[EV_K0 + 2 * k], ls.ev[EV_K0 + 2 * k + 1]) == hipSuccess)
                g.stats.kernel_ms[k] = ms;
        }
        if (g.pending_is_rt && g.pending_empty) {
            g.stats.primary_rays = g.stats.shadow_rays = g.stats.tests = 0;
        } else if (g.pending_is_rt) {
            static unsigned long long shard[HIT_SHARDS * HIT_SHARD_STRIDE];
            HIP_TRY(hipMemcpy(shard, g.d_hits, sizeof shard, hipMemcpyDeviceToHost));
            unsigned long long hits = 0, tests = 0, cands = 0, sp = 0, ss = 0, dr = 0;
            for (int i = 0; i < HIT_SHARDS; i++) {
                const unsigned long long *w = shard + i * HIT_SHARD_STRIDE;
                hits += w[0]; tests += w[1]; cands += w[2]; sp += w[3]; ss += w[4]; dr += w[5];
            }
            g.stats.tests = tests;
            g.stats.candidates = cands;
            g.stats.steps_primary = sp; g.stats.steps_shadow = ss; g.stats.drains = dr;
#ifdef MIRT_TR_TIMING
            {   // (experiments, rt_trace.hip built with -DMIRT_TR_TIMING: the shard words carry the waves' time per segment)
                unsigned long long seg[11] = { 0 };
                for (int i = 0; i < HIT_SHARDS; i++) {
                    for (int k = 0; k < 10; k++) seg[k] += shard[i * HIT_SHARD_STRIDE + 3 + k];
                    seg[10] = std::max(seg[10], shard[i * HIT_SHARD_STRIDE + 13]);
                }
                fprintf(stderr, "[mirt timing] Mticks: record %.1f | stage %.1f steps %.1f drains %.1f merge %.1f | light term %.1f offsets+first row %.1f walk %.1f drain %.1f | rest %.1f | longest wave %llu ticks\n",
                        seg[0] * 1e-6, seg[1] * 1e-6, seg[2] * 1e-6, seg[3] * 1e-6, seg[4] * 1e-6, seg[5] * 1e-6, seg[6] * 1e-6, seg[7] * 1e-6, seg[8] * 1e-6, seg[9] * 1e-6, seg[10]);
            }
#endif
            g.stats.primary_rays = g.pending_primary;
            g.stats.shadow_rays = (uint64_t)hits * (uint64_t)g.pending_nlights;
            if (g.stats.mode_used == MIRT_RT_BINNED && g.stats_sel_count) {
                uint32_t nsel = 0;
                HIP_TRY(hipMemcpy(&nsel, g.stats_sel_count, 4, hipMemcpyDeviceToHost));
                g.stats.selected_triangles = nsel;
            }
            if (g.stats.mode_used == MIRT_RT_BRUTE && !g.pending_counted)      // every ray tests every triangle
                g.stats.tests = (g.stats.primary_rays + g.stats.shadow_rays) * (uint64_t)g.n;
            if (g.stats.candidates == 0) g.stats.candidates = g.stats.tests;        // kernels that test every candidate they are offered
        }
        g.stats_pending = false;
        (void)hipGetLastError();                 // an event pair a frame never recorded (no clear needed, ...) leaves hipErrorInvalidHandle
                                                 // behind: do not hand it to the next HIP user of this thread
    }
    *out = g.stats;
    return MIRT_OK;
}

// Per-kernel GPU times of the call BEFORE the last one.
extern "C" int mirt_get_previous_kernel_ms(float *kernel_ms8, float *gpu_ms)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (!kernel_ms8) return fail(MIRT_ERR_INVALID_ARGUMENT, "kernel_ms8 must not be NULL");
    if (g.in_flight < 2) return fail(MIRT_ERR_INVALID_ARGUMENT, "the call before the last one keeps its events only with two or more frames in flight (mirt_set_frames_in_flight)");
    HIP_TRY(sync_all());
    const StreamState &ps = g.streams[(g.ev_cur + g.in_flight - 1) % g.in_flight];
    float ms = 0.0f;
    if (gpu_ms) *gpu_ms = (ps.call_timed && hipEventElapsedTime(&ms, ps.ev[EV_CALL0], ps.ev[EV_CALL1]) == hipSuccess) ? ms : 0.0f;
    for (int k = 0; k < 8; k++) {
        kernel_ms8[k] = 0.0f;
        if (g.profiling && ps.ev_used[k] && hipEventElapsedTime(&ms, ps.ev[EV_K0 + 2 * k], ps.ev[EV_K0 + 2 * k + 1]) == hipSuccess)
            kernel_ms8[k] = ms;
    }
    (void)hipGetLastError();
    return MIRT_OK;
}

// ---- several GPUs of one node: frames shard by row bands, one process per GPU ----------------------

extern "C" int mirt_band_of(int rank, int world, int height, int *y0, int *y1)
{
    if (world < 1 || rank < 0 || rank >= world || height < 0 || !y0 || !y1) return fail(MIRT_ERR_INVALID_ARGUMENT, "band of rank %d / %d, %d rows", rank, world, height);
    band_of(rank, world, height, y0, y1);
    return MIRT_OK;
}

extern "C" int mirt_band_plan(int world, int root, int width, int height, int nviews, uint64_t *root_offset, uint64_t *band_offset,
                              uint64_t *bytes, int32_t *peer, int max_pieces)
{
    if (world < 1 || root < 0 || root >= world || width < 1 || height < 0 || nviews < 1 || max_pieces < 0)
        return fail(MIRT_ERR_INVALID_ARGUMENT, "band plan: world %d root %d frame %dx%d views %d", world, root, width, height, nviews);
    return plan_out(world, root, width, height, nviews, 0, nullptr, root_offset, band_offset, bytes, peer, max_pieces);
}

extern "C" int mirt_set_partition(int strip_rows)
{
    if (strip_rows != MIRT_PARTITION_WEIGHTED && (strip_rows < 0 || (strip_rows % BIN_TILE) != 0))
        return fail(MIRT_ERR_INVALID_ARGUMENT, "strip height %d must be 0 (bands), a multiple of %d rows, or MIRT_PARTITION_WEIGHTED", strip_rows, BIN_TILE);
    if (g.init) HIP_TRY(sync_all());
    g.strip_rows = strip_rows;
    return MIRT_OK;
}

extern "C" int mirt_set_cost_histogram(int on)
{
    int rc;
    if ((rc = need_init())) return rc;
    g.want_hist = on != 0;
    return MIRT_OK;
}

extern "C" int mirt_weighted_bounds(const uint32_t *hist, int hist_rows, int hist_shift, int width, int height, int world, int32_t *bounds)
{
    if (world < 1 || width < 1 || height < 0 || !bounds || hist_rows < 0 || hist_shift < 0 || hist_shift > 16 || (hist_rows > 0 && !hist))
        return fail(MIRT_ERR_INVALID_ARGUMENT, "weighted bounds: world %d frame %dx%d, %d histogram rows, shift %d", world, width, height, hist_rows, hist_shift);
    std::vector<int> b((size_t)world + 1);
    part_weighted_bounds(hist, hist_rows, hist_shift, width, height, world, part_tile_weight(), b.data());
    for (int r = 0; r <= world; r++) bounds[r] = b[(size_t)r];
    return MIRT_OK;
}

extern "C" int mirt_cost_histogram(uint32_t *hist, int max_rows, int *rows, int *shift)
{
    int rc;
    if ((rc = need_init())) return rc;
    int nr = 0, sh = 0;
    const uint32_t *h = hist_lookup(0, &nr, &sh);
    if (!h) { if (rows) *rows = 0; if (shift) *shift = 0; return 0; }
    if (rows) *rows = nr;
    if (shift) *shift = sh;
    for (int i = 0; i < nr && i < max_rows && hist; i++) hist[i] = h[i];
    return nr;
}

extern "C" int mirt_partition_bounds(int world, int width, int height, int32_t *bounds)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (world < 1 || width < 1 || height < 0 || !bounds) return fail(MIRT_ERR_INVALID_ARGUMENT, "partition bounds: world %d frame %dx%d", world, width, height);
    std::vector<int> b;
    current_bounds(world, width, height, b);
    for (int r = 0; r <= world; r++) bounds[r] = b[(size_t)r];
    return MIRT_OK;
}

extern "C" int mirt_bounds_plan(int world, int root, int width, int height, int nviews, const int32_t *bounds, uint64_t *root_offset, uint64_t *band_offset,
                                uint64_t *bytes, int32_t *peer, int max_pieces)
{
    if (world < 1 || root < 0 || root >= world || width < 1 || height < 0 || nviews < 1 || max_pieces < 0 || !bounds)
        return fail(MIRT_ERR_INVALID_ARGUMENT, "bounds plan: world %d root %d frame %dx%d views %d", world, root, width, height, nviews);
    if (bounds[0] != 0 || bounds[world] != height) return fail(MIRT_ERR_INVALID_ARGUMENT, "bounds plan: boundaries must start at 0 and end at %d", height);
    for (int r = 0; r < world; r++)
        if (bounds[r + 1] < bounds[r]) return fail(MIRT_ERR_INVALID_ARGUMENT, "bounds plan: boundaries must rise from 0 to %d", height);
    return plan_out(world, root, width, height, nviews, 0, bounds, root_offset, band_offset, bytes, peer, max_pieces);
}

extern "C" int mirt_partition_segments(int rank, int world, int height, int strip_rows, int32_t *y0, int32_t *y1, int max_segments)
{
    if (world < 1 || rank < 0 || rank >= world || height < 0 || strip_rows < 0 || max_segments < 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "segments of rank %d / %d, %d rows, strips of %d", rank, world, height, strip_rows);
    const int n = part_segments(rank, world, height, strip_rows);
    for (int k = 0; k < n && k < max_segments; k++) {
        int a, b;
        part_segment(rank, world, height, strip_rows, k, &a, &b);
        if (y0) y0[k] = a;
        if (y1) y1[k] = b;
    }
    return n;
}

extern "C" int mirt_partition_plan(int world, int root, int width, int height, int nviews, int strip_rows, uint64_t *root_offset, uint64_t *band_offset,
                                   uint64_t *bytes, int32_t *peer, int max_pieces)
{
    if (world < 1 || root < 0 || root >= world || width < 1 || height < 0 || nviews < 1 || max_pieces < 0 || strip_rows < 0)
        return fail(MIRT_ERR_INVALID_ARGUMENT, "partition plan: world %d root %d frame %dx%d views %d strips %d", world, root, width, height, nviews, strip_rows);
    return plan_out(world, root, width, height, nviews, strip_rows, nullptr, root_offset, band_offset, bytes, peer, max_pieces);
}

extern "C" int mirt_comm_create_id(void *id128)
{
    if (!id128) return fail(MIRT_ERR_INVALID_ARGUMENT, "id must not be NULL");
    if (!comm_create_id(id128)) return fail(MIRT_ERR_HIP, "%s", comm_error(nullptr));
    return MIRT_OK;
}

extern "C" int mirt_comm_init(const void *id128, int rank, int world)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (!id128) return fail(MIRT_ERR_INVALID_ARGUMENT, "id must not be NULL");
    if (g.comm) { HIP_TRY(sync_all()); comm_destroy(g.comm); g.comm = nullptr; }
    g.comm = comm_init(id128, rank, world);
    if (!g.comm) return fail(MIRT_ERR_HIP, "%s", comm_error(nullptr));
    if (!g.comm_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&g.comm_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&g.ev_rendered, hipEventDisableTiming));
        for (int i = 0; i < 2; i++) HIP_TRY(hipEventCreateWithFlags(&g.ev_sent[i], hipEventDisableTiming));
    }
    return MIRT_OK;
}

extern "C" int mirt_comm_selfcheck(size_t bytes)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (!g.comm) return fail(MIRT_ERR_INVALID_ARGUMENT, "mirt_comm_selfcheck before mirt_comm_init");
    HIP_TRY(sync_all());
    if (!comm_selfcheck(g.comm, bytes, g.comm_stream)) return fail(MIRT_ERR_HIP, "%s", comm_error(g.comm));
    return MIRT_OK;
}

extern "C" int mirt_comm_shutdown(void)
{
    if (!g.init || !g.comm) return MIRT_OK;
    HIP_TRY(sync_all());
    comm_destroy(g.comm);
    g.comm = nullptr;
    return MIRT_OK;
}

extern "C" int mirt_raytrace_sharded(const mirt_view *views, int nviews, const mirt_light *lights, int nlights, const float *indirect,
                                     int mode, int root, void *d_frames, int pitch_bytes)
{
    return render_sharded(views, nviews, root, d_frames, pitch_bytes, false, lights, nlights, indirect, mode);
}

extern "C" int mirt_rasterise_sharded(const mirt_view *views, int nviews, const mirt_light *lights, int nlights, const float *indirect,
                                      int root, void *d_frames, int pitch_bytes)
{
    return render_sharded(views, nviews, root, d_frames, pitch_bytes, true, lights, nlights, indirect, 0);
}
