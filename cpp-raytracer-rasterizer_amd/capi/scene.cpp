// scene.cpp -- scenes that live on the device: triangles uploaded from device memory (mirt_scene_upload_device), replaced in part
// (mirt_scene_update*), moved in place (mirt_scene_transform), posed object by object from a rest pose the library keeps
// (mirt_scene_set_objects, mirt_scene_pose), read back (mirt_scene_download) and described (mirt_scene_info); the kernels:
// ../scene/scene_kernels.hip.  Every call that changes the scene starts as mirt_scene_upload does -- it waits for every
// library stream and for the device, so frames in flight finish on the old scene and the caller's source is complete whatever
// stream wrote it -- and returns with the scene, its tables, its bounding box and its finiteness flag current: one 32-byte
// read-back behind the kernels.  scene_commit is what all of them, mirt_scene_upload included, do to the host's state last.
#include "capi.hpp"
#include "../scene/scene_kernels.hpp"

namespace mirt {

static_assert(SCENE_CULL_COPIES == MAX_FLIGHT, "one copy of the cull flags per stream");

void scene_commit(bool flags_changed)
{
    for (StreamState &ss : g.streams) {
        ss.cam.forget_scene();                                      // tables, kept passes and pair counts belong to the old scene
        ss.lt.forget_scene();
        ss.hist.forget_scene();                                     // ... and so do the cost histograms
    }
    g.lc.valid = false;
    if (flags_changed) {
        g.cull_calls++;
        for (StreamState &ss : g.streams) ss.culled_ver = g.cull_calls;
    }
    g.scene_version++;
}

static int need_scene()
{
    if (g.n <= 0) return fail(MIRT_ERR_NO_SCENE, "no scene uploaded (mirt_scene_upload)");
    return MIRT_OK;
}

// The checks of a call on rows [first, first + count) of the scene, before anything touches the device: the not-initialised status
// first, then what can be said without a scene, then the scene, then the range.  ptr: the rows' source or destination (nullable when
// count is 0; has_array = false: the call has none).
static int check_range(int first, int count, const void *ptr, const char *what, bool has_array = true)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (first < 0 || count < 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "%s: range [%d, %d + %d) is negative", what, first, first, count);
    if (has_array && count > 0 && !ptr) return fail(MIRT_ERR_INVALID_ARGUMENT, "%s: the triangle array must not be NULL when count is > 0", what);
    if ((uintptr_t)ptr & 3) return fail(MIRT_ERR_INVALID_ARGUMENT, "%s: the triangle array %p is not 4-byte aligned", what, ptr);
    if ((rc = need_scene())) return rc;
    if ((long long)first + count > g.n) return fail(MIRT_ERR_INVALID_ARGUMENT, "%s: range [%d, %d + %d) leaves the scene's %d triangles", what, first, first, count, g.n);
    return MIRT_OK;
}

static int begin_change()
{
    HIP_TRY(sync_all());
    HIP_TRY(hipDeviceSynchronize());             // the caller's streams too: its source buffer is complete
    (void)hipGetLastError();
    return MIRT_OK;
}

template <int MODE> static void launch_range(const SceneRange &a)
{
    hipLaunchKernelGGL(k_scene_range<MODE>, dim3((unsigned)((a.count + SCENE_BLOCK_ROWS - 1) / SCENE_BLOCK_ROWS)), dim3(SCENE_BLOCK_ROWS), 0, g.stream, a);
}

// What every pass over the scene starts from: the scene's arrays, and the bounds block at its initial values (one launch).
static int range_begin(int n, SceneRange *a)
{
    if (!g.d_scene_bounds) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&g.d_scene_bounds), sizeof(SceneBounds)));
    *a = SceneRange{};
    a->tris = g.d_tris; a->geo = g.d_geo; a->shade = g.d_shade;
    a->n = n;
    a->bounds = reinterpret_cast<SceneBounds *>(g.d_scene_bounds);
    hipLaunchKernelGGL(k_scene_bounds_init, dim3(1), dim3(8), 0, g.stream, a->bounds);
    return MIRT_OK;
}

// ... and ends with: the bounds of the whole scene behind the launches that changed rows (have_bounds: the launch over the whole
// scene took them itself) and the host's copy of them.
static int range_end(SceneRange a, bool have_bounds)
{
    if (!have_bounds) {
        a.first = 0; a.count = a.n;
        launch_range<SCENE_BOUNDS>(a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g.stream));
    SceneBounds hb;
    HIP_TRY(hipMemcpy(&hb, a.bounds, sizeof hb, hipMemcpyDeviceToHost));
    g.scene_finite = hb.not_finite == 0;
    for (int c = 0; c < 3; c++) { g.bbox_lo[c] = scene_unord(hb.lo[c]); g.bbox_hi[c] = scene_unord(hb.hi[c]); }
    return MIRT_OK;
}

// Rows [first, first + count) of g.d_tris from d_src (NULL: the scene's own rows moved by rot / tr), their table entries, the
// bounds of the whole scene and the host's copy of them: three launches, two when the range is the whole scene.
static int change_rows(int first, int count, int n, const float *d_src, const float *rot9, const float *tr3, bool set_culled, const uint8_t *d_culled_src)
{
    int rc;
    SceneRange a;
    if ((rc = range_begin(n, &a))) return rc;
    a.src = d_src;
    a.first = first; a.count = count;
    a.culled = set_culled ? g.d_culled : nullptr; a.culled_src = d_culled_src;
    if (rot9) { memcpy(a.rot, rot9, sizeof a.rot); memcpy(a.tr, tr3, sizeof a.tr); }
    const bool whole = first == 0 && count == n;
    if (whole) {
        if (rot9) launch_range<SCENE_INGEST | SCENE_XFORM | SCENE_BOUNDS>(a); else launch_range<SCENE_INGEST | SCENE_BOUNDS>(a);
    } else {
        if (rot9) launch_range<SCENE_INGEST | SCENE_XFORM>(a); else launch_range<SCENE_INGEST>(a);
    }
    return range_end(a, whole);
}

int scene_upload_device(const void *d_tris15, const void *d_culled, int n)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (!d_tris15 || n < 1) return fail(MIRT_ERR_INVALID_ARGUMENT, "scene needs at least one triangle (n = %d)", n);
    if ((uintptr_t)d_tris15 & 3) return fail(MIRT_ERR_INVALID_ARGUMENT, "mirt_scene_upload_device: the triangle array %p is not 4-byte aligned", d_tris15);
    if ((rc = begin_change())) return rc;
    g.n = 0;
    scene_forget_objects();                      // (their ranges were checked against the old scene)
    if ((rc = dev_realloc(&g.d_tris, (size_t)n * 15))) return rc;
    if ((rc = dev_realloc(&g.d_culled, (size_t)MAX_FLIGHT * n))) return rc;
    if ((rc = dev_realloc(&g.d_geo, (size_t)n))) return rc;
    if ((rc = dev_realloc(&g.d_shade, (size_t)n))) return rc;
    if ((rc = change_rows(0, n, n, static_cast<const float *>(d_tris15), nullptr, nullptr, true, static_cast<const uint8_t *>(d_culled)))) return rc;
    g.n = n;
    scene_commit(true);
    return MIRT_OK;
}

int scene_update_device(int first, int count, const void *d_tris15)
{
    int rc;
    if ((rc = check_range(first, count, d_tris15, "mirt_scene_update_device"))) return rc;
    if (count == 0) return MIRT_OK;
    if ((rc = begin_change())) return rc;
    if ((rc = change_rows(first, count, g.n, static_cast<const float *>(d_tris15), nullptr, nullptr, false, nullptr))) return rc;
    scene_commit(false);
    return MIRT_OK;
}

int scene_update_host(int first, int count, const float *tris15)
{
    int rc;
    if ((rc = check_range(first, count, tris15, "mirt_scene_update"))) return rc;
    if (count == 0) return MIRT_OK;
    if ((rc = begin_change())) return rc;
    const size_t words = (size_t)count * 15;
    if (g.scene_stage_cap < words && (rc = dev_grow(&g.d_scene_stage, &g.scene_stage_cap, words, words, false))) return rc;
    HIP_TRY(hipMemcpy(g.d_scene_stage, tris15, words * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());             // (a null-stream copy, as in mirt_scene_upload: landed before a kernel of our streams reads it)
    if ((rc = change_rows(first, count, g.n, g.d_scene_stage, nullptr, nullptr, false, nullptr))) return rc;
    scene_commit(false);
    return MIRT_OK;
}

int scene_transform(int first, int count, const float *rot9, const float *translate3)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (!rot9 || !translate3) return fail(MIRT_ERR_INVALID_ARGUMENT, "mirt_scene_transform: rot9 / translate3 must not be NULL");
    if ((rc = check_range(first, count, nullptr, "mirt_scene_transform", false))) return rc;
    if (count == 0) return MIRT_OK;
    if ((rc = begin_change())) return rc;
    if ((rc = change_rows(first, count, g.n, nullptr, rot9, translate3, false, nullptr))) return rc;
    scene_commit(false);
    return MIRT_OK;
}

// ---- posed scenes ----

void scene_forget_objects()
{
    g.objects.clear();
    g.nrest = 0;
    if (g.d_rest) (void)hipFree(g.d_rest);
    if (g.d_pose_table) (void)hipFree(g.d_pose_table);
    if (g.h_pose_table) (void)hipHostFree(g.h_pose_table);
    g.d_rest = nullptr; g.rest_cap = 0;
    g.d_pose_table = g.h_pose_table = nullptr; g.pose_table_cap = 0;
}

int scene_set_objects(const mirt_object *objects, int nobjects, const float *rest15, int nrest)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (nobjects < 0 || nrest < 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "mirt_scene_set_objects: %d objects, %d rest triangles", nobjects, nrest);
    if (nobjects > 0 && !objects) return fail(MIRT_ERR_INVALID_ARGUMENT, "mirt_scene_set_objects: the object array must not be NULL when nobjects is > 0");
    if (nrest > 0 && !rest15) return fail(MIRT_ERR_INVALID_ARGUMENT, "mirt_scene_set_objects: the rest array must not be NULL when nrest is > 0");
    if ((uintptr_t)rest15 & 3) return fail(MIRT_ERR_INVALID_ARGUMENT, "mirt_scene_set_objects: the rest array %p is not 4-byte aligned", (const void *)rest15);
    if ((rc = need_scene())) return rc;
    const bool snapshot = !rest15;
    if (snapshot) nrest = g.n;
    const ObjectCheck oc = check_objects(objects, nobjects, nrest, g.n);
    if (oc.fault != OBJECTS_OK) {
        const mirt_object &o = objects[oc.a];
        if (oc.fault == OBJECTS_OVERLAP)
            return fail(MIRT_ERR_INVALID_ARGUMENT, "mirt_scene_set_objects: the scene ranges of objects %d and %d, [%d, %d + %d) and [%d, %d + %d), overlap", oc.a, oc.b,
                        o.scene_first, o.scene_first, o.count, objects[oc.b].scene_first, objects[oc.b].scene_first, objects[oc.b].count);
        return fail(MIRT_ERR_INVALID_ARGUMENT, "mirt_scene_set_objects: object %d {rest %d, scene %d, count %d} %s (%d rest triangles, %d in the scene)", oc.a,
                    o.rest_first, o.scene_first, o.count,
                    oc.fault == OBJECT_NEGATIVE ? "has a negative field" : oc.fault == OBJECT_LEAVES_REST ? "leaves the rest pose" : "leaves the scene", nrest, g.n);
    }
    if (nobjects == 0) { scene_forget_objects(); return MIRT_OK; }
    // The scene is not touched: frames in flight only read it, and it only changes inside calls that return with it complete, so
    // the snapshot is a plain copy; a pose waits for the device before its kernel reads the rest pose, wherever the copy ran.
    const size_t words = (size_t)nrest * 15;
    g.objects.clear();                           // (a copy that fails leaves no objects, not the old ones over a rest pose half replaced)
    g.nrest = 0;
    if (g.rest_cap < words && (rc = dev_grow(&g.d_rest, &g.rest_cap, words, words, false))) return rc;
    if (words) HIP_TRY(hipMemcpy(g.d_rest, snapshot ? g.d_tris : rest15, words * sizeof(float), snapshot ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    g.objects.assign(objects, objects + nobjects);
    g.nrest = nrest;
    return MIRT_OK;
}

int scene_pose(const int32_t *which, int count, const float *xforms12)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (count < 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "mirt_scene_pose: count %d is negative", count);
    if (count > 0 && !xforms12) return fail(MIRT_ERR_INVALID_ARGUMENT, "mirt_scene_pose: the transforms must not be NULL when count is > 0");
    if ((rc = need_scene())) return rc;
    const int nobjects = (int)g.objects.size();
    const WhichCheck wc = check_which(which, count, nobjects);
    switch (wc.fault) {
    case WHICH_OK: break;
    case WHICH_NO_OBJECTS: return fail(MIRT_ERR_INVALID_ARGUMENT, "mirt_scene_pose: no objects declared (mirt_scene_set_objects)");
    case WHICH_TOO_MANY: return fail(MIRT_ERR_INVALID_ARGUMENT, "mirt_scene_pose: count %d exceeds the %d objects declared", count, nobjects);
    case WHICH_OUTSIDE: return fail(MIRT_ERR_INVALID_ARGUMENT, "mirt_scene_pose: which[%d] = %d is outside the %d objects declared", wc.at, which[wc.at], nobjects);
    case WHICH_TWICE: return fail(MIRT_ERR_INVALID_ARGUMENT, "mirt_scene_pose: which[%d] = %d is listed twice", wc.at, which[wc.at]);
    }
    if (count == 0) return MIRT_OK;
    // the table of the call, filled where the host can write it: a pose returns with its stream idle, so neither copy is in use
    const size_t words = pose_table_words(count);
    if (g.pose_table_cap < words) {
        if (g.h_pose_table) (void)hipHostFree(g.h_pose_table);
        g.h_pose_table = nullptr;
        if ((rc = dev_grow(&g.d_pose_table, &g.pose_table_cap, words, words, false))) return rc;
        if (hipHostMalloc(reinterpret_cast<void **>(&g.h_pose_table), words * 4, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            g.h_pose_table = nullptr; g.pose_table_cap = 0;
            return fail(MIRT_ERR_OUT_OF_MEMORY, "mirt_scene_pose: no pinned memory for a table of %d objects", count);
        }
    }
    const uint32_t items = fill_pose_table(g.objects.data(), which, count, xforms12, g.h_pose_table);
    if (items == 0) return MIRT_OK;              // every listed object is empty: nothing changes
    if ((rc = begin_change())) return rc;
    SceneRange a;
    if ((rc = range_begin(g.n, &a))) return rc;
    HIP_TRY(hipMemcpyAsync(g.d_pose_table, g.h_pose_table, words * 4, hipMemcpyHostToDevice, g.stream));
    a.src = g.d_rest;
    a.pose = reinterpret_cast<const PoseEntry *>(g.d_pose_table); a.pose_count = count;
    hipLaunchKernelGGL(k_scene_range<SCENE_INGEST | SCENE_XFORM | SCENE_POSE>, dim3(items), dim3(SCENE_BLOCK_ROWS), 0, g.stream, a);
    if ((rc = range_end(a, false))) return rc;
    scene_commit(false);
    return MIRT_OK;
}

int scene_download(int first, int count, float *tris15)
{
    int rc;
    if ((rc = check_range(first, count, tris15, "mirt_scene_download"))) return rc;
    if (count == 0) return MIRT_OK;
    // (the scene only changes inside calls that return with it complete: nothing to wait for)
    HIP_TRY(hipMemcpy(tris15, g.d_tris + (size_t)15 * first, (size_t)count * 15 * sizeof(float), hipMemcpyDeviceToHost));
    return MIRT_OK;
}

int scene_info(struct mirt_scene_info *out)
{
    int rc;
    if ((rc = need_init())) return rc;
    if (!out) return fail(MIRT_ERR_INVALID_ARGUMENT, "out must not be NULL");
    if ((rc = need_scene())) return rc;
    out->n = g.n;
    out->finite = g.scene_finite ? 1 : 0;
    for (int c = 0; c < 3; c++) { out->bbox_lo[c] = g.bbox_lo[c]; out->bbox_hi[c] = g.bbox_hi[c]; }
    out->version = g.scene_version;
    return MIRT_OK;
}

}  // namespace mirt
