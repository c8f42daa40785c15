/*
 * mirt.h -- C-ABI of the MI355X-native per-pixel render path ("mirt").
 *
 * This is the drop-in boundary for the two hot loops of ArchDD/CPP-Raytracer-Rasterizer.  The reference
 * has no plugin / FFI layer: its hot path is the free function `void Draw()` reading globals and writing
 * through `PutPixelSDL` (raytracer/Source/raytracer.cpp:104,547; rasteriser/Source/rasteriser.cpp:86,461;
 * raytracer/Source/SDLauxiliary.h:29,70-81).  Each entry point below names the reference interface it
 * replaces.  The host-side `Draw()` adapter that marshals the reference-shaped globals into these calls is
 * cpp-raytracer-rasterizer_amd/host/mirt_draw.hpp; INTEGRATION.md shows the lines a maintainer adds.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary; every function returns 0 on success or a negative
 *     mirt_status, with a human-readable message available from mirt_last_error();
 *   - the library never exits the process and never falls back to a CPU path: without a usable GPU
 *     every compute entry point fails with MIRT_ERR_NO_DEVICE;
 *   - the caller owns every host pointer for the duration of a call; the library owns all device memory;
 *   - entry points are meant for one host thread (the SDL loop), are not re-entrant, and are synchronous
 *     (the frame is complete on return) unless the name ends in `_device`/`_async`;
 *   - a triangle is 15 floats {v0, v1, v2, normal, color} -- the field order of `class Triangle`
 *     (raytracer/Source/TestModel.h:11-32; sizeof == 60); a light is 7 floats {position, color,
 *     intensity} == `class Light` (TestModel.h:35-45; sizeof == 28); matrices are GLM column-major mat3;
 *   - per-pixel planes are row-major with row stride == width (the reference indexes them with
 *     SCREEN_HEIGHT, which is only correct for its square 500x500 frame -- SURVEY Appendix E-1).
 */
#ifndef MIRT_H
#define MIRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIRT_API __attribute__((visibility("default")))
#define MIRT_ABI_VERSION 4
#define MIRT_MAX_LIGHTS 32            /* Light lights[32], raytracer.cpp:48 / rasteriser.cpp:50 */
/* Most light POSITIONS of a ray-traced frame or a DirectLight query: lights x soft-shadow samples (vec3 randomPositions[256],
 * raytracer.cpp:84).  MIRT_MAX_LIGHTS stays the most lights, and the most positions one pass and one light cube take. */
#define MIRT_MAX_LIGHT_POSITIONS 256

typedef enum mirt_status {
    MIRT_OK = 0,
    MIRT_ERR_NO_DEVICE = -1,          /* no HIP device / wrong architecture                     */
    MIRT_ERR_NOT_INITIALISED = -2,    /* mirt_init not called                                    */
    MIRT_ERR_INVALID_ARGUMENT = -3,
    MIRT_ERR_NO_SCENE = -4,           /* render call before mirt_scene_upload                    */
    MIRT_ERR_OUT_OF_MEMORY = -5,
    MIRT_ERR_HIP = -6                 /* a HIP runtime call failed; see mirt_last_error()        */
} mirt_status;

/* cameraPos / cameraRot / focalLength / SCREEN_WIDTH / SCREEN_HEIGHT (raytracer.cpp:64-73,
 * rasteriser.cpp:35-41). rot is GLM column-major: rot[c*3+r] == cameraRot[c][r]. */
typedef struct mirt_view {
    float pos[3];
    float rot[9];
    float focal;
    int32_t width;
    int32_t height;
} mirt_view;

/* class Light (TestModel.h:35-45), same field order and size (28 bytes). */
typedef struct mirt_light {
    float pos[3];
    float color[3];
    float intensity;
} mirt_light;

/* How the ray tracer finds each ray's candidate triangles.  All modes return identical results. */
typedef enum mirt_rt_mode {
    MIRT_RT_AUTO = 0,     /* brute force for small scenes, binned otherwise                          */
    MIRT_RT_BRUTE = 1,    /* every ray tests every triangle (what ClosestIntersection does)         */
    MIRT_RT_BINNED = 2    /* conservative screen-tile / light-cube binning, same accept arithmetic  */
} mirt_rt_mode;

/* Counters of the last render call (ray accounting follows SURVEY section 8(d)). */
typedef struct mirt_stats {
    uint64_t primary_rays;        /* width * rows rendered                                          */
    uint64_t shadow_rays;         /* nlights * (pixels whose primary ray hit): DirectLight's calls, in every mode -- the binned
                                     kernel settles a ray whose light term is exactly zero (a face turned away from the light)
                                     without walking it, as it always has a ray ended by a certain occluder; both count     */
    uint64_t tests;               /* ray-triangle tests actually executed (0 if not counted: the binned kernel keeps this and
                                     the four counts below for frames rendered with mirt_set_profiling(1) only; a shadow ray
                                     that is not walked adds nothing to them)                                               */
    float gpu_ms;                 /* hipEvent time of the call's device work; 0 unless profiling is on   */
    float kernel_ms[8];           /* per-kernel time of the call when profiling is on (see below)    */
    int32_t mode_used;            /* mirt_rt_mode actually used                                      */
    uint64_t candidates;          /* ray-candidate pairs offered to the rays after the early end (a tile's list ends at the depth
                                     shell of the tile's farthest hit; >= tests: the binned kernel skips candidates that cannot
                                     matter before it tests them); == tests elsewhere */
    /* the binned ray tracer's own loop counts (0 elsewhere): wave-level steps of the two filter loops -- one step = one
     * candidate row tested by the lanes of a wave -- and exact-stage drains; what the kernel's instruction count scales with */
    uint64_t steps_primary;
    uint64_t steps_shadow;
    uint64_t drains;
    /* binned ray tracer (ABI 4): 1 when the frame kept the CAMERA's binning pass of its stream -- nothing that pass depends on had
     * changed since (the view stood still: a light key, a toggle; raytracer.cpp:385-537) --, and how many of the scene's triangles
     * the rows of the call can see at all (what the camera's pass walked; 0 when it was kept) */
    uint32_t bins_reused;
    uint32_t selected_triangles;
} mirt_stats;

/* indices into mirt_stats.kernel_ms */
enum { MIRT_K_PREP = 0, MIRT_K_BIN = 1, MIRT_K_TRACE = 2, MIRT_K_DOF = 3,
       MIRT_K_RASTER_SETUP = 4, MIRT_K_RASTER_FRAG = 5, MIRT_K_RASTER_RESOLVE = 6, MIRT_K_CLEAR = 7 };

/* ---- lifetime ------------------------------------------------------------------------------------ */

/* One context per process, driven from one thread at a time (the reference is a single-threaded main loop); the calls
 * are not re-entrant.  Several processes may share a GPU (one process per GPU under torch.distributed). */

/* Replaces nothing in the reference (it has no device).  Selects HIP device `device` (use the process's
 * LOCAL_RANK under torch.distributed), checks it is gfx950, creates the library stream. */
MIRT_API int mirt_init(int device);
MIRT_API void mirt_shutdown(void);
MIRT_API const char *mirt_last_error(void);
MIRT_API int mirt_abi_version(void);
/* When on, every call and every kernel launch is bracketed by hipEvents on the library stream and
 * mirt_stats.gpu_ms / kernel_ms are filled (costs a few microseconds per event; off by default). */
MIRT_API int mirt_set_profiling(int on);
/* Blocks until all work queued by the library has finished. */
MIRT_API int mirt_sync(void);
/* The library's hipStream_t (as void*), so a caller can order its own work around ours (wait for an event before a
 * call, record one after it).  With several frames in flight (below) it is the stream of the most recent call only:
 * order with mirt_sync() instead. */
MIRT_API void *mirt_stream(void);
/* How many *_device frames may be in flight at once: 1 (default; calls run in order on one stream) up to 4 (calls take
 * that many streams in turn; the next frames are dispatched, and run where the device has room, while the previous ones
 * drain -- the kernels of a frame are short dependent chains, and several frames fill each other's gaps).  With k frames
 * in flight the caller must give k consecutive frames DIFFERENT output planes -- the double (k-fold) buffering a render
 * loop that presents one frame while drawing the next already has (the reference's SDL_UpdateRect after Draw(),
 * raytracer.cpp:653); frames i and i + k share a stream and may share planes -- and mirt_sync() before reading them.
 * Every scratch buffer a frame writes (origin and bin tables, raster keys, depth-of-field planes, counters) exists once
 * per stream. */
MIRT_API int mirt_set_frames_in_flight(int frames);

/* ---- host surfaces --------------------------------------------------------------------------------- */

/* The surface PutPixelSDL writes (SDL_Surface::pixels of InitializeSDL's SDL_SetVideoMode, SDLauxiliary.h:31-52) is ordinary
 * pageable memory; a frame copied into it is staged by the runtime at about half the link rate.  Registering it once --
 * pixels, h * pitch bytes -- pins and maps it: mirt_raytrace / mirt_rasterise / their _ex forms then deliver every frame whose
 * out_xrgb rows lie inside a registered surface by one DMA copy into the pinned pages (MIRT_HOST_PATH=direct: the render
 * kernels store the XRGB words straight into the mapped surface instead, no staging plane).  On the MI355X box of this
 * repository's measurements neither beats the pageable path (the link gives 37-46 GB/s either way, see bench.py host_path);
 * the calls exist for hosts whose pageable copies are slower.  The caller keeps the memory alive until
 * mirt_surface_unregister / mirt_shutdown.  Up to 4 surfaces. */
MIRT_API int mirt_surface_register(void *pixels, size_t bytes);
MIRT_API int mirt_surface_unregister(void *pixels);

/* Asynchronous frames into a registered surface: the frame is rendered and copied (one stream-ordered DMA copy into the
 * pinned pages) on the library stream and the call returns as soon as both are queued; mirt_sync() -- the SDL_UpdateRect of the
 * loop (raytracer.cpp:653, rasteriser.cpp:528) -- completes it.  With mirt_set_frames_in_flight(2) the copy of frame i overlaps
 * the render of frame i + 1, which is what makes the host boundary run at the rate of the link (bench.py host_path.async):
 * consecutive frames then need DIFFERENT surfaces (double buffering), exactly as the *_device calls do.  out_xrgb must lie in a
 * surface registered above (MIRT_ERR_INVALID_ARGUMENT otherwise: pageable memory cannot take a stream-ordered copy).  Same
 * pixels as mirt_raytrace / mirt_rasterise: interior only for the ray tracer, the whole surface for the rasteriser. */
MIRT_API int mirt_raytrace_async(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                                 int mode, uint32_t *out_xrgb, int pitch_bytes);
MIRT_API int mirt_rasterise_async(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                                  uint32_t *out_xrgb, int pitch_bytes);

/* ---- scene --------------------------------------------------------------------------------------- */

/* Replaces the global `vector<Triangle> triangles` (raytracer.cpp:28, rasteriser.cpp:64): copies n
 * triangles (n x 15 floats, reference AoS order) to the device and precomputes the per-triangle edge
 * data.  `culled` (nullable, n bytes) is Triangle::isCulled of the rasteriser (rasteriser/Source/
 * TestModel.h:18); the ray tracer ignores it.  The caller may free both arrays on return. */
MIRT_API int mirt_scene_upload(const float *tris15, const uint8_t *culled, int n);
/* Replaces the per-frame `triangles[i].isCulled = ...` writes of the rasteriser's Update()
 * (rasteriser.cpp:404-447) for an already uploaded scene. */
MIRT_API int mirt_scene_set_culled(const uint8_t *culled, int n);
MIRT_API int mirt_scene_size(void);

/* LoadTestModel (raytracer/Source/TestModel.h:51-192): writes the 30 Cornell-box triangles, returns 30. */
MIRT_API int mirt_scene_cornell(float *tris15);
/* Synthetic soup for the benchmark configs (no reference counterpart; generator defined in SURVEY
 * section 8(d)): mt19937(seed), centres U[-1,1]^3, two edges U[-s,s]^3, colours U[0.15,0.75]^3,
 * normal by the reference's Triangle::ComputeNormal rule. */
MIRT_API int mirt_scene_soup(uint32_t seed, int n, float s, float *tris15);
/* The cull step of the rasteriser's Update() (rasteriser.cpp:385-447, InCuboid :451-458), host side.
 * flags: bit0 = BACKFACE_CULLING_ENABLED, bit1 = FRUSTUM_CULLING_ENABLED (both default on, :25-26). */
MIRT_API int mirt_cull(const float *tris15, int n, const mirt_view *view, int flags, uint8_t *culled);
/* The same step on the device for the uploaded scene (one thread per triangle; the flags go straight into the scene's
 * device-side cull array, no host copy either way) -- what replaces the loop at rasteriser.cpp:404-447 once meshes are
 * large.  mirt_scene_get_culled reads the flags back (the reference's triangles[i].isCulled).  The flags are those of the
 * NEXT mirt_rasterise* call(s), as Update() culls right before Draw(): with several frames in flight they are written for,
 * and on, the stream the next call takes, so the frames still running on the other streams keep their own; a rasterised
 * frame that lands on another stream (the second row band of a frame, or after a ray-traced frame took that turn) brings
 * the most recent flags over, ordered behind the cull kernel. */
MIRT_API int mirt_cull_device(const mirt_view *view, int flags);
MIRT_API int mirt_scene_get_culled(uint8_t *culled, int n);
/* LoadSTL::LoadSTLFile (rasteriser/Source/LoadSTL.cpp:17-97): reads an ASCII STL the way the reference does (every line
 * containing "outer" is followed by three vertex lines), multiplies every coordinate by -scale (the reference: 0.05f),
 * sets the colour (the reference: 0.5, 0.5, 0.5) and recomputes the normals.  Returns the number of facets in the file;
 * writes the first max_tris of them when tris15 is not NULL (call with NULL first to size the array). */
MIRT_API int mirt_scene_load_stl(const char *path, float scale, const float *colour3, float *tris15, int max_tris);

/* ---- moving and device-resident scenes ------------------------------------------------------------- */

/* The reference changes `triangles` in place whenever it likes (LoadTestModel scales and flips its vertices, TestModel.h:172-191;
 * LoadSTL scales the mesh; a game loop would move enemy1.stl every frame) and recomputes the normals afterwards.  These calls are
 * that for the uploaded scene, without a trip through host memory.
 *
 * Ordering, for the four calls that change the scene (mirt_scene_upload_device, mirt_scene_update_device, mirt_scene_update,
 * mirt_scene_transform): each begins as mirt_scene_upload does -- it waits for every library stream and for the device, so frames in
 * flight finish on the OLD scene and a source buffer in device memory is complete whatever stream wrote it -- and returns with the
 * scene, its per-triangle tables, its bounding box and its finiteness flag current (one 32-byte read-back behind the kernels).
 * Every frame or query queued afterwards, on any stream, sees the new scene; every cache the library keeps (binning passes, light
 * and query cubes, query rows, rasteriser sizing) is keyed by the scene's version and is rebuilt, not refitted.  A double-buffered
 * scene, which would let an update overlap frames in flight, is not provided.
 *
 * Arguments are checked before anything touches the device: MIRT_ERR_NOT_INITIALISED first; MIRT_ERR_INVALID_ARGUMENT for
 * first < 0, count < 0, a NULL array with count > 0 or an array that is not 4-byte aligned; MIRT_ERR_NO_SCENE without a scene;
 * MIRT_ERR_INVALID_ARGUMENT for first + count > n.  count == 0 then does nothing and returns MIRT_OK. */

/* mirt_scene_upload with both arrays in DEVICE memory (d_culled nullable, n bytes): the scene, tables and flags that result are
 * those of uploading the same values from the host.  A new n reallocates as the host upload does. */
MIRT_API int mirt_scene_upload_device(const void *d_tris15, const void *d_culled, int n);
/* Replaces triangles [first, first + count) of the uploaded scene with count x 15 floats from device / host memory (the host form is
 * staged through the device); n and the cull flags stay as they are.  The bounding box is taken over the whole scene again: it
 * can shrink. */
MIRT_API int mirt_scene_update_device(int first, int count, const void *d_tris15);
MIRT_API int mirt_scene_update(int first, int count, const float *tris15);
/* Moves triangles [first, first + count) in place, on the device: each of the three vertices becomes rot9 * v + translate3 -- GLM's
 * column-major mat3 * vec3 in its written order (per row: three products summed left to right), then one add per component, no
 * contraction; Draw() does the same to its ray direction (cameraRot * d, raytracer.cpp:580) -- and the normal is recomputed by
 * Triangle::ComputeNormal, normalize(cross(v2 - v0, v1 - v0)) (TestModel.h:26-31).  The colour is untouched.  Repeated calls
 * compound their rounding: a caller who needs a drift-free pose keeps the rest pose and sends the posed rows with
 * mirt_scene_update*, or leaves the rest pose to the library (mirt_scene_set_objects, mirt_scene_pose below). */
MIRT_API int mirt_scene_transform(int first, int count, const float rot9[9], const float translate3[3]);
/* The same arithmetic on n triangles of a HOST array, bit for bit (pure arithmetic, no device: to mirt_scene_transform what mirt_cull
 * is to mirt_cull_device) -- for a caller that keeps a host mirror of the scene. */
MIRT_API int mirt_transform(float *tris15, int n, const float rot9[9], const float translate3[3]);
/* Reads triangles [first, first + count) back into count x 15 floats; complete on return. */
MIRT_API int mirt_scene_download(int first, int count, float *tris15);
/* The values the library decides with, whichever way the scene arrived: finite = every one of the 15 n floats is below 1e8 in
 * magnitude (a scene that is not takes the brute-force paths); the box is fminf / fmaxf over the vertex coordinates (a NaN is
 * skipped, an infinity counts, an axis without a number stays at +inf / -inf); version changes with every change of the triangles.
 * (A struct tag, not a typedef: C keeps tags apart from function names, as with stat.) */
struct mirt_scene_info {
    int32_t n;
    int32_t finite;
    float bbox_lo[3];
    float bbox_hi[3];
    uint64_t version;
};
MIRT_API int mirt_scene_info(struct mirt_scene_info *out);

/* ---- posed scenes: many objects moved from a rest pose in one call ---------------------------------- */

/* The game loop above moves MANY meshes every frame, each from the pose it was loaded in.  One mirt_scene_transform per mesh pays
 * the fixed part of a scene change (two waits, the launches, the read-back) once per mesh, and compounds its rounding from frame
 * to frame; thirty-two enemies loaded from one enemy1.stl are thirty-two copies of it on the host.  Here the library keeps a REST
 * pose on the device, the caller declares objects as (rest range -> scene range) maps, and one call poses any subset of them from
 * the rest rows: one launch chain, one bounds pass, one read-back, however many objects move. */
typedef struct mirt_object { int32_t rest_first; int32_t scene_first; int32_t count; } mirt_object;   /* 12 bytes */

/* Declares the objects of the uploaded scene and the rest pose they are posed from: object k writes rest rows [rest_first,
 * rest_first + count) to scene rows [scene_first, scene_first + count).  rest15: nrest x 15 floats in host memory, copied to the
 * device (the caller may free it on return); instances may share rest ranges.  rest15 == NULL with nrest == 0: the rest pose is a
 * snapshot of the scene as it is now (a device-to-device copy; nrest becomes n).  count == 0 is allowed: such an object is never
 * work.  Scene ranges must be pairwise disjoint, rest ranges may overlap.  nobjects == 0 forgets the objects and frees the rest
 * pose.
 *
 * The call does not change the scene: it bumps no version, invalidates no cache and drains no stream (the scene only changes
 * inside calls that return with it complete, so a plain copy is ordered).  The objects and the rest pose are forgotten by
 * mirt_scene_upload, mirt_scene_upload_device and mirt_shutdown.  mirt_scene_update* and mirt_scene_transform change live rows
 * only: the rest pose stays, and the next pose of that object overwrites what they wrote.
 *
 * Checks, in this order, before anything touches the device: MIRT_ERR_NOT_INITIALISED; MIRT_ERR_INVALID_ARGUMENT for nobjects < 0,
 * nrest < 0, NULL objects with nobjects > 0, NULL rest15 with nrest > 0, a rest15 that is not 4-byte aligned; MIRT_ERR_NO_SCENE;
 * MIRT_ERR_INVALID_ARGUMENT for a negative field, a rest range outside [0, nrest) ([0, n) for the snapshot), a scene range outside
 * [0, n), two scene ranges that overlap. */
MIRT_API int mirt_scene_set_objects(const mirt_object *objects, int nobjects, const float *rest15, int nrest);
/* Poses `count` objects from the rest pose.  which[i] (host memory) is an index into the declared list, NULL means objects
 * 0 .. count - 1; xforms12[12 i ..] = { rot9 column-major, translate3 } is that object's transform.  Every triangle of a listed
 * object becomes the rest row moved as mirt_scene_transform moves a row, bit for bit, the normal recomputed, the colour the rest
 * row's.  Objects not listed keep their live rows -- their last pose --, and so do triangles that belong to no object and the cull
 * flags.  The call is never cumulative: posing with A and then with B leaves exactly the scene that posing once with B leaves.
 *
 * Ordering and result are those of the four calls above, to the letter: the call waits for every library stream and for the
 * device, so frames in flight finish on the old scene, and returns with the scene, its tables, its bounding box (taken over all n
 * again) and its finiteness flag current; the version moves on and every cache is rebuilt.  Three launches and one 32-byte
 * read-back, whatever count is.
 *
 * Checks, in this order: MIRT_ERR_NOT_INITIALISED; MIRT_ERR_INVALID_ARGUMENT for count < 0 or NULL xforms12 with count > 0;
 * MIRT_ERR_NO_SCENE; MIRT_ERR_INVALID_ARGUMENT when no objects are declared, for count above the declared number when which is
 * NULL, an index outside the list, an index listed twice.  count == 0 then does nothing and returns MIRT_OK, and so does a list
 * whose objects are all empty. */
MIRT_API int mirt_scene_pose(const int32_t *which, int count, const float *xforms12);
/* The same arithmetic on HOST arrays, bit for bit (pure, no device, no mirt_init: to mirt_scene_pose what mirt_transform is to
 * mirt_scene_transform) -- for a caller that keeps a host mirror of the scene.  tris15 (n x 15 floats) is written in place, and
 * only the rows of listed objects are touched; rest15 == NULL with nrest == 0 takes tris15 as it arrives for the rest pose.  The
 * checks of both calls above without the two statuses that need the library, with n and nrest as given: MIRT_ERR_INVALID_ARGUMENT
 * also for n < 0 and a NULL tris15 with n > 0. */
MIRT_API int mirt_pose(const float *rest15, int nrest, const mirt_object *objects, int nobjects,
                       const int32_t *which, int count, const float *xforms12, float *tris15, int n);

/* Soft shadows (SOFT_SHADOWS_ENABLED / SOFT_SHADOWS_SAMPLES / randomPositions, raytracer.cpp:40-41,84,186-190,
 * 272-287): when samples > 1 every light k is replaced in DirectLight by `samples` jittered positions
 * positions[(k*samples + i)*3 .. +2] with 1/samples of its power each.  The caller generates the positions (the
 * reference draws them with rand() in AddLight; host/mirt_draw.hpp does the same).  samples <= 1 switches back to
 * hard shadows.  samples in [2, MIRT_MAX_LIGHT_POSITIONS], samples <= npositions <= MIRT_MAX_LIGHT_POSITIONS; a call with
 * nlights lights (at most MIRT_MAX_LIGHTS) needs nlights x samples <= npositions positions.  With the reference's 16 samples
 * that is its own limit of sixteen lights.
 * More than MIRT_MAX_LIGHTS positions.  The fused frame kernels carry MIRT_MAX_LIGHTS positions.  A ray-traced frame with more
 * (every mirt_raytrace* form, row bands and depth of field included) is rendered deferred: its primary rays without light, then
 * DirectLight over one hit record per pixel in passes of at most MIRT_MAX_LIGHTS positions -- DirectLight's two accumulators
 * are carried from pass to pass, so every bit is the single loop's --, then pixelColours.  The frame's `mode` chooses the
 * passes' kernels as it chooses the frame's (mirt_set_query_mode does not govern frames); mirt_stats reports the primary pass's
 * mode_used and shadow_rays = positions x pixels that hit.  Supersampling (mirt_set_antialiasing) shades a carried record per
 * sub-ray, which one record per pixel cannot follow: a frame with more than MIRT_MAX_LIGHTS positions AND supersampling on
 * returns MIRT_ERR_INVALID_ARGUMENT unless mirt_set_supersampled_many_lights (below) is on, which renders it.
 * MIRT_MANY_LIGHTS_MIN (environment, default 33) lowers the position count from which frames without supersampling are
 * deferred. */
MIRT_API int mirt_set_soft_shadows(int samples, const float *positions, int npositions);

/* Depth of field (DOF_ENABLED / DOF_KERNEL_SIZE / FOCAL_LENGTH, raytracer.cpp:43-45,613-640; rasteriser.cpp:29-31,
 * 494-513): kernel_size > 1 blurs pixelColours with a kernel_size x kernel_size stencil weighted by the centre pixel's
 * |distance - focal_length| before PutPixelSDL, for both renderers (the reference uses 8 with 1.3 / 1.9).  Taps whose
 * flat index leaves the frame are undefined behaviour in the reference; here they contribute nothing.  out_rgb keeps
 * the unblurred pixelColours, as in the reference.  kernel_size <= 1 switches it off. */
MIRT_API int mirt_set_depth_of_field(int kernel_size, float focal_length);

/* Supersampling (AA_ENABLED / AA_SAMPLES, raytracer.cpp:37-38,549-599): samples > 1 fires samples x samples sub-rays
 * per pixel and averages them, reproducing the reference's loop exactly (the pixel's closest-hit record is carried
 * across the sub-rays, x1 only advances after a sub-ray that hit).  samples <= 1 switches it off.  The reference uses 3.
 * Up to MIRT_MAX_LIGHTS light positions the fused frame kernels render such a frame; with more, see below. */
MIRT_API int mirt_set_antialiasing(int samples);

/* Supersampled frames with more than MIRT_MAX_LIGHTS light positions (the reference's AA_ENABLED + SOFT_SHADOWS_ENABLED with a
 * third light: 48 positions, 3 x 3 sub-rays).  on != 0: such a frame -- every mirt_raytrace* form, row bands, depth of field,
 * asynchronous and sharded frames included -- is rendered by shading each record a pixel carries ONCE: the carried record only ever
 * moves to a closer (or equal) hit and DirectLight depends on the record alone, so consecutive sub-rays that shade the same record
 * add the same bits; the pixel's sum is "c_0 times R_0, then c_1 times R_1, ..." added one term at a time, bit for bit the
 * reference's.  The band is rendered in chunks of rows inside a scratch budget per stream (MIRT_AA_DEFER_SCRATCH_MB, default 256;
 * MIRT_AA_DEFER_ROWS forces the rows of a chunk); `mode` chooses the primary sub-rays' kernel (a cube around the camera, or a sweep)
 * and the DirectLight passes' kernels; mirt_stats reports primary_rays = pixels x samples^2, shadow_rays = positions x sub-rays
 * that hit, and mode_used = MIRT_RT_BINNED when the primary sub-rays walked the camera's cube.  MIRT_AA_DEFER_MIN (environment,
 * default 33) lowers the position count from which supersampled frames take this path while it is on.
 * Off by default: the frame is then refused as described at mirt_set_soft_shadows.  Flipping the default is left to a later
 * change.  Context state: mirt_shutdown puts it back to 0. */
MIRT_API int mirt_set_supersampled_many_lights(int on);
/* The last such frame: the sub-rays that hit (each shades the carried record in the reference) and the records actually shaded.
 * Waits for the frame's stream; zeros when no such frame has run. */
MIRT_API int mirt_get_supersample_stats(uint64_t *hit_subrays, uint64_t *records_shaded);

/* ---- ray tracer: replaces Draw() + CalculateDOF() of raytracer.cpp:547-656 -------------------------- */

/* One frame into host buffers.  out_xrgb (required) is the SDL surface's `pixels` (XRGB8888, the words
 * PutPixelSDL stores, SDLauxiliary.h:75-80) with `pitch_bytes` per row; as in the reference only interior
 * pixels x in [1,W-2], y in [1,H-2] are written (raytracer.cpp:618-620) -- border words are left untouched.
 * out_rgb (nullable, W*H*3 floats) receives `pixelColours` (raytracer.cpp:88,600); out_index (nullable,
 * W*H int32) receives closestIntersections[].triangleIndex, -1 where the primary ray missed (:98,243-247). */
MIRT_API int mirt_raytrace(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                           int mode, uint32_t *out_xrgb, int pitch_bytes, float *out_rgb, int32_t *out_index);

/* Same frame, rows [y0, y1) only, into DEVICE buffers the caller owns (e.g. torch tensors), queued on the
 * library stream without a host sync; used for screen-band sharding across GPUs and for benchmarking with
 * resident buffers.  d_xrgb points at row 0 of a full-frame (or band-relative, see row_origin) surface:
 * row y is written at d_xrgb + (y - row_origin) * pitch_bytes.  d_rgb / d_index (nullable) likewise use
 * row stride W.  Interior-only rule as above (relative to the FULL frame). */
MIRT_API int mirt_raytrace_device(const mirt_view *view, const mirt_light *lights, int nlights,
                                  const float *indirect, int mode, int y0, int y1, int row_origin,
                                  void *d_xrgb, int pitch_bytes, void *d_rgb, void *d_index);

/* The same two calls with the rest of `struct Intersection` (raytracer.cpp:91-98): out_distance / d_distance (nullable, W*H
 * floats, row stride W) receives closestIntersections[].distance -- the FLT_MAX of Update()'s reset (:335-339) where the
 * primary ray missed -- and out_position / d_position (nullable, W*H*3 floats) closestIntersections[].position (0 where it
 * missed; the reference leaves it uninitialised).  With depth of field on, the rows the blur reads beyond the band are
 * rendered too and their entries of these two planes are written as well. */
MIRT_API int mirt_raytrace_ex(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                              int mode, uint32_t *out_xrgb, int pitch_bytes, float *out_rgb, int32_t *out_index,
                              float *out_distance, float *out_position);
MIRT_API int mirt_raytrace_device_ex(const mirt_view *view, const mirt_light *lights, int nlights,
                                     const float *indirect, int mode, int y0, int y1, int row_origin,
                                     void *d_xrgb, int pitch_bytes, void *d_rgb, void *d_index,
                                     void *d_distance, void *d_position);

/* ---- ray queries: ClosestIntersection (raytracer.cpp:202-257) and DirectLight (:265-327) for the caller's own rays ---- */

/* The two workhorses of the reference are free functions, and Draw() is only one of their callers: a mirror bounce, a mouse pick,
 * an occlusion probe or a second light pass calls them with rays of its own.  These entry points are those two functions, one
 * call per array element, against the uploaded scene (mirt_intersect* by brute force, as ClosestIntersection is; the shadow rays
 * of mirt_direct_light* through the light-cube bins where that pays: mirt_set_query_mode; rays that share their origin through a
 * cube around it: mirt_intersect_from*, below). */
typedef struct mirt_ray { float start[3]; float dir[3]; } mirt_ray;                      /* 24 bytes */
/* struct Intersection (raytracer.cpp:91-96), same field order and size (20 bytes). */
typedef struct mirt_hit { float position[3]; float distance; int32_t index; } mirt_hit;

/* hits[i] is the in/out `closestIntersection` argument of one ClosestIntersection(rays[i].start, rays[i].dir, triangles, hits[i])
 * call: the caller puts in Update()'s reset (distance = FLT_MAX, :335-339; index = -1) for a fresh query, or the record an earlier
 * ray left.  A triangle the reference accepts replaces the record when record.distance >= distance (:243): equal distances go to
 * the later index, an incoming record loses every tie, an incoming distance that is negative or NaN is never replaced and +inf
 * by any hit; a ray that accepts nothing closer leaves all 20 bytes of its record untouched.  dir is used as given, not
 * normalised (:229 negates it).  mirt_intersect: host arrays, complete on return.  mirt_intersect_device: device arrays, queued
 * like the *_device frames (the streams of mirt_set_frames_in_flight in turn; mirt_sync() completes it).  nrays == 0 does nothing.
 * Queries leave mirt_get_stats alone: it keeps reporting the last render call. */
MIRT_API int mirt_intersect(const mirt_ray *rays, int nrays, mirt_hit *hits);
MIRT_API int mirt_intersect_device(const void *d_rays, int nrays, void *d_hits);
/* out_rgb[3*i ..] = DirectLight(hits[i]) for the given lights, with the reference's `result2 += result` double count (:319-322)
 * and the final multiply by the triangle's colour (:325-326), under the current mirt_set_soft_shadows state.  Only position and
 * index of a record are read; an index outside [0, n) -- the reference would index outside `triangles` -- yields (0, 0, 0).
 * nlights <= MIRT_MAX_LIGHTS and nlights x samples <= MIRT_MAX_LIGHT_POSITIONS.  More than MIRT_MAX_LIGHTS positions are answered
 * in passes over consecutive ranges of at most MIRT_MAX_LIGHTS positions (a range may end inside a light): the accumulators
 * `result` and `result2` travel between the passes in per-stream scratch (24 bytes per record), so the additions, their operands
 * and their order are the single loop's and no bit differs.  Binned, every pass walks a kept cube of its own range's positions. */
MIRT_API int mirt_direct_light(const mirt_hit *hits, int nhits, const mirt_light *lights, int nlights, float *out_rgb);
MIRT_API int mirt_direct_light_device(const void *d_hits, int nhits, const mirt_light *lights, int nlights, void *d_rgb);

/* How mirt_direct_light* walks its shadow rays.  A shadow ray of DirectLight starts at a light position whatever the record, so the
 * six-face light cubes of the binned frame path hold every one of a query's shadow rays: BINNED lets each ray test only the
 * triangles of its cube bin (bit-identical results); the cube of (scene, light positions) is built by the first call that needs it,
 * kept for later calls and shared by the streams -- or it is the frame path's own cube, when the binned frames hold one for the
 * same lights.  BRUTE sweeps every triangle for every shadow ray.  AUTO bins when the scene has MIRT_BIN_THRESHOLD triangles or
 * more and records x light positions x triangles >= 4e7 (the frame path's rule), or when a cube for the call's lights is already
 * held.  Whatever the mode, a call the frame path would not bin (a scene or light position outside the filter's proven range)
 * takes the brute-force kernel.  Context state: mirt_shutdown puts it back to AUTO. */
typedef enum mirt_query_mode { MIRT_QUERY_AUTO = 0, MIRT_QUERY_BRUTE = 1, MIRT_QUERY_BINNED = 2 } mirt_query_mode;
MIRT_API int mirt_set_query_mode(int mode);
/* The last mirt_direct_light* call (mirt_get_stats stays with the last render call).  cube_source: 0 no cube (brute force), 1 built
 * by this call, 2 kept from an earlier query, 3 the frame path's.  The four counters are filled for a binned call made with
 * mirt_set_profiling(1) and zero otherwise: shadow rays (records inside the scene x light positions), candidate rows offered to
 * them, tests executed, and records for which a light position swept its whole table because the cube's ray family does not
 * cover their shadow ray (a position that is not finite, equals the light or lies beyond float range of it).
 * A call of several passes (more than MIRT_MAX_LIGHTS positions): the four counters are summed over the passes (fallback_records
 * counts a record once per pass in which it swept), cube_bins and shells are the last pass's, and cube_source is 0 none, 1 some
 * pass built its cube, 2 every pass's cube was held -- 3 only for a call of one pass.  Binned or brute is decided once for the
 * whole call, `held` meaning that every pass's cube is. */
typedef struct mirt_query_stats {
    int32_t mode_used;                /* MIRT_QUERY_BRUTE or MIRT_QUERY_BINNED                   */
    int32_t cube_source;
    int32_t cube_bins;                /* bins per face side, 0 without a cube                     */
    int32_t shells;                   /* depth shells per bin                                     */
    uint64_t shadow_rays;
    uint64_t candidates;
    uint64_t tests;
    uint64_t fallback_records;
} mirt_query_stats;
/* Waits for the stream of the last DirectLight query. */
MIRT_API int mirt_get_query_stats(mirt_query_stats *out);

/* ---- origin fans: ClosestIntersection for many directions from ONE origin ---- */

/* ClosestIntersection(origin, dirs[i], triangles, hits[i]) for i in [0, nrays): exactly mirt_intersect with
 * rays[i] = { origin, dirs[i] }, bit for bit, for every ray and every incoming record.  A cube-map or environment probe, an
 * omnidirectional camera, a point light's shadow map, a visibility fan from a probe point, a pick from the eye: rays that share their
 * origin share the frame path's per-origin tables, and a six-face cube around the origin holds every direction, so each ray tests
 * only the triangles of its cube bin, nearest depth shells first, and stops where nothing closer than its record can follow.
 * dirs3: nrays x 3 floats, used as given and not normalised.  hits: the in/out records of mirt_intersect, with its rules (ties
 * to the later index, an incoming record loses every tie, a negative or NaN incoming distance is never replaced, +inf by any hit,
 * a ray that accepts nothing closer leaves all 20 bytes unwritten).  nrays == 0 does nothing.  The _device form is queued like
 * mirt_intersect_device (the streams in turn, mirt_sync() completes it); neither form touches mirt_get_stats or
 * mirt_get_query_stats.  mirt_set_query_mode governs these calls too: BRUTE sweeps the origin's table for every ray and never builds
 * a cube; BINNED builds the cube of (scene, origin) when it is not held -- one cube is kept, apart from DirectLight's --; AUTO bins
 * when the scene has 2000 triangles or more (measured: with its build the binned call is ahead of the sweep from one ray on at
 * 2000 and at 100 000 triangles), when it has MIRT_BIN_THRESHOLD triangles or more and rays x triangles >= 4e7 (the frame path's
 * figure, not measured for this use), or when the cube of this origin is already held.  A call the frame path would not bin (a scene or origin
 * coordinate beyond 1e8) sweeps under every mode; so does, per ray, a direction that is zero, not finite, or whose largest
 * component lies outside [2^-32, 2^19). */
MIRT_API int mirt_intersect_from(const float origin[3], const float *dirs3, int nrays, mirt_hit *hits);
MIRT_API int mirt_intersect_from_device(const float origin[3], const void *d_dirs3, int nrays, void *d_hits);
/* The last mirt_intersect_from* call; mirt_get_query_stats stays with the last DirectLight query, mirt_get_stats with the last
 * frame.  The struct's field names are DirectLight's: here cube_source is 0 none, 1 built by this call, 2 kept from an earlier
 * call; with profiling on and a binned call, shadow_rays = rays of the call, candidates = rows a ray stepped over before its
 * list's (moving) end, tests = those of them not beyond the ray's record, fallback_records = rays that swept the whole table.
 * Waits for the stream of that call. */
MIRT_API int mirt_get_fan_stats(mirt_query_stats *out);

/* ---- origin fans from MANY origins in one call (additions to ABI 4) ---- */

/* ClosestIntersection(origins[origin_of[i]], dirs[i], triangles, hits[i]) for i in [0, nrays): exactly mirt_intersect on the rays
 * { origins3[3 * origin_of[i] ..], dirs3[3 * i ..] }, bit for bit, for every ray and every incoming record.  A grid of light
 * probes, the shadow maps of all of a scene's point lights, an omnidirectional camera at several stations, visibility fans from a
 * handful of points: one call instead of one mirt_intersect_from* call -- one cube build, one host read-back -- per origin.
 * origins3: a HOST array of norigins x 3 floats in both forms (as `origin` of mirt_intersect_from_device).  origin_of: one int32
 * per ray; it may be NULL only when norigins == 1 (every ray takes origin 0: the call equals mirt_intersect_from*).  Rays come in
 * any order; the lanes of a wave may hold different origins.  Records and directions: mirt_intersect's rules to the letter, as
 * above.  Checks, in this order: MIRT_ERR_NOT_INITIALISED; MIRT_ERR_INVALID_ARGUMENT for norigins < 0, nrays < 0, a NULL array with
 * a positive count, norigins == 0 with nrays > 0, a NULL origin_of with norigins > 1; MIRT_ERR_NO_SCENE.  nrays == 0 does
 * nothing.  The host form also checks every origin_of[i] against [0, norigins) before anything touches the device
 * (MIRT_ERR_INVALID_ARGUMENT, nothing written); the device form cannot look: there a ray whose index lies outside the range reads
 * nothing out of bounds and leaves its record's 20 bytes unwritten.  The _device form is queued like mirt_intersect_from_device;
 * neither form touches mirt_get_stats or mirt_get_query_stats.
 * How it is answered.  The origins go into cubes of up to MIRT_MAX_LIGHTS positions each (fewer where the sort's key space
 * allows fewer at the scene's grid), built in one binning chain per cube; a call with more origins runs in passes over consecutive
 * ranges of the list, each pass over all rays.  One cube per pass is kept for these calls, up to eight, apart from
 * mirt_intersect_from*'s and DirectLight's, keyed by scene version, positions and their order -- a repeated call of up to 256
 * origins builds nothing --; a pass whose positions are exactly those the frame path's or DirectLight's cube holds reads that cube
 * and builds nothing.  mirt_set_query_mode: BRUTE never builds a cube (the rays are
 * written out on the device and go through mirt_intersect_device's kernels); BINNED bins whenever the frame path would; AUTO uses
 * the single fan's rule -- 2000 triangles or more, or MIRT_BIN_THRESHOLD triangles or more and nrays x triangles >= 4e7, or the
 * cubes of these origins are held -- which is MEASURED FOR ONE ORIGIN ONLY, with one condition more that the measurement of
 * several origins showed (profiles/ray_query_bench.txt, section `fans`): unless the cubes are held, a call of at most
 * MIRT_QUERY_WAVE_RAYS rays (4096) does not bin -- the brute path answers those a wave per ray and was ahead of every build.
 * Measured there (1 .. 128 origins x 64 .. 65536 rays each, 2000 and 100 000 triangles): one call with its builds was behind K
 * mirt_intersect_from_device calls on the same rays nowhere (K = 32: 9 to 30 times ahead); under AUTO it stayed behind
 * BRUTE in two cells at 2000 triangles, 4 origins x 4096 rays (0.60 against 0.53 ms) and 128 origins x 64 rays (1.30 against 0.53
 * ms).  Whatever the mode, the WHOLE call takes the brute path when the frame path would not bin one of its parts: a scene
 * coordinate, or any component of any origin, that is not finite or not below 1e8. */
MIRT_API int mirt_intersect_fans(const float *origins3, int norigins, const int32_t *origin_of, const float *dirs3, int nrays, mirt_hit *hits);
MIRT_API int mirt_intersect_fans_device(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays, void *d_hits);
/* mirt_get_fan_stats reports the last call of EITHER fan entry point.  For mirt_intersect_fans* the four counters are summed over
 * the passes (fallback_records: the rays that swept), cube_bins and shells are the last pass's, and cube_source is 0 none, 1 some
 * pass built a cube, 2 every pass's cube was held from an earlier call, 3 every pass read the frame path's cube, 4 every pass read
 * DirectLight's cube.  mirt_intersect_from* keeps reporting 0 - 2. */

/* ---- occlusion queries: any-hit rays (additions to ABI 4) ---- */

/* "Is anything in the way before distance L": occluded[i] = 1 when some triangle that
 * ClosestIntersection(rays[i].start, rays[i].dir, ...) accepts (raytracer.cpp:239) has distance < max_distance[i], the distance
 * being the reference's glm::distance(start, pos) (:241-242); else 0.  This is DirectLight's shadow decision (:306-315) for the
 * caller's own ray and limit: a line-of-sight test, a shadow mask without shading, the visibility of N points from K observers, an
 * occlusion probe.  A ray stops at its first occluder instead of finding the closest hit.
 * The comparison is strict (`<`, :313): a limit that is NaN, negative or 0 gives 0 for every ray, and an accepted triangle whose
 * computed distance is +inf or NaN never occludes.  That is the reference's two-step form -- ClosestIntersection on a fresh record
 * (distance FLT_MAX), then `j.distance < limit` -- for every limit, +inf included.  max_distance == NULL: every limit is +inf.
 * `dir` is used as given and not normalised, so the caller scales the limit: the segment A -> B is dir = B - A with the limit
 * |B - A| * 0.99f, as the reference does it.
 * Every byte [0, nrays) is written, 0 or 1 -- there is no "left untouched" as with the hit records --, and nothing beyond.
 * nrays == 0 does nothing.  Checks: mirt_intersect's, in its order (MIRT_ERR_NOT_INITIALISED; MIRT_ERR_INVALID_ARGUMENT for nrays < 0
 * or a NULL rays / occluded array with a positive count; MIRT_ERR_NO_SCENE).  The _device form is queued like mirt_intersect_device
 * (the streams in turn, mirt_sync() completes it); neither form touches mirt_get_stats, mirt_get_query_stats or mirt_get_fan_stats.
 * Up to MIRT_QUERY_WAVE_RAYS rays (4096) a wave answers each ray and leaves the triangle list at the first occluder any lane finds;
 * beyond, a lane answers each ray and a workgroup ends its sweep when all its rays are settled. */
MIRT_API int mirt_occluded(const mirt_ray *rays, int nrays, const float *max_distance, uint8_t *occluded);
MIRT_API int mirt_occluded_device(const void *d_rays, int nrays, const void *d_max_distance, void *d_occluded);
/* The same for the rays { origins3[3 * origin_of[i] ..], dirs3[3 * i ..] }: mirt_occluded on those rays, byte for byte.  Arguments,
 * checks and their order are mirt_intersect_fans*' (origins3 a HOST array in both forms; origin_of may be NULL only when norigins ==
 * 1), with `occluded` in the place of the records.  The host form also checks every origin_of[i] against [0, norigins) before
 * anything touches the device (MIRT_ERR_INVALID_ARGUMENT, nothing written); in the device form a ray whose index lies outside the
 * range reads nothing out of bounds and its byte is written 0, under every mode.
 * How it is answered: as mirt_intersect_fans* -- the same passes over cubes of up to MIRT_MAX_LIGHTS origins, the SAME kept cubes
 * and the same sharing with the frame path's and DirectLight's cubes, so a cube that mirt_intersect_fans* built for these origins
 * serves this call and the reverse.  Each ray walks its bin's list front to back up to the depth shell its limit falls into, skips
 * rows that lie wholly beyond the limit and stops at its first occluder; a direction outside mirt_intersect_from's window sweeps
 * its origin's table up to the first occluder.  mirt_set_query_mode: BRUTE writes the rays out on the device and takes
 * mirt_occluded_device's kernels; BINNED bins whenever the frame path would; AUTO is mirt_intersect_fans*' rule unchanged: it was
 * measured for closest hits, and the sweep of this call puts the crossing in the same place (profiles/ray_query_bench.txt, section
 * `occluded`: brute ahead in every cell of at most 4096 rays; beyond, binning with its builds behind only at 2000 triangles and 4
 * origins, 0.50 - 0.53 against 0.47 - 0.49 ms). */
MIRT_API int mirt_occluded_fans(const float *origins3, int norigins, const int32_t *origin_of, const float *dirs3, int nrays,
                                const float *max_distance, uint8_t *occluded);
MIRT_API int mirt_occluded_fans_device(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays,
                                       const void *d_max_distance, void *d_occluded);
/* The last mirt_occluded* call of either pair, in mirt_query_stats' fields.  mirt_occluded* itself always reports MIRT_QUERY_BRUTE
 * and no cube.  For mirt_occluded_fans*: cube_source 0 - 4, cube_bins and shells as mirt_get_fan_stats reports them for
 * mirt_intersect_fans*; with profiling on and a binned call, summed over the passes, shadow_rays = rays of the call whose index
 * names an origin, candidates = rows a ray stepped over before its occluder or its list's end, tests = those of them not beyond
 * the ray's limit, fallback_records = rays that swept their origin's table.  Waits for the stream of that call. */
MIRT_API int mirt_get_occlusion_stats(mirt_query_stats *out);

/* ---- ray queries along ONE direction: binned closest hits and occlusion (additions to ABI 4) ---- */

/* ClosestIntersection(origins[i], dir, triangles, hits[i]) for i in [0, nrays): exactly mirt_intersect on the rays { origins3[3 * i ..],
 * dir }, bit for bit, for every ray and every incoming record -- and mirt_occluded on the same rays, byte for byte.  Rays that share
 * their DIRECTION and differ in their start: an orthographic camera, a height or depth map, a directional (sun) shadow or exposure
 * map, many objects dropped to the ground, a parallel-beam scan.  For such a family the dot products of the test are affine in the
 * projection of the start onto a plane across dir, so a grid of B x B cells over the projection of the SCENE's bounding box holds
 * every start: each ray tests only the rows of its cell, front to back in depth shells along dir, and stops where nothing closer
 * than its record (or its limit) can follow.  The grid does not depend on the call's origins: no pass over them, no read-back for
 * them, and a repeated call with the same scene and direction builds nothing.
 * dir: a HOST array of three floats in both forms, used as given and not normalised.  origins3: nrays x 3 floats.  hits: the in/out
 * records of mirt_intersect, with its rules (ties to the later index, an incoming record loses every tie, a negative or NaN incoming
 * distance is never replaced, +inf by any hit, a record nothing replaced is left unwritten).  occluded / max_distance: as
 * mirt_occluded -- every byte [0, nrays) is written, a NULL limit array means +inf.  nrays == 0 does nothing.  Checks, in this order:
 * MIRT_ERR_INVALID_ARGUMENT for nrays < 0, a NULL origins or output array or a NULL dir with a positive count (the arguments
 * first: a malformed call is told so with or without a device); MIRT_ERR_NOT_INITIALISED; MIRT_ERR_NO_SCENE.  The host forms are complete on return; the _device forms are queued like mirt_intersect_device.  Neither
 * touches mirt_get_stats, mirt_get_query_stats, mirt_get_fan_stats or mirt_get_occlusion_stats.
 * mirt_set_query_mode: BRUTE writes the rays out on the device and takes mirt_intersect_device's / mirt_occluded_device's kernels;
 * BINNED builds the grid of (scene, dir) when it is not held -- one is kept, shared by the streams, forgotten with the scene --;
 * AUTO is the many-origin fans' rule, which this call's own sweep arrived at (profiles/ray_query_bench.txt, section `along`): more
 * than MIRT_QUERY_WAVE_RAYS (4096) rays and 2000 triangles or more (or MIRT_BIN_THRESHOLD triangles or more and nrays x triangles >=
 * 4e7), or the grid of this direction is held -- with its build the call was behind the brute path in every measured cell of at most
 * 4096 rays and ahead in every one from 16 384 rays on.  Under every mode the whole call takes the brute-force kernels
 * when the scene is not finite (a coordinate not below 1e8), when dir has a component that is not finite or its largest lies
 * outside [2^-32, 2^19), when a float cannot tell the grid's cells apart (a scene far thinner than it is far from the origin), or
 * when more than an eighth of the scene (and more than 64 triangles) is edge-on to dir or otherwise unfit for a cell -- those go on
 * one list every ray tests; mode_used then says BRUTE.  Per ray, a start that is not finite, or has a component beyond eight times
 * the scene's largest |coordinate| or not below 1e8, sweeps every row of the scene; a start whose projection falls outside the
 * grid tests the every-ray list alone. */
MIRT_API int mirt_intersect_along(const float dir[3], const float *origins3, int nrays, mirt_hit *hits);
MIRT_API int mirt_intersect_along_device(const float dir[3], const void *d_origins3, int nrays, void *d_hits);
MIRT_API int mirt_occluded_along(const float dir[3], const float *origins3, int nrays, const float *max_distance, uint8_t *occluded);
MIRT_API int mirt_occluded_along_device(const float dir[3], const void *d_origins3, int nrays, const void *d_max_distance, void *d_occluded);
/* The last call of either kind, in mirt_query_stats' fields: mode_used; cube_source 0 no grid, 1 built by this call, 2 kept;
 * cube_bins = cells per grid side; shells; and, with profiling on and a binned call, shadow_rays = rays of the call, candidates =
 * rows offered to them, tests = those of them not beyond the ray's record or limit, fallback_records = rays that swept the scene.
 * Waits for the stream of that call. */
MIRT_API int mirt_get_along_stats(mirt_query_stats *out);

/* ---- ray queries along SEVERAL directions in one call (additions to ABI 4) ---- */

/* ClosestIntersection(origins[i], dirs[dir_of[i]], triangles, hits[i]) for i in [0, nrays): exactly mirt_intersect on the rays
 * { origins3[3 * i ..], dirs3[3 * dir_of[i] ..] }, bit for bit, for every ray and every incoming record -- and mirt_occluded on the same
 * rays, byte for byte, for every limit.  The callers of the single-direction calls above with more than one direction: a sun study
 * over the hours of a day, six orthographic views, a parallel-beam scan from many angles, the ambient occlusion or sky visibility
 * of N points towards K directions -- one call, one launch per pass and one statistics record instead of K, and the rays in any
 * order: the lanes of a wave may hold different directions, and the same direction may appear twice in the list.
 * Each direction gets exactly the grid mirt_intersect_along builds for it; a GROUP of up to 32 directions (15 from 32 769 triangles
 * on, where a grid has 256 x 256 cells) shares one build: one pair list, one sort, one read-back.  A call of more directions runs in
 * passes over consecutive ranges of its list.  Pass p keeps its group in slot p % 8 of eight kept groups, apart from the grid of the
 * single-direction calls, under the scene and the pass's directions compared bit for bit and in order: a repeated call of up to eight
 * passes builds nothing, and neither family evicts the other's structure.  mirt_intersect_alongs and mirt_occluded_alongs share the
 * groups.
 * dirs3: a HOST array of ndirs x 3 floats in both forms, used as given.  dir_of: one index per ray; NULL only when ndirs == 1.
 * origins3, hits, occluded, max_distance: as mirt_intersect_along / mirt_occluded_along.  nrays == 0 does nothing.  Checks, in this
 * order: MIRT_ERR_INVALID_ARGUMENT for a negative count, a NULL array with a positive count, ndirs == 0 with nrays > 0 or a NULL dir_of
 * with ndirs > 1 (the arguments first, with or without a device); MIRT_ERR_NOT_INITIALISED; MIRT_ERR_NO_SCENE.  The host forms look at
 * every dir_of[i] before anything touches the device: an index outside [0, ndirs) is MIRT_ERR_INVALID_ARGUMENT and nothing is written.
 * The _device forms cannot: such a ray reads nothing out of bounds, its record's 20 bytes stay unwritten and its occlusion byte is
 * written 0, under every mode.
 * mirt_set_query_mode governs the calls: BRUTE writes the rays out on the device and takes mirt_intersect_device's /
 * mirt_occluded_device's kernels; BINNED builds the groups that are not held; AUTO is the single call's rule -- more than
 * MIRT_QUERY_WAVE_RAYS rays on a scene the fans would bin, or every group of the call is held.  When one direction of the call is unfit
 * for a grid (mirt_intersect_along's cases: outside the window, cells a float cannot tell apart, an every-ray list beyond its share)
 * or the scene is not finite, the WHOLE call takes the brute-force kernels and mode_used says BRUTE; the group remembers it, so the
 * next call builds nothing either.
 * mirt_get_along_stats reports the last call of either along family.  For these calls shadow_rays, candidates, tests and
 * fallback_records are summed over the passes, cube_bins and shells are the last pass's, and cube_source is 0 none, 1 some pass
 * built its group, 2 every pass's group was held. */
MIRT_API int mirt_intersect_alongs(const float *dirs3, int ndirs, const int32_t *dir_of, const float *origins3, int nrays, mirt_hit *hits);
MIRT_API int mirt_intersect_alongs_device(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, void *d_hits);
MIRT_API int mirt_occluded_alongs(const float *dirs3, int ndirs, const int32_t *dir_of, const float *origins3, int nrays, const float *max_distance, uint8_t *occluded);
MIRT_API int mirt_occluded_alongs_device(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, const void *d_max_distance, void *d_occluded);

/* ---- arbitrary rays through a cell grid (additions to ABI 4) ---- */

/* mirt_intersect* and mirt_occluded* take rays that share neither origin nor direction -- a mirror bounce, an ambient-occlusion
 * hemisphere, a segment test between arbitrary points -- and sweep every triangle for every ray.  mirt_set_ray_grid(1) makes these
 * four entry points (and no other) answer through a structure kept per scene version instead, whatever the ray count: G x G x G cells
 * over the scene's box (G the smallest power of two with G^3 >= 2 n, within [4, 128]) for the pairs the reference's test decides by
 * geometry, an index of the triangles' planes for the pairs it decides by rounding -- a ray nearly inside a triangle's plane may be
 * given a hit on a triangle it never comes near, and gets it here too --, and a list every ray tests for the triangles too sharp for
 * either.  Every record, all 20 bytes, and every occlusion byte equal the switch-off call's.  The structure is built by the first
 * call that needs it (one host read-back), shared by the streams, and forgotten when the triangles change.  A ray whose direction is
 * zero, not finite or outside [2^-32, 2^19) in its largest component, or whose start is not finite or lies more than two scene
 * extents (largest |coordinate| of the bounding box) from the origin, sweeps every triangle inside the same kernel.  A call the
 * frame path would not bin (a scene that is not finite), a scene so far from the origin that a float cannot tell the cells apart,
 * or one too many of whose triangles are for every ray (more than n / 8 and more than 64: `gave_up`, kept) sweeps as with the switch
 * off.  0 changes nothing anywhere.  mirt_set_query_mode neither affects the switch nor is affected by it; no AUTO rule uses the
 * grid.  Context state: mirt_shutdown puts it back to 0. */
MIRT_API int mirt_set_ray_grid(int on);
/* The last mirt_intersect* / mirt_occluded* call made with the switch on; waits for that call's stream.  mode_used is 0 while there
 * was no such call.  A mirt_occluded* call the grid answers (mode_used MIRT_QUERY_BINNED here) leaves mirt_get_occlusion_stats as it
 * was: that getter keeps reporting the last occlusion call that swept or walked a cube.  The six counters are filled for a binned call made with mirt_set_profiling(1) and zero otherwise. */
typedef struct mirt_ray_grid_stats {
    int32_t mode_used;                /* 0 no call; MIRT_QUERY_BRUTE or MIRT_QUERY_BINNED                          */
    int32_t source;                   /* 0 none, 1 built by this call, 2 kept                                      */
    int32_t gave_up;                  /* the every-ray list outgrew its share: the call swept                      */
    int32_t cells;                    /* G: cells per side                                                         */
    int32_t plane_bins;               /* (alpha, beta) bins per side and plane class                               */
    int32_t offset_bins;              /* delta bins per (alpha, beta) bin                                          */
    uint32_t pairs;                   /* rows of the structure: cells, plane index and every-ray list              */
    uint32_t plane_pairs;             /* ... of the plane index                                                    */
    uint32_t every_rows;              /* ... of the every-ray list                                                 */
    uint32_t reserved;
    uint64_t rays;
    uint64_t rows_cells;              /* rows offered from cells                                                   */
    uint64_t rows_planes;             /* ... from the plane index                                                  */
    uint64_t rows_every;              /* ... from the every-ray list                                               */
    uint64_t tests;                   /* exact-stage operand sets evaluated, the sweeping rays' included           */
    uint64_t swept_rays;              /* rays that swept every triangle                                            */
} mirt_ray_grid_stats;
MIRT_API int mirt_get_ray_grid_stats(mirt_ray_grid_stats *out);

/* ---- every hit along a ray, in order (additions to ABI 4) ---- */

/* mirt_intersect* answers with the ONE triangle ClosestIntersection ends on.  The loop that finds it (raytracer.cpp:202-257) accepts
 * a set of triangles per ray, each with a position p_j (:241) and a distance d_j (:242), and its record rule `closest.distance >=
 * distance` (:243) ranks them: j comes before k when d_j < d_k, or when d_j == d_k and j > k (the later index of a tie wins the
 * record).  mirt_intersect_ordered* returns the first max_hits triangles of that order per ray, bit for bit: the thickness of a part
 * along a ray, transparency layers, a point-in-mesh test by counting crossings, a bounce ray that skips the surface it starts on.
 * Eligible for ray i are the triangles j the reference's test accepts (:239) with FLT_MAX >= d_j -- what a fresh record takes, so
 * never a NaN or +inf distance -- and, when `after` is given, with d_j > a || (d_j == a && j < k) for a = after[i].distance, k =
 * after[i].index: float and signed-int comparisons as written, so a NaN a admits nothing, a negative a everything, and -0.0f
 * behaves as 0.0f; only distance and index of an `after` record are read.  The first min(max_hits, eligible) of them go to
 * hits[i * max_hits + 0 ...] in order, each a whole struct Intersection (p_j, d_j, j); counts[i] is that number; every remaining
 * slot of the ray is written as Update()'s reset (position 0, FLT_MAX, index -1).  Unlike mirt_intersect, `hits` is a pure output:
 * all max_hits * 20 bytes per ray and the count are always written.  So with after == NULL slot 0 (and counts[i] > 0) is
 * mirt_intersect on a fresh record, and a caller enumerates every hit of a ray by calling again with after[i] = the last record
 * written, for the rays whose count equals max_hits; an exhausted ray stays exhausted (a fresh record admits nothing).
 * 1 <= max_hits <= MIRT_MAX_ORDERED_HITS, otherwise MIRT_ERR_INVALID_ARGUMENT (and for a negative count, or NULL rays, hits or counts
 * with a positive one); nrays == 0 does nothing.  `after` must not overlap `hits`, except that with max_hits == 1 after == hits
 * exactly is allowed and peels in place: a ray's record is read before its slot is written.  mirt_intersect_ordered: host arrays,
 * complete on return.  mirt_intersect_ordered_device: device arrays, queued like mirt_intersect_device (the streams of
 * mirt_set_frames_in_flight in turn, no host sync; mirt_sync() completes it).  Under mirt_set_ray_grid(1) the call walks the cell
 * grid whenever its structure can be built and is then the call mirt_get_ray_grid_stats reports; otherwise it sweeps every
 * triangle.  mirt_set_query_mode does not affect it. */
#define MIRT_MAX_ORDERED_HITS 8
MIRT_API int mirt_intersect_ordered(const mirt_ray *rays, int nrays, const mirt_hit *after /* nullable */, int max_hits,
                                    mirt_hit *hits /* nrays * max_hits, ray-major */, int32_t *counts /* nrays */);
MIRT_API int mirt_intersect_ordered_device(const void *d_rays, int nrays, const void *d_after, int max_hits, void *d_hits, void *d_counts);

/* The same along parallel rays: the thickness of a part along a beam, X-ray and CT projections, voxelisation and point-in-mesh tests
 * by counting crossings along parallel lines, transparency layers under an orthographic camera.  The four calls are
 * mirt_intersect_ordered on the rays {origins[i], dir} or {origins[i], dirs[dir_of[i]]}, byte for byte: max_hits, `after`, the slots,
 * the counts and the overlap rule (after == hits only with max_hits == 1) are that call's, the directions, origins and dir_of those
 * of mirt_intersect_along* / mirt_intersect_alongs*, and the argument checks the union of both (MIRT_ERR_INVALID_ARGUMENT, nothing
 * written; nrays == 0 does nothing).  They are dispatched as the along calls are: mirt_set_query_mode applies, AUTO is their rule,
 * the grid kept per (scene, direction) and the kept groups of directions are the very ones those calls build and use, and
 * mirt_get_along_stats reports the call.  What is not binned sweeps every triangle; mirt_set_ray_grid does not affect these calls.
 * An index of dir_of outside [0, ndirs): the host form refuses the call; the _device form leaves that ray's slots unwritten and writes
 * its count 0. */
MIRT_API int mirt_intersect_ordered_along(const float dir[3], const float *origins3, int nrays, const mirt_hit *after /* nullable */, int max_hits,
                                          mirt_hit *hits /* nrays * max_hits, ray-major */, int32_t *counts /* nrays */);
MIRT_API int mirt_intersect_ordered_along_device(const float dir[3], const void *d_origins3, int nrays, const void *d_after, int max_hits, void *d_hits,
                                                 void *d_counts);
MIRT_API int mirt_intersect_ordered_alongs(const float *dirs3, int ndirs, const int32_t *dir_of /* nullable */, const float *origins3, int nrays,
                                           const mirt_hit *after /* nullable */, int max_hits, mirt_hit *hits, int32_t *counts);
MIRT_API int mirt_intersect_ordered_alongs_device(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, const void *d_after,
                                                  int max_hits, void *d_hits, void *d_counts);

/* The same for rays that share their origin -- an eye, a probe, a point light: transparency layers and depth peeling under a
 * perspective camera, a pick that reports everything under the cursor, the thickness of a part seen from a sensor, a point light's
 * translucent shadow map, a bounce ray from a surface point that skips the surface it starts on.  The four calls are
 * mirt_intersect_ordered on the rays {origin, dirs[i]} or {origins[origin_of[i]], dirs[i]}, byte for byte: max_hits, `after`, the
 * slots, the counts and the overlap rule (after == hits only with max_hits == 1) are that call's, the origins, directions and
 * origin_of those of mirt_intersect_from* / mirt_intersect_fans* (origins on the host in the _device forms too), and the argument
 * checks the union of both (MIRT_ERR_INVALID_ARGUMENT, nothing written; nrays == 0 does nothing).  So slot 0 without `after` is
 * mirt_intersect_from / mirt_intersect_fans on a fresh record, all 20 bytes.  They are dispatched as the fan calls are:
 * mirt_set_query_mode applies, AUTO is their rule, the cubes kept around the origins are the very ones those calls (and
 * mirt_occluded_fans*) build and use, and mirt_get_fan_stats reports the call.  What is not binned sweeps every triangle;
 * mirt_set_ray_grid does not affect these calls.  A call of more origins than one cube holds runs in passes; the in-place peel is
 * safe across them.  An index of origin_of outside [0, norigins): the host form refuses the call; the _device form leaves that
 * ray's slots unwritten and writes its count 0. */
MIRT_API int mirt_intersect_ordered_from(const float origin[3], const float *dirs3, int nrays, const mirt_hit *after /* nullable */, int max_hits,
                                         mirt_hit *hits /* nrays * max_hits, ray-major */, int32_t *counts /* nrays */);
MIRT_API int mirt_intersect_ordered_from_device(const float origin[3], const void *d_dirs3, int nrays, const void *d_after, int max_hits, void *d_hits,
                                                void *d_counts);
MIRT_API int mirt_intersect_ordered_fans(const float *origins3, int norigins, const int32_t *origin_of /* nullable for one origin */, const float *dirs3,
                                         int nrays, const mirt_hit *after /* nullable */, int max_hits, mirt_hit *hits, int32_t *counts);
MIRT_API int mirt_intersect_ordered_fans_device(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays,
                                                const void *d_after, int max_hits, void *d_hits, void *d_counts);

/* ---- the number of hits along a ray (additions to ABI 4) ---- */

/* How many triangles a ray crosses: a point-in-mesh test by the parity of the crossings, the occupancy of a voxel line, the number of
 * surfaces an X-ray or CT beam passes, the layers of a part -- every hit of a ray in ONE call, where mirt_intersect_ordered* holds at
 * most MIRT_MAX_ORDERED_HITS and has to be called again behind its last record.  A count needs no list and no order: counts[i] is the
 * number of triangles j such that
 *   - the reference's test accepts j for ray i (raytracer.cpp:239),
 *   - FLT_MAX >= d_j -- what a fresh record takes, so never a NaN or +inf distance; d_j is the reference's own distance (:241-242),
 *     with `dir` used as given --,
 *   - when `after` is given, d_j > a || (d_j == a && j < k) for a = after[i].distance, k = after[i].index: float and signed-int
 *     comparisons as written (a NaN a admits nothing, a negative a everything, -0.0f behaves as 0.0f); only distance and index of
 *     an `after` record are read,
 *   - when `max_distance` is given, d_j < max_distance[i], strictly: a NaN, 0 or negative limit gives the count 0, +inf is no limit.
 * So without `after` and limit the count is the number of records repeated mirt_intersect_ordered calls enumerate; with the same
 * `after` and no limit min(counts[i], max_hits) is mirt_intersect_ordered's count; and without `after`, counts[i] > 0 is the byte
 * of mirt_occluded for the same limit.  Every counts[i] for i in [0, nrays) is written and nothing beyond; nrays == 0 does nothing.
 * MIRT_ERR_INVALID_ARGUMENT for a negative count, NULL rays or counts with a positive one, and an `after` array that overlaps
 * `counts` (nothing is written); `max_distance` must not overlap `counts` either.  mirt_count_hits: host arrays, complete on return.
 * mirt_count_hits_device: device arrays, queued like mirt_intersect_device (the streams of mirt_set_frames_in_flight in turn, no
 * host sync; mirt_sync() completes it).
 * Unlike the closest hit, the any-hit byte and the first hits, a count is NOT indifferent to a triangle that a structure offers
 * twice.  mirt_count_hits* therefore sweeps every triangle whatever mirt_set_ray_grid says: the cell grid offers a triangle from
 * several cells along a ray and from its plane index as well.  It touches neither mirt_get_ray_grid_stats nor any other statistics,
 * and mirt_set_query_mode does not affect it. */
MIRT_API int mirt_count_hits(const mirt_ray *rays, int nrays, const mirt_hit *after /* nullable */, const float *max_distance /* nullable */,
                             int32_t *counts /* nrays */);
MIRT_API int mirt_count_hits_device(const void *d_rays, int nrays, const void *d_after, const void *d_max_distance, void *d_counts);

/* The same along parallel rays: the four calls are mirt_count_hits on the rays {origins[i], dir} or {origins[i], dirs[dir_of[i]]},
 * count for count.  `after`, the limits and the counts are that call's, the directions, origins and dir_of those of
 * mirt_occluded_along* / mirt_occluded_alongs*, and the argument checks the union of both (MIRT_ERR_INVALID_ARGUMENT, nothing written,
 * with or without a device; nrays == 0 does nothing).  They are dispatched as those calls are: mirt_set_query_mode applies, AUTO is
 * their rule (it has not been examined for counts), the grid kept per (scene, direction) and the kept groups of directions are the
 * very ones the along calls build and use -- a ray walks its cell's list and the every-ray list, and a triangle stands on one of the
 * two, once: every triangle is offered at most once, so the count is exact -- and mirt_get_along_stats reports the call.  What is
 * not binned sweeps every triangle, and so does mirt_count_hits_along* down a direction every triangle is edge-on to (a grid that
 * holds nothing but its every-ray list: mode_used says BRUTE).  An index of dir_of outside [0, ndirs): the host form refuses the call and writes nothing; the
 * _device form writes that ray's count 0.
 * There is no form for rays from shared origins yet: that a cube bin's list names a triangle only once has not been shown. */
MIRT_API int mirt_count_hits_along(const float dir[3], const float *origins3, int nrays, const mirt_hit *after /* nullable */,
                                   const float *max_distance /* nullable */, int32_t *counts /* nrays */);
MIRT_API int mirt_count_hits_along_device(const float dir[3], const void *d_origins3, int nrays, const void *d_after, const void *d_max_distance,
                                          void *d_counts);
MIRT_API int mirt_count_hits_alongs(const float *dirs3, int ndirs, const int32_t *dir_of /* nullable */, const float *origins3, int nrays,
                                    const mirt_hit *after /* nullable */, const float *max_distance /* nullable */, int32_t *counts);
MIRT_API int mirt_count_hits_alongs_device(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, const void *d_after,
                                           const void *d_max_distance, void *d_counts);

/* ---- shadow masks: DirectLight's shadow decision per (record, light position), and DirectLight from a mask (additions to ABI 4) ---- */

/* The one value DirectLight computes and throws away (raytracer.cpp:306-315): whether the shadow ray of a record towards a light
 * position found an occluder nearer than 0.99 r.  mirt_shadow_mask* returns it, one bit per (record, position);
 * mirt_direct_light_masked* is DirectLight with the ray replaced by that bit.  Together they are mirt_direct_light* in every bit, and
 * apart they are a relight without shadow rays when a light changes colour or intensity or the last light is deleted, a shadow mask
 * without shading, the visibility of N points from K positions at one bit a pair, and per-light shadow buffers for compositing.
 * Positions are mirt_direct_light's: npos = nlights x samples under the current mirt_set_soft_shadows state, position
 * j = light * samples + sample, with its limits (MIRT_MAX_LIGHTS lights, MIRT_MAX_LIGHT_POSITIONS positions).
 * Layout: MIRT_MASK_WORDS(npos) planes of nhits words, plane-major -- word w of record i at mask[(size_t)w * nhits + i], position j
 * in bit j & 31 of word j >> 5. */
#define MIRT_MASK_WORDS(npositions) (((npositions) + 31) / 32)
/* Bit j of record i is 1 exactly when DirectLight(hits[i]) executes `D = vec3(0)` (:314) for position j: the decision
 * mirt_direct_light* itself makes for that record and position, by the same kernels' arithmetic (the rays the cube's bins do not cover
 * and the per-ray exact-only override included).  Only the record's POSITION is read, not its index: a list of bare points, any
 * index, gets its bits -- unlike mirt_direct_light, which casts no ray for an index outside [0, n).
 * Exactly MIRT_MASK_WORDS(npos) x nhits words are written, bits at or beyond npos as 0, and nothing beyond them; with npos == 0
 * nothing is written.  mirt_set_query_mode applies with mirt_direct_light's rules unchanged (AUTO: the same rule over records x
 * positions x triangles, or the cubes held; a call the frame path would not bin sweeps; one range of positions that fits no cube
 * sends the whole call to the sweep), and the passes, the kept cubes and the borrowed frame-path cube are mirt_direct_light's own:
 * a cube either call built serves the other.  No scratch travels between the passes: a record's bits belong to its own lane.
 * Checks, in mirt_direct_light's order: MIRT_ERR_NOT_INITIALISED; MIRT_ERR_INVALID_ARGUMENT for a negative count, a NULL array with
 * a positive count (the mask: when there are records and positions) or the lights' limits; nhits == 0 does nothing;
 * MIRT_ERR_NO_SCENE.  mirt_shadow_mask: host arrays, complete on return.  mirt_shadow_mask_device: device arrays, queued like
 * mirt_direct_light_device (the streams in turn; mirt_sync() completes it).  Neither form touches mirt_get_stats,
 * mirt_get_query_stats, mirt_get_fan_stats or mirt_get_occlusion_stats. */
MIRT_API int mirt_shadow_mask(const mirt_hit *hits, int nhits, const mirt_light *lights, int nlights, uint32_t *mask);
MIRT_API int mirt_shadow_mask_device(const void *d_hits, int nhits, const mirt_light *lights, int nlights, void *d_mask);
/* out_rgb[3*i ..] = DirectLight(hits[i]) with, per position, D = bit ? (0, 0, 0) : the light's term (:294-304) in the place of the
 * shadow ray; everything else is DirectLight's: result += D (:319), result2 += result where the position closes a light (:322), the
 * multiply by the triangle's colour (:325-326), the reference's NaN bits, and (0, 0, 0) for an index outside [0, n).  A pure
 * function of records, lights, soft-shadow state and mask: it builds no cube, casts no ray, keeps no statistics and ignores
 * mirt_set_query_mode.  With the mask mirt_shadow_mask* returned for the same records, lights and state it equals
 * mirt_direct_light* in every bit -- whatever the lights' colours and intensities are now: the bits depend on positions only.  A
 * prefix of the lights under the same `samples` reads a prefix of the planes (the plane stride stays nhits), so the mask of three
 * lights serves after the last was deleted.  With npos == 0 the mask is not read and the result is mirt_direct_light's without
 * lights.  Checks and queuing as above. */
MIRT_API int mirt_direct_light_masked(const mirt_hit *hits, int nhits, const mirt_light *lights, int nlights,
                                      const uint32_t *mask, float *out_rgb);
MIRT_API int mirt_direct_light_masked_device(const void *d_hits, int nhits, const mirt_light *lights, int nlights,
                                             const void *d_mask, void *d_rgb);
/* The last mirt_shadow_mask* call, in mirt_query_stats' fields with DirectLight's meanings; cube_source is folded over the passes as
 * for mirt_direct_light.  With mirt_set_profiling(1) the counters are filled for a binned call AND for a sweep: shadow_rays =
 * records x positions (every record casts its rays), candidates = rows offered (the sweep: all n per ray), tests = rows tested
 * before the ray's first occluder, fallback_records as for mirt_direct_light (0 for a sweep).  Waits for the stream of that call. */
MIRT_API int mirt_get_shadow_mask_stats(mirt_query_stats *out);

/* Which triangles a binned frame casts no shadow ray from: out[t] = 1 when ONE other triangle hides the whole of triangle t from
 * light position `position` (lights x soft-shadow samples, in the frames' order), so that DirectLight's term for that position is
 * (0, 0, 0) at every hit point on t -- the frames conclude so without a ray (MIRT_TR_SHADOWED=0 in the environment makes them cast
 * it all the same; the frames are bit for bit the same either way).  The table belongs to the light cube the binned frames share
 * once the lights have stood still for a few frames; n must be the scene's triangle count.  MIRT_ERR_INVALID_ARGUMENT when no such
 * cube is held (no binned frame yet, the scene or a light has just changed), for a position it does not hold or another n.  Waits
 * for everything in flight. */
MIRT_API int mirt_get_shadowed(int position, uint8_t *out, int n);

/* ---- rasteriser: replaces Update()'s clear + Draw() + CalculateDOF() of rasteriser.cpp:183-192,461-529 */

/* One frame into host buffers.  Every word of out_xrgb is written: the whole surface is cleared to black
 * (rasteriser.cpp:190) and interior pixels then receive the resolved colour (:491-519).  out_rgb (nullable)
 * = pixelColours, out_zinv (nullable) = depthBuffer (1/z, 0 where nothing was drawn, :52,188), out_index
 * (nullable) = index of the triangle that owns each pixel or -1. */
MIRT_API int mirt_rasterise(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                            uint32_t *out_xrgb, int pitch_bytes, float *out_rgb, float *out_zinv,
                            int32_t *out_index);

/* Rows [y0, y1) into DEVICE buffers, queued on the library stream (see mirt_raytrace_device). */
MIRT_API int mirt_rasterise_device(const mirt_view *view, const mirt_light *lights, int nlights,
                                   const float *indirect, int y0, int y1, int row_origin,
                                   void *d_xrgb, int pitch_bytes, void *d_rgb, void *d_zinv, void *d_index);

/* ---- several GPUs of one node: frames shard by row bands ----------------------------------------- */

/* One process per GPU, as under torch.distributed / MPI; the reference itself is a single process (its only parallelism is
 * OpenMP over rows, raytracer.cpp:557): these calls are what a sharded host loop adds around Draw().  Every rank uploads the
 * same scene (the triangle list is replicated) and makes the same calls in the same order.
 *
 * mirt_band_of          rows [y0, y1) of `rank` when `height` rows are split into `world` contiguous bands (sizes differ by at
 *                       most one row).  Pure arithmetic, no device needed.
 * mirt_comm_create_id   rank 0: creates the 128-byte id of a new group (ncclGetUniqueId); the caller hands it to the other
 *                       ranks by its own means (MPI_Bcast, torch.distributed.broadcast_object_list, a file).
 * mirt_comm_init        every rank, after mirt_init: joins the group (collective).  Transport: RCCL point-to-point over xGMI,
 *                       loaded at run time; MIRT_COMM=shm selects a host-staged loopback for ranks that share one GPU (tests).
 * mirt_*_sharded        renders THIS rank's band of `nviews` consecutive frames (views[0..nviews) share a frame size) and
 *                       gathers the XRGB bands on rank `root` -- the one exchange step of the path: each peer sends its rows
 *                       straight to the root on its own link (a direct gather, not a ring), grouped into one collective per
 *                       call, so frames that render in microseconds can travel many to a gather.  d_frames (device memory,
 *                       required on the root only): nviews frames of height * pitch_bytes, pitch_bytes == 4 * width; frame i
 *                       of the call is byte-identical to a single-GPU mirt_*_device frame (border words of received bands,
 *                       which the ray tracer never writes, arrive as 0).  Asynchronous: the gather runs on a communication
 *                       stream and overlaps the next call's render (two band buffers per rank); mirt_sync() waits for both.
 *                       Without mirt_comm_init (or world == 1) the calls simply render whole frames.  Needs
 *                       mirt_set_frames_in_flight(1). */
#define MIRT_COMM_ID_BYTES 128
MIRT_API int mirt_band_of(int rank, int world, int height, int *y0, int *y1);
/* The messages of one gather (what mirt_*_sharded sends): piece i moves bytes[i] from band_offset[i] of rank peer[i]'s band
 * buffer (nviews bands of its rows, 4 * width bytes per row) to root_offset[i] of the root's frame buffer.  Returns the number
 * of pieces (writes at most max_pieces; arrays nullable).  Pure arithmetic, no device needed. */
MIRT_API int mirt_band_plan(int world, int root, int width, int height, int nviews, uint64_t *root_offset, uint64_t *band_offset,
                            uint64_t *bytes, int32_t *peer, int max_pieces);
/* The partition of a sharded frame among the ranks (every rank must set the same; default 0).  The setting belongs to the library's
 * context: mirt_shutdown() puts it back to 0, so set it after mirt_init().  Nothing exchanges or verifies it: ranks with different strip
 * heights build different gather plans and the grouped send / receive then mismatches (RCCL waits instead of failing) -- the weighted
 * partition has no per-rank parameter to disagree about and is what bench.py uses for binned frames.
 *
 *   strip_rows == 0   contiguous bands (mirt_band_of): one binning pass and one launch chain per rank and frame -- the right
 *                     choice for the binned ray tracer, whose per-frame cost has a part that does not shrink with the rows;
 *   strip_rows  > 0   interleaved strips of that many rows (a multiple of 8), strip s to rank s % world: every rank samples the
 *                     whole height of the frame, which evens out scenes whose cost is concentrated in some rows -- what the
 *                     reference's `#pragma omp parallel for schedule(auto)` over rows does (raytracer.cpp:557, rasteriser.cpp:467),
 *                     at the granularity a GPU launch needs (64).  Each strip is a launch chain of its own.
 * mirt_partition_segments / mirt_partition_plan: a rank's row segments [y0[k], y1[k]) and the gather's messages for either
 * partition (mirt_band_of / mirt_band_plan are the strip_rows == 0 case); a band buffer holds a rank's segments of one view back
 * to back.  Pure arithmetic, no device needed; both return the count (arrays nullable, at most max_* entries written).
 *   MIRT_PARTITION_WEIGHTED   contiguous bands of equal ESTIMATED COST instead of equal height: the counterpart of
 *                     `schedule(auto)` for a frame whose rows differ in what they cost (a triangle soup seen in perspective: the
 *                     middle bands of BASELINE configs[4] hold twice the candidates of the outer ones).  The first kernel of
 *                     a binned ray-traced frame leaves an estimate of the (tile, triangle) pairs per tile row of the WHOLE frame,
 *                     whatever rows it renders.  A ray-traced sharded call whose whole frame would be binned (its mode, the scene,
 *                     the frame size and the settings decide: the same on every rank) files view 0's estimate on every rank --
 *                     from the pass of the rank's own band, or from a histogram-only pass where that band is rendered brute
 *                     force, keeps the pass of an earlier call or is empty; no other pass of the call files one, and frames
 *                     outside sharded calls never do.  The bands of sharded call c come from the newest estimate filed by a
 *                     call before c - 1, by integer arithmetic -- identical on every rank, nothing exchanged.  Equal bands
 *                     until a histogram exists (the first two calls, calls that file none).
 * mirt_weighted_bounds: that arithmetic as a pure function (world + 1 boundaries, multiples of 8 rows, from a histogram of
 * hist_rows coarse tile rows of (1 << hist_shift) tile rows each); mirt_partition_bounds: the boundaries the NEXT sharded call
 * will use; mirt_bounds_plan: the gather's messages for explicit boundaries (bounds[0] == 0 <= ... <= bounds[world] == height);
 * mirt_set_cost_histogram(1) makes binned frames leave the histogram outside sharded calls too (into a copy of its own that the
 * partition never reads) and mirt_cost_histogram returns the newest one, whichever stream filed it (returns its row count,
 * 0: none). */
#define MIRT_PARTITION_WEIGHTED (-1)
MIRT_API int mirt_set_partition(int strip_rows);
MIRT_API int mirt_set_cost_histogram(int on);
MIRT_API int mirt_cost_histogram(uint32_t *hist, int max_rows, int *rows, int *shift);
MIRT_API int mirt_weighted_bounds(const uint32_t *hist, int hist_rows, int hist_shift, int width, int height, int world, int32_t *bounds);
MIRT_API int mirt_partition_bounds(int world, int width, int height, int32_t *bounds);
MIRT_API int mirt_bounds_plan(int world, int root, int width, int height, int nviews, const int32_t *bounds, uint64_t *root_offset,
                              uint64_t *band_offset, uint64_t *bytes, int32_t *peer, int max_pieces);
MIRT_API int mirt_partition_segments(int rank, int world, int height, int strip_rows, int32_t *y0, int32_t *y1, int max_segments);
MIRT_API int mirt_partition_plan(int world, int root, int width, int height, int nviews, int strip_rows, uint64_t *root_offset,
                                 uint64_t *band_offset, uint64_t *bytes, int32_t *peer, int max_pieces);
MIRT_API int mirt_comm_create_id(void *id128);
MIRT_API int mirt_comm_init(const void *id128, int rank, int world);
MIRT_API int mirt_comm_shutdown(void);
/* Link check after mirt_comm_init: `bytes` of a pattern travel from this rank to itself through the group's transport (one send
 * and one receive in a group, exactly as in a gather) and are compared.  Any world size; synchronous. */
MIRT_API int mirt_comm_selfcheck(size_t bytes);
MIRT_API int mirt_raytrace_sharded(const mirt_view *views, int nviews, const mirt_light *lights, int nlights, const float *indirect,
                                   int mode, int root, void *d_frames, int pitch_bytes);
MIRT_API int mirt_rasterise_sharded(const mirt_view *views, int nviews, const mirt_light *lights, int nlights, const float *indirect,
                                    int root, void *d_frames, int pitch_bytes);

/* Counters / timings of the most recent render call. */
MIRT_API int mirt_get_stats(mirt_stats *out);
/* With profiling on and two or more frames in flight: the per-kernel GPU times (kernel_ms8[8], indexed like mirt_stats.kernel_ms) and the
 * GPU time of the call BEFORE the last one -- the frame on the other stream, whose kernels ran while the frames on both sides of
 * it were running, which is the state a render loop is in.  (mirt_get_stats reports the last call, whose tail runs alone.)
 * Waits for all streams. */
MIRT_API int mirt_get_previous_kernel_ms(float *kernel_ms8, float *gpu_ms);

#ifdef __cplusplus
}
#endif
#endif /* MIRT_H */
