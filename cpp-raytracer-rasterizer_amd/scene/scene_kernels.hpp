// scene_kernels.hpp -- parameter blocks and declarations of the scene kernels (scene_kernels.hip): triangles that arrive from
// device memory, change in part, move in place or are posed from the rest pose (mirt_scene_upload_device, mirt_scene_update*,
// mirt_scene_transform, mirt_scene_pose), and the bounding box and finiteness flag of the scene they leave, which mirt_scene_upload
// takes on the host.
#pragma once

#include "../csrc/rt_binned.hpp"
#include "../capi/object_plan.hpp"
#include "scene_xform.hpp"

#include <string.h>

namespace mirt {

// The order-preserving unsigned image of a float: a < b as floats <=> scene_ord(a) < scene_ord(b) as unsigned integers (-0 sorts
// below +0), so atomicMin / atomicMax on the images are the minimum / maximum of the floats.  NaNs never get here.
MIRT_HD uint32_t scene_ord(float x)
{
#ifdef __HIP_DEVICE_COMPILE__
    const uint32_t u = __float_as_uint(x);
#else
    uint32_t u; memcpy(&u, &x, 4);
#endif
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
MIRT_HD float scene_unord(uint32_t o)
{
    const uint32_t u = o ^ ((o >> 31) ? 0x80000000u : 0xffffffffu);
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(u);
#else
    float x; memcpy(&x, &u, 4); return x;
#endif
}

// What the bounds pass leaves for the host: the box as images (k_scene_bounds_init: lo = image of +inf, hi = image of -inf -- an
// axis no number was seen on stays there, as fminf / fmaxf leave it on the host) and whether any of the 15 n floats failed
// fabsf(x) < 1e8f.
struct SceneBounds { uint32_t lo[3], hi[3], not_finite, pad; };
constexpr int SCENE_BOUNDS_WORDS = sizeof(SceneBounds) / 4;

constexpr int SCENE_BLOCK_ROWS = 256;             // triangles per workgroup, one per lane: 15 360 bytes of LDS
constexpr int SCENE_CULL_COPIES = 4;              // copies of the cull flags the scene keeps (capi.hpp: MAX_FLIGHT)
static_assert(SCENE_BLOCK_ROWS == POSE_CHUNK_ROWS, "a work item of a pose is one workgroup's rows");

// One pass over rows [first, first + count) of the scene (tris / geo / shade point at triangle 0) -- under POSE: over the rows of
// the objects in `pose`, first and count unused.
struct SceneRange {
    const float *src;           // INGEST without XFORM: count rows that replace the range (row 0 = triangle `first`); POSE: the rest
                                // pose (row 0 = rest row 0); else unused
    float *tris;
    GeoRow *geo;
    ShadeRow *shade;
    int first, count;
    int n;                      // triangles of the scene (stride of the cull copies)
    uint8_t *culled;            // nullable: SCENE_CULL_COPIES x n flags to set for the range, from ...
    const uint8_t *culled_src;  // ... count bytes (row 0 = triangle `first`), or zero when NULL
    float rot[9], tr[3];        // XFORM
    SceneBounds *bounds;        // BOUNDS
    const PoseEntry *pose;      // POSE: the call's table (object_plan.hpp: pose_count entries, then the prefix of their work items)
    int pose_count;
};

// MODE bits.  INGEST: the rows are written to the scene with their GeoRow / ShadeRow entries (and cull flags); XFORM: they are the
// scene's own, moved by (rot, tr), instead of src's; BOUNDS: they are folded into *bounds (meant for first = 0, count = n: a box
// can shrink, so it is never merged).  BOUNDS alone reads the scene and writes nothing else.  POSE (with INGEST and XFORM, without
// BOUNDS): workgroup b is work item b of the table -- it finds its object there, takes that object's rows of the rest pose, its
// transform and its place in the scene, and is one block of an INGEST | XFORM pass over that object otherwise; the grid is the
// table's last prefix entry.
enum { SCENE_INGEST = 1, SCENE_XFORM = 2, SCENE_BOUNDS = 4, SCENE_POSE = 8 };
template <int MODE> __attribute__((global)) void k_scene_range(const SceneRange);
__attribute__((global)) void k_scene_bounds_init(SceneBounds *);

}  // namespace mirt
