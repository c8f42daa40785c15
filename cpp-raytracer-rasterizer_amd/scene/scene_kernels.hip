// scene_kernels.hip -- the scene on the device: rows that arrive from device memory (mirt_scene_upload_device,
// mirt_scene_update*), rows that move in place (mirt_scene_transform), rows posed from the rest pose (mirt_scene_pose), and the
// bounds of what they leave.
//
// Bandwidth kernels: 60 bytes read and 60 + 48 + 32 written per triangle.  A 60-byte row is only 4-byte aligned, so a lane that
// loaded its own row would issue 15 dword loads 60 bytes apart.  Instead a workgroup moves its 256 rows as FLAT dwords through
// LDS: lane l loads dwords l, l + 256, ... of the block's 3840 (every wave instruction covers 256 contiguous bytes), the lanes
// then read their rows out of LDS (stride 15 dwords: odd, so the 32 lanes of a half wave hit 32 banks), and the rows leave the
// same way.  The table entries are stored per lane as whole float4s, as k_geo_table stores them.
//
// GeoRow / ShadeRow carry the expressions of k_geo_table (csrc/rt_trace.hip) on the same operands, so they carry its bits: a
// range ingested here and a scene uploaded from the host cannot be told apart.
#include "scene_kernels.hpp"

namespace mirt {

__global__ __launch_bounds__(8) void k_scene_bounds_init(SceneBounds *b)
{
    const int i = threadIdx.x;
    if (i < 3) b->lo[i] = scene_ord(INFINITY);
    else if (i < 6) b->hi[i - 3] = scene_ord(-INFINITY);
    else if (i == 6) b->not_finite = 0u;
    else b->pad = 0u;
}

template <int MODE>
__global__ __launch_bounds__(SCENE_BLOCK_ROWS) void k_scene_range(const SceneRange a)
{
    constexpr bool INGEST = (MODE & SCENE_INGEST) != 0, XFORM = (MODE & SCENE_XFORM) != 0, BOUNDS = (MODE & SCENE_BOUNDS) != 0;
    constexpr bool POSE = (MODE & SCENE_POSE) != 0;
    static_assert(!POSE || (INGEST && XFORM && !BOUNDS), "a pose ingests moved rows; the bounds are a pass of their own");
    __shared__ float rows[SCENE_BLOCK_ROWS * 15];
    // the range the block is part of, its number within it, where the range's rows come from and how they move: the launch's,
    // or -- POSE -- those of the object the block's work item belongs to (uniform: scalar loads, before anything is stored)
    int first = a.first, count = a.count, block = blockIdx.x;
    const float *src = a.src, *rot = a.rot, *tr = a.tr;
    PoseEntry e;
    if (POSE) {
        const uint32_t *prefix = pose_prefix_of(a.pose, a.pose_count);
        const int k = pose_find(prefix, a.pose_count, blockIdx.x);
        e = a.pose[k];
        first = e.scene_first; count = e.count; block = (int)(blockIdx.x - prefix[k]);
        src = a.src + (size_t)15 * (size_t)e.rest_first; rot = e.rot; tr = e.tr;
    }
    const int r0 = block * SCENE_BLOCK_ROWS;                                 // the block's first row within the range
    const int nrows = min(SCENE_BLOCK_ROWS, count - r0);
    const int nw = nrows * 15;
    float *own = a.tris + (size_t)15 * ((size_t)first + r0);                 // the block's rows of the scene
    const float *in = (INGEST && (!XFORM || POSE)) ? src + (size_t)15 * r0 : own;
    for (int i = threadIdx.x; i < nw; i += SCENE_BLOCK_ROWS) rows[i] = in[i];
    __syncthreads();

    const int r = threadIdx.x;
    float t[15];
    if (r < nrows) {
#pragma unroll
        for (int k = 0; k < 15; k++) t[k] = rows[r * 15 + k];
        if (XFORM) {
            transform_tri(t, rot, V3(tr[0], tr[1], tr[2]));
#pragma unroll
            for (int k = 0; k < 12; k++) rows[r * 15 + k] = t[k];
        }
        if (INGEST) {
            const size_t tri = (size_t)first + r0 + r;
            const v3 v0 = ld3(t), e1 = sub3(ld3(t + 3), v0), e2 = sub3(ld3(t + 6), v0);
            GeoRow g;
            g.g0 = make_float4(v0.x, v0.y, v0.z, e1.x);
            g.g1 = make_float4(e1.y, e1.z, e2.x, e2.y);
            g.g2 = make_float4(e2.z, 0.0f, 0.0f, 0.0f);
            a.geo[tri] = g;
            const v3 nd = normalize3(ld3(t + 9));
            ShadeRow sr;
            sr.n = make_float4(nd.x, nd.y, nd.z, 0.0f);
            sr.col = make_float4(t[12], t[13], t[14], 0.0f);
            a.shade[tri] = sr;
            if (a.culled) {
                const uint8_t c = a.culled_src ? a.culled_src[r0 + r] : (uint8_t)0;
                for (int h = 0; h < SCENE_CULL_COPIES; h++) a.culled[(size_t)h * a.n + tri] = c;
            }
        }
    }

    if (BOUNDS) {
        // the host loops of mirt_scene_upload: finite fails on NaN, colours and normals count; the box is fminf / fmaxf over the nine
        // vertex floats -- a NaN is skipped here, by the lane (fminf returns the other operand), infinities count
        float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
        bool bad = false;
        if (r < nrows) {
#pragma unroll
            for (int k = 0; k < 15; k++) bad |= !(fabsf(t[k]) < 1.0e8f);
#pragma unroll
            for (int k = 0; k < 9; k++) { lo[k % 3] = fminf(lo[k % 3], t[k]); hi[k % 3] = fmaxf(hi[k % 3], t[k]); }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
#pragma unroll
            for (int c = 0; c < 3; c++) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], off)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], off)); }
        const bool any_bad = __ballot(bad) != 0;
        if ((threadIdx.x & 63) == 0) {
            // one atomic per wave and bound at most: a wave that cannot move a bound (it reads a value that is at worst out of
            // date, so never tighter than the truth) leaves it alone
            for (int c = 0; c < 3; c++) {
                const uint32_t ol = scene_ord(lo[c]), oh = scene_ord(hi[c]);
                if (ol < *(volatile uint32_t *)&a.bounds->lo[c]) atomicMin(&a.bounds->lo[c], ol);
                if (oh > *(volatile uint32_t *)&a.bounds->hi[c]) atomicMax(&a.bounds->hi[c], oh);
            }
            if (any_bad) atomicOr(&a.bounds->not_finite, 1u);
        }
    }

    if (INGEST) {
        __syncthreads();
        for (int i = threadIdx.x; i < nw; i += SCENE_BLOCK_ROWS) own[i] = rows[i];
    }
}

template __global__ void k_scene_range<SCENE_INGEST>(const SceneRange);
template __global__ void k_scene_range<SCENE_INGEST | SCENE_XFORM>(const SceneRange);
template __global__ void k_scene_range<SCENE_INGEST | SCENE_BOUNDS>(const SceneRange);
template __global__ void k_scene_range<SCENE_INGEST | SCENE_XFORM | SCENE_BOUNDS>(const SceneRange);
template __global__ void k_scene_range<SCENE_BOUNDS>(const SceneRange);
template __global__ void k_scene_range<SCENE_INGEST | SCENE_XFORM | SCENE_POSE>(const SceneRange);

}  // namespace mirt
