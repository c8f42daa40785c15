// many_lights.hpp -- parameter block and declarations of the kernels of a DEFERRED ray-traced frame (many_lights.hip): a frame with
// more light positions than the fused frame kernels carry (RtFrame: MIRT_MAX_LIGHTS) renders its primary rays with no light at
// all, turns the intersection planes into hit records, runs DirectLight over them in passes (../query/light_passes.hpp) and
// resolves pixelColours from the result (../capi/rt_frame.cpp: rt_enqueue).
#pragma once

#include "../query/rt_query.hpp"

namespace mirt {

// Rows [y0, y1) of a frame W wide: pixel (x, y) is record (y - y0) * W + x.  The planes are the frame kernels' (RtFrame: index,
// dist, pos), addressed by full-frame pixel numbers y * W + x.
struct ManyLightsFrame {
    int W, H, y0, y1, row_origin;
    const int32_t *index;       // closest triangle, -1 on a miss
    const float *dist;          // closestIntersections[].distance
    const float *pos;           // 3 floats per pixel
    uint32_t *records;          // pixels x HIT_WORDS (k_frame_records writes, DirectLight reads)
    const float *direct;        // pixels x 3: DirectLight of every record (k_frame_resolve reads)
    const float *tris15;
    int n;
    float indirect[3];
    uint32_t *xrgb;             // as RtFrame's: row y at (y - row_origin) * pitch_words, interior pixels only
    int pitch_words;
    float *rgb;                 // nullable, full-frame pixel numbers
};

__attribute__((global)) void k_frame_records(const ManyLightsFrame);
__attribute__((global)) void k_frame_resolve(const ManyLightsFrame);

}  // namespace mirt
