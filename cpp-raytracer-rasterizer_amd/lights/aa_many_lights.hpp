// aa_many_lights.hpp -- parameter block and declarations of the kernels of a SUPERSAMPLED frame that shades each carried record
// once (aa_many_lights.hip; aa_versions.hpp has the argument): a frame with supersampling on and more light positions than the
// fused frame kernels carry -- or, under MIRT_AA_DEFER_MIN, any supersampled frame -- runs, per chunk of rows, k_aa_primary (all
// aa x aa sub-rays of a pixel in one lane: the final planes, one hit record per version appended to a compact list, the pixel's
// (slot, count) pairs), DirectLight over the list in passes (../query/light_passes.hpp) and k_aa_resolve (../capi/rt_frame.cpp).
#pragma once

#include "../query/rt_query.hpp"
#include "aa_versions.hpp"

namespace mirt {

// Rows [y0, y1) of a frame W wide -- one chunk: pixel (x, y) is chunk pixel i = (y - y0) * W + x.  The planes are the frame
// kernels' (RtFrame: index, fd, dist, pos), addressed by full-frame pixel numbers y * W + x, every one of them nullable.
// Version k of chunk pixel i has its slot and its count at [k * pixels + i] of `slots` / `counts` (the lanes of a wave write
// neighbouring words); `records` and `direct` are indexed by slot, up to pixels * aa * aa of them.
struct AaFrame {
    const float *tris15;
    int n;
    const OriginRow *tab;       // the camera's origin table: k_prep_origin's (sweep), or the cube's own (binned: directions no bin takes)
    const uint32_t *unsafe;     // sweep: != 0 runs every test through the exact path
    CubeView cube;              // binned: the cube around the camera, one position
    float cam[3];
    float rot[9];
    float focal;
    int W, H, aa;
    int y0, y1, row_origin;
    int32_t *index;
    float *fd;
    float focal_plane;
    float *dist;
    float *pos;
    unsigned long long *hit_count;      // the frame's HIT_SHARDS counters (csrc/rt_common.hpp: count_hits): hit sub-rays
    uint32_t *records;          // pixels * aa * aa x HIT_WORDS, filled with 0xFF before k_aa_primary (index -1)
    uint32_t *cursor;           // records appended so far, zero before k_aa_primary
    uint32_t *slots, *counts;   // aa * aa planes of `pixels` words
    uint32_t *nver;             // pixels: versions of each pixel
    const float *direct;        // DirectLight of every record, by slot (k_aa_resolve reads)
    float indirect[3];
    uint32_t *xrgb;             // as RtFrame's: row y at (y - row_origin) * pitch_words, interior pixels only
    int pitch_words;
    float *rgb;                 // nullable, full-frame pixel numbers
    unsigned long long *stats;  // [0] hit sub-rays, [1] records appended, summed over the frame's chunks
};

template <bool BINNED> __attribute__((global)) void k_aa_primary(const AaFrame);
__attribute__((global)) void k_aa_resolve(const AaFrame);

}  // namespace mirt
