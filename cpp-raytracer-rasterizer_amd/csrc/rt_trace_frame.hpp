// rt_trace_frame.hpp -- the parameter block of the binned ray-trace kernel (k_rt_trace2, rt_trace.hip) and the tile-pair record its
// waves pick up, declared ONCE for the kernel and for the host code that fills them (capi/binned.cpp).
#pragma once

#include "rt_binned.hpp"

#include <cstddef>

namespace mirt {

// A tile pair as the trace kernel's waves pick it up: the first tile's place in the frame (column | row << 16, in tiles: the wave
// divides nothing; capi/binned.cpp refuses a frame of more than 65535 tiles either way), where its list starts (the second tile's follows it), and the two lengths.
struct TilePairRec { uint32_t txy, beg, nA, nB; };
constexpr int ORDER_CLASSES = 8;                 // classes of max(nA, nB) / ORDER_CLASS_STEP, the last one open-ended
constexpr int ORDER_GROUPS = 8;                  // one list per XCD group (workgroup id % 8)
constexpr uint32_t ORDER_CLASS_STEP = 16;        // = TR_STAGE: a class is a number of staging chunks
constexpr int TR_WG_WAVES = 1;                   // a workgroup of the trace kernel is ONE wave.  A name for 1, not a knob: the kernel's wave -> pair
                                                 // map and its LDS slice are written for it (static_assert there and beside the launch)

// What is uniform per launch and decides which of the kernel's once-per-wave blocks a frame needs at all: made on the host
// (trace_frame_flags) into one word that arrives with the prologue's batch, instead of being found out by every wave from
// pointers and counts loaded one behind the other.
enum : uint32_t {
    TRF_PLANES = 1u,                             // some optional output plane (rgb, index, fd, dist, pos) is asked for; without it a wave stores XRGB only
    TRF_ONE_SAMPLE = 2u,                         // one sample per light: every light position closes a light's sum (no soft shadows)
    TRF_LAZY_GEO = 4u,                           // geometry rows are fetched by the exact stage, for the pairs it accepts, instead of being staged
                                                 // with every candidate (scenes whose tables no longer fit the caches: see the staging code)
    TRF_LIST_END = 8u,                           // a tile's list ends at the shell of the tile's farthest record (the primary loop); MIRT_TR_LIST_END
    TRF_SHADOWED = 16u,                          // the shared cube's table of covered triangles stands behind light_pair_count (below); MIRT_TR_SHADOWED
};

// The shared cube's covered words (csrc/shadowed.hpp, k_shadowed_table): bit k of word t says that one other triangle hides the whole
// of triangle t from light position k.  The table travels in the block the shared cube hands the kernel as light_pair_count: the
// cube's lists never overflow, so the count is a word that is always zero -- word 0 of that block -- and the n words of the table
// start SHADOWED_HEAD words behind it (a cache line of their own).  The parameter block keeps its size and every field its offset:
// both are pinned as literal numbers below and in tests/cpp/trace_flags_test.cpp, and the block's four 4-byte paddings are not
// contiguous, so a pointer of its own would move the fields behind it.  Whoever lifts that pin should give the table its own field.
constexpr uint32_t SHADOWED_HEAD = 16;

inline uint32_t trace_frame_flags(const RtFrame &f, bool lazy_geo, bool list_end, bool shadowed = false)
{
    uint32_t flags = 0u;
    if (f.rgb || f.index || f.fd || f.dist || f.pos) flags |= TRF_PLANES;
    if (f.samples == 1) flags |= TRF_ONE_SAMPLE;
    if (lazy_geo) flags |= TRF_LAZY_GEO;
    if (list_end) flags |= TRF_LIST_END;
    if (shadowed) flags |= TRF_SHADOWED;
    return flags;
}

struct RtTraceFrame {
    RtFrame f;
    const uint32_t *cam_off;          // camera bins (8x8-pixel tiles): first entry of each key, nbins * cam_shells + 1
    const uint32_t *cam_entries;      // triangle ids ordered by camera key
    const GeoRow *geo;                // n geometry rows (k_geo_table)
    const ShadeRow *shade;            // n shading rows (k_geo_table)
    const uint32_t *light_off;        // light-cube keys of all light positions: first row of each, nlights*6*B*B*light_shells + 1
    const LightRow *light_rows;       // expanded candidates ordered by light-cube key (k_expand_light_rows)
    const uint32_t *light_tri;        // the triangle of each of them
    const BinFrameDesc *light_frames; // 6 per light position: the depth-shell parameters (the faces of a light share them)
    int tiles_x;                      // camera bins per row
    int cube_bins;                    // B: light-cube bins per face side
    int cam_shells;                   // depth shells per camera bin: bin b's list is cam_off[b * cam_shells] .. cam_off[(b + 1) * cam_shells]
    int light_shells;                 // depth shells per light-cube bin
    float shell_d0, shell_iw;         // the camera frame's shell parameters (BinFrameDesc): what the tiles' lists were sorted with
    uint32_t flags;                   // TRF_* (trace_frame_flags)
    const uint32_t *pair_count;       // pairs this frame's binning produced / room in the pair list: beyond it the lists are
    uint32_t pair_cap;                // incomplete and every tile takes the whole triangle list instead (brute force)
    const TilePairRec *order;         // the frame's tile pairs by XCD group and list-length class (k_tile_order): ORDER_GROUPS x ORDER_CLASSES
                                      // segments of order_seg records
    const uint32_t *order_count;      // records in each segment
    uint32_t order_seg;               // room per segment = the most pairs a group can have = waves per group
    const uint32_t *sel;              // the triangles k_prep_select found the frame may see, and how many: what a frame that fell
    const uint32_t *sel_count;        // back to brute force walks (their origin rows are the ones the frame has built)
    const uint32_t *light_pair_count; // the same for the light-cube lists when a pass of their own built them (the shared, cached cube never
    uint32_t light_pair_cap;          // overflows: a word that reads zero and a cap of 2^32 - 1): beyond it the shadow rays walk the lights' origin tables.
                                      // TRF_SHADOWED: the word is the head of the shared cube's covered table (SHADOWED_HEAD above)
};

// Host and device passes must agree on the block's layout, byte for byte: the numbers are spelled out, so that either pass fails to
// compile when it would lay the block out differently (tests/cpp/trace_flags_test.cpp checks the same from outside).
constexpr size_t RT_TRACE_FRAME_TAIL_BYTES = 168;          // what RtTraceFrame adds behind its RtFrame
#define MIRT_TRF_AT(field, at) (offsetof(RtTraceFrame, field) == sizeof(RtFrame) + (at))
static_assert(sizeof(TilePairRec) == 16, "a record is one 16-byte scalar load");
static_assert(sizeof(RtFrame) % 8 == 0 && offsetof(RtTraceFrame, f) == 0 && MIRT_TRF_AT(cam_off, 0) && MIRT_TRF_AT(light_frames, 56) &&
              MIRT_TRF_AT(tiles_x, 64) && MIRT_TRF_AT(shell_iw, 84) && MIRT_TRF_AT(flags, 88) && MIRT_TRF_AT(pair_count, 96) &&
              MIRT_TRF_AT(pair_cap, 104) && MIRT_TRF_AT(order, 112) && MIRT_TRF_AT(order_seg, 128) && MIRT_TRF_AT(sel, 136) &&
              MIRT_TRF_AT(light_pair_count, 152) && MIRT_TRF_AT(light_pair_cap, 160) &&
              sizeof(RtTraceFrame) == sizeof(RtFrame) + RT_TRACE_FRAME_TAIL_BYTES,
              "RtTraceFrame's layout changed: the kernel and capi/binned.cpp share it");

}  // namespace mirt
