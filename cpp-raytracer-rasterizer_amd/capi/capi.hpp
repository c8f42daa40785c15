// capi.hpp -- the host side of the C-ABI (csrc/mirt_capi.hip and the files of this directory): the library's state, one
// StreamState per frame in flight inside one Ctx, and the helpers the topic files share.  Host code only: the frame kernels are
// defined under csrc/, the ray-query kernels under query/, the scene kernels under scene/ and the kernels of a deferred frame under lights/
// (tools/check_spills.py compiles all four); the ones launched from here are declared below, in query/rt_query.hpp, in lights/many_lights.hpp
// and in lights/aa_many_lights.hpp.
#pragma once

#include "../csrc/bin_sort.hpp"
#include "../csrc/comm.hpp"
#include "../csrc/cull.hpp"
#include "../csrc/dof.hpp"
#include "../csrc/rt_common.hpp"
#include "../csrc/raster_common.hpp"
#include "../csrc/rt_binned.hpp"
#include "../csrc/rt_trace_frame.hpp"
#include "../csrc/scan.hpp"
#include "../query/rt_query.hpp"
#include "../along/along.hpp"
#include "../along/alongs.hpp"
#include "../grid/ray_grid.hpp"
#include "../order/ordered_hits.hpp"
#include "../order/ordered_along.hpp"
#include "../order/ordered_fans.hpp"
#include "../count/count_hits.hpp"
#include "../lights/many_lights.hpp"
#include "../lights/aa_many_lights.hpp"
#include "cube_plan.hpp"
#include "pass_plan.hpp"
#include "along_plan.hpp"
#include "object_plan.hpp"
#include "dof_plan.hpp"
#include "aa_plan.hpp"
#include "env.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <functional>
#include <cmath>
#include <vector>

// (a kernel DECLARATION: the definitions live in csrc/ and query/)
#define MIRT_KERNEL __attribute__((global))

namespace mirt {

// ---- kernels (rt_kernels.hip, rt_tile.hip, rt_trace.hip, rt_binned.hip, raster_kernels.hip) ----
MIRT_KERNEL void k_prep_origin(const float *, int, const float *, v3, int, OriginRow *, OriginRow *, uint32_t *, unsigned long long *, uint32_t *);
template <int P> MIRT_KERNEL void k_rt_brute(const RtFrame);
template <int P> MIRT_KERNEL void k_rt_small(const RtFrame, int);
MIRT_KERNEL void k_rt_wave(const RtFrame);
struct RtTileFrame {
    RtFrame f;
    BinFrameDesc cam;
    int tiles_x, tiles_y;
    unsigned long long *clear_hits;
    float4 *tables;
};
MIRT_KERNEL void k_tile_tables(const RtTileFrame);
template <int TW, bool AA> MIRT_KERNEL void k_rt_tile2(const RtTileFrame);
template <int WG> MIRT_KERNEL void k_bin_pairs(const float *, const OriginRow *, const OriginRow *, int, BinSet, BinPairs);
template <bool AA, bool STATS, int WAVES = 4> MIRT_KERNEL void k_rt_trace2(const RtTraceFrame);
MIRT_KERNEL void k_prep_select(const float *, int, const BinFrameDesc, const SelectOut);
MIRT_KERNEL void k_select_faces(const float *, int, const float *, const BinFrameDesc *, OriginRow *, uint32_t *, uint32_t, uint32_t *);
MIRT_KERNEL void k_tile_order(const uint32_t *, int, int, int, int, uint32_t *, uint32_t, TilePairRec *, uint32_t);
MIRT_KERNEL void k_geo_table(const float *, int, GeoRow *, ShadeRow *);
MIRT_KERNEL void k_expand_light_rows(const uint32_t *, const uint32_t *, int, uint32_t, const OriginRow *, int, LightRow *, const uint32_t *, uint32_t, uint32_t *);
MIRT_KERNEL void k_shadowed_table(const float *, int, const float *, const OriginRow *, const uint32_t *, const LightRow *, const BinFrameDesc *, int, int, uint32_t *);
MIRT_KERNEL void k_cull(const float *, int, const CullParams, uint8_t *);
size_t rt_trace_lds_bytes(int waves);
int launch_raster(RasterFrame &f, RasterScratch &s, uint64_t scene_version, hipStream_t stream, hipEvent_t *ev, bool *ev_used);

// ---- errors ----
extern char g_err[512];
int fail(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(MIRT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

enum { EV_CALL0 = 0, EV_CALL1 = 1, EV_K0 = 2, EV_COUNT = 2 + 2 * 8 };
constexpr int MAX_FLIGHT = 4;                    // most frames in flight (mirt_set_frames_in_flight): one HIP stream and one set of scratch each
constexpr int SEL_COUNT0 = 80;                   // word of d_bin_counters where the two selection counters start
constexpr int HIST_SEL_COUNT = 82;               // ... and the two of a histogram-only pass (hist_only_pass), apart from a frame's
constexpr int HIST_RING = 4;                     // pinned copies of the cost histograms sharded calls file (the weighted partition reads them) ...
constexpr int HIST_SLOTS = HIST_RING + 1;        // ... and one behind them for frames outside sharded calls (mirt_cost_histogram only)
constexpr size_t HIT_BYTES = sizeof(unsigned long long) * HIT_SHARDS * HIT_SHARD_STRIDE;   // one hit-counter buffer (rt_common.hpp: count_hits)

// What the ray-trace frames of a stream write besides the caller's planes, by role: one set per stream, so that two frames in
// flight never share any of it.
//
// The origin tables: the brute-force path's camera and light rows (k_prep_origin), a histogram-only pass's camera rows, and the
// camera rows of a binned frame (k_prep_select).
struct OriginTables {
    OriginRow *d_cam_tab = nullptr;              // n rows (cam_tab_n)
    OriginRow *d_light_tab = nullptr;            // light_tab_lights x n rows
    int cam_tab_n = 0, light_tab_n = 0, light_tab_lights = 0;
    float *d_origins = nullptr;                  // (1 + MIRT_MAX_LIGHTS) x 3
    uint32_t *d_flags = nullptr;                 // [0] = unsafe flag

    int ensure_cam_rows();                       // d_cam_tab for the scene's n triangles
    void release();
};

// The (bin, triangle) pair list of a binning pass, its sorted copy and the sort's scratch (bin_pass).
// Sizing the list without a host sync: the count of a frame is copied to pinned memory behind it and looked at by a LATER frame
// of this stream; meanwhile the list is sized from the last count seen, with a device-side fallback if that was too small
// (k_rt_trace2 then takes every triangle for every tile).
struct PairList {
    uint32_t *d_entries = nullptr;               // triangle ids ordered by bin (the sorted pair values)
    uint32_t *d_pair_keys = nullptr, *d_pair_vals = nullptr, *d_sorted_keys = nullptr;   // unsorted pairs, sorted bin ids
    uint32_t *d_tmp_vals = nullptr;              // bucket sort: the pairs partitioned by bucket (keys go to d_sorted_keys)
    uint32_t *d_bucket = nullptr;                // bucket sort: counts | bases (+1) | cursors, cap_buckets each
    uint32_t cap_buckets = 0;
    bool bucket_dirty = false;                   // d_bucket may hold counts of a pass whose sort never ran
    uint32_t cap_entries = 0;
    uint32_t cap_used = 0;                       // capacity the last binning pass told its kernels (== cap_entries outside tests)
    uint32_t *h_count = nullptr;                 // pinned
    hipEvent_t ev_count = nullptr;
    bool count_pending = false;
    bool count_event_due = false;                // bin_pass published a count: record_count() records ev_count behind the frame's last kernel
    bool have_known = false;
    uint32_t known_pairs = 0;

    int ensure(size_t cap);                      // room for `cap` pairs
    void poll();                                 // picks up the count an earlier frame has published, if it has landed
    int record_count();                          // the event of a published count, on g.stream
    void forget_scene() { have_known = false; count_pending = false; }        // the counts belong to the old scene
    void release();
};

// The pass a stream holds: what it binned, so that a frame whose pass would be the same starts at the trace kernel.
struct KeptPass {
    uint64_t bin_key = 0;
    bool bin_key_valid = false;
    int last_bin_mode = -1;                      // what the last pass binned (0: the camera frame / n: n light cubes): a guessed
                                                 // list size only carries over between passes of the same kind
    uint32_t bin_entries = 0;                    // pairs of the current binning

    PassPlan plan_for(uint64_t key, int mode, PairList &P) const;   // picks up P's published count first (binned.cpp)
    void keep(uint64_t key, int mode) { bin_key = key; last_bin_mode = mode; bin_key_valid = true; }
    void forget() { bin_key_valid = false; }                        // the tables it counts on are overwritten
};

// What the two binning passes of a stream have in common: the list, the pass held, the offsets of the sorted list and a block of
// counters the pass's first kernel zeroes.
struct BinPass {
    PairList pairs;
    KeptPass kept;
    uint32_t *d_bin_off = nullptr;
    uint32_t cap_bins = 0;                       // keys + 1 of d_bin_off
    uint32_t *d_bin_counters = nullptr;          // [0] pairs, [16] tile pairs in order, ... (512 bytes / LIGHT_COUNTER_BYTES)
    BinFrameDesc *d_frames = nullptr;            // descriptor buffer

    int ensure_counters(size_t bytes);           // d_bin_counters, zero
    void forget_scene() { kept.forget(); pairs.forget_scene(); }
};

// The camera's binning pass of a binned frame: selection, pairs by tile and shell, offsets, tile order.
struct CameraPass : BinPass {
    // k_prep_select: the triangles the frame may see (indices, sel_n slots) and the two counters its passes use in turn (the pass
    // that counts into one zeroes the other: d_bin_counters[SEL_COUNT0 + parity])
    uint32_t *d_sel = nullptr;
    int sel_n = 0;
    int sel_parity = 0;
    // the frame's tile pairs ordered longest lists first (k_tile_order): ORDER_CLASSES segments of cap_order records
    TilePairRec *d_order = nullptr;
    uint32_t cap_order = 0;

    int ensure_sel();                            // (the stream must be idle when the list grows; the kept pass goes with it)
    SelectOut select_out(const OriginTables &T, int count_word) const;   // rows, list and the counter pair at count_word
    void release();
};

// A LIGHT-cube pass of a stream -- the cubes of lights that move, binned by the frame (transient_light_pass), and the scratch of
// every shared cube's build (light_cache_ensure) -- apart from the camera's, so that either pass is kept while only the other
// one's inputs change.  Its counter block: words 0 .. 127 as in the camera's, 128 .. the face counts; its descriptor buffer:
// [6 * nlights descriptors | (1 + nlights) x 3 origins] of the lights that move.
constexpr size_t LIGHT_COUNTER_BYTES = sizeof(uint32_t) * (128 + 6 * MIRT_MAX_LIGHTS);
struct LightPass : BinPass {
    uint32_t *d_face_counts = nullptr;           // 6 * MIRT_MAX_LIGHTS words (inside d_bin_counters' block)
    // k_select_faces: per face of the light cubes the triangles the face can see -- list i at d_face_sel + i * n
    uint32_t *d_face_sel = nullptr;
    size_t cap_face_sel = 0;                     // slots
    OriginRow *d_light_tab = nullptr;            // light_tab_lights x n origin rows of the lights that move
    int light_tab_n = 0, light_tab_lights = 0;
    LightRow *d_light_rows = nullptr;            // their rows in the order of the pair list
    uint32_t cap_light_rows = 0;

    void release();
};

// The cost histogram of a stream's binned frames (weighted partition): device words, and where they travel for the host to read --
// HIST_RING pinned copies that sharded calls take in turn, and slot HIST_RING for frames outside them; an event behind each
struct CostHist {
    uint32_t *d_hist = nullptr;
    uint32_t *h_hist = nullptr;                  // pinned: HIST_SLOTS x SEL_HIST_MAX words
    hipEvent_t ev_hist[HIST_SLOTS] = {};
    uint64_t hist_key[HIST_SLOTS] = {};          // the sharded call a copy was filed under + 1 (slot HIST_RING: any non-zero); 0 = none
    uint64_t hist_seq[HIST_SLOTS] = {};          // when it was filed (Ctx::hist_seq): the newest copy of all streams is mirt_cost_histogram's
    int hist_rows[HIST_SLOTS] = {}, hist_shift[HIST_SLOTS] = {};
    int hist_next = 0;                           // the ring's next slot

    void forget_scene() { for (uint64_t &k : hist_key) k = 0; }
    void release();
};

// The light-cube bins of the binned ray tracer: they depend on the scene and the light positions only, not on the camera,
// so they are built once per (scene version, light positions, grid) and shared by the frames of every stream.
struct LightCache {
    bool valid = false;
    uint64_t key = 0;                            // scene version + light positions (not the grid)
    int cube_bins = 0;                           // bins per face side of the tables held
    uint64_t track_key = 0;                      // the lights of the most recent binned frame ...
    int stable = 0;                              // ... and for how many frames in a row they have been the same
    OriginRow *d_light_tab = nullptr;            // nl x n origin rows
    size_t cap_tab = 0;
    BinFrameDesc *d_frames = nullptr;            // 6 x nl frame descriptors
    uint32_t *d_off = nullptr;                   // nbins + 1
    uint32_t cap_bins = 0, nbins = 0;
    LightRow *d_rows = nullptr;                  // expanded candidates in key order
    uint32_t *d_row_tri = nullptr;               // the triangle of each row
    uint32_t cap_rows = 0, nrows = 0;
    int shells = 1;                              // depth shells per bin of the tables held
    float *d_origins = nullptr;                  // (1 + MIRT_MAX_LIGHTS) x 3
    uint32_t *d_counter = nullptr;               // pair counter of the build
    // The covered words of the frame path's cube (csrc/shadowed.hpp; light_cache_ensure builds them where asked to): SHADOWED_HEAD
    // words that stay zero -- the trace kernel reads word 0 as the pair count of a cube that never overflows -- then one word per
    // triangle, bit k = "one other triangle hides the whole triangle from position k".  Under the cube's key: built with it, gone with it.
    uint32_t *d_shadowed = nullptr;
    size_t cap_shadowed = 0;                     // triangles it has room for
    bool has_shadowed = false;                   // the tables held carry the words
    int nlights = 0, n = 0;                      // positions and triangles of the tables held

    bool holds(uint64_t k, int bins) const { return valid && key == k && cube_bins == bins; }
    void release();
};

// Depth of field: the planes the render kernels write for a band plus the halo its blur reaches into (render_with_dof).
struct DofPlanes {
    float *rgb = nullptr, *fd = nullptr;         // pixelColours / focalDistances of the band + halo
    uint32_t *xrgb = nullptr;                    // unblurred words the render kernels emit (discarded)
    int32_t *index = nullptr;
    float *zinv = nullptr;
    size_t cap_px = 0;

    int ensure(size_t px);
    void release();
};

// The queries that walk a cube and keep statistics: DirectLight (mirt_get_query_stats), origin fans (mirt_get_fan_stats) and
// occlusion queries (mirt_get_occlusion_stats) and shadow masks (mirt_get_shadow_mask_stats); and the queries along one direction,
// which walk a grid of their own (mirt_get_along_stats).
enum { QUERY_DIRECT_LIGHT = 0, QUERY_FAN = 1, QUERY_OCCLUDED = 2, QUERY_SHADOW_MASK = 3, QUERY_ALONG = 4, QUERY_KINDS = 5 };
// The last query of a kind: how it was answered, the stream it ran on and where its kernel's counters are (device; profiling on,
// binned -- read once, query_get_stats).
struct QueryStats {
    mirt_query_stats s = {};
    hipStream_t stream = nullptr;
    const unsigned long long *dev = nullptr;
};

// What a DirectLight query (query.cpp) writes besides the caller's colours: the origin tables of its light positions, apart from
// the stream's frame tables, so that a query between two frames disturbs nothing a kept binning pass counts on.
struct QueryScratch {
    OriginRow *d_light_tab = nullptr;            // tab_lights x tab_n rows
    int tab_n = 0, tab_lights = 0;
    float *d_origins = nullptr;                  // (1 + MIRT_MAX_LIGHTS) x 3; row 0 (the camera's place) is unused
    uint32_t *d_flags = nullptr;                 // [0] = unsafe flag
    uint64_t rows_seen = 0;                      // the QueryRows::version this stream is already ordered behind (0 = none)
    unsigned long long *d_stats[QUERY_KINDS] = {};   // QSTAT_WORDS counters of the stream's last binned query of each kind (profiling on)
    // mirt_intersect_fans* by brute force: the call's origins and its rays written out for k_query_closest* (k_query_fans_expand)
    float *d_fan_origins = nullptr;              // fan_origins_cap x 3
    float *d_fan_rays = nullptr;                 // fan_rays_cap x RAY_WORDS
    size_t fan_origins_cap = 0, fan_rays_cap = 0;
    // mirt_direct_light* with more than MIRT_MAX_LIGHTS positions: the accumulators between two passes (light_passes.hpp)
    float *d_carry = nullptr;                    // LIGHT_CARRY_WORDS x carry_cap floats
    size_t carry_cap = 0;                        // records
    // mirt_direct_light_masked*: lpos / lcol of the call's positions, MIRT_MAX_LIGHT_POSITIONS x 6 floats (k_query_relight)
    float *d_relight = nullptr;
    // mirt_intersect_ordered_alongs* peeling in place (after == hits): the `after` records set aside before the first pass writes
    uint32_t *d_order_after = nullptr;           // order_after_cap x HIT_WORDS
    size_t order_after_cap = 0;

    void release();
};

// What a deferred frame (more than MIRT_MAX_LIGHTS light positions: rt_frame.cpp, ../lights/many_lights.hip) keeps between its
// kernels, per stream and grow-only, sized for the pixels of the largest call so far: 20 bytes of record, 12 of DirectLight's
// answer and 24 of carry per pixel, and 20 more for the index, distance and position planes where the caller passes none.
struct ManyLightsScratch {
    uint32_t *d_records = nullptr;               // cap_px x HIT_WORDS
    float *d_direct = nullptr;                   // cap_px x 3
    float *d_carry = nullptr;                    // LIGHT_CARRY_WORDS x cap_px
    int32_t *d_index = nullptr;                  // cap_px each: the planes the caller did not ask for
    float *d_dist = nullptr, *d_pos = nullptr;
    size_t cap_px = 0;

    int ensure(size_t px);                       // (the stream must be idle when they grow: ensure waits for it)
    void release();
};

// What a supersampled frame that shades each carried record once (rt_frame.cpp: aa_record_once_frame, ../lights/aa_many_lights.hip)
// keeps between the kernels of a chunk of rows, per stream and grow-only: the chunk's record list with DirectLight's answers and
// carry, sized for the worst case of pixels x aa x aa records (aa_plan.hpp), the pixels' (slot, count) pairs and version counts, the
// list's cursor, and the two statistics of the stream's last such frame (mirt_get_supersample_stats).
struct AaScratch {
    uint32_t *d_records = nullptr;               // cap_rec x HIT_WORDS
    float *d_direct = nullptr;                   // cap_rec x 3
    float *d_carry = nullptr;                    // LIGHT_CARRY_WORDS x cap_rec
    uint32_t *d_slots = nullptr, *d_counts = nullptr;   // cap_rec each
    uint32_t *d_nver = nullptr;                  // cap_px
    uint32_t *d_cursor = nullptr;                // one word
    unsigned long long *d_stats = nullptr;       // [0] hit sub-rays, [1] records shaded
    size_t cap_rec = 0, cap_px = 0;

    int ensure(size_t px, size_t rec);           // (the stream must be idle when they grow: ensure waits for it)
    void release();
};

// The structure of the queries along one direction (along.cpp; ../along/along.hpp): the grid across `dir` over the scene's projected
// bounding box, kept per (scene version, direction) as the fans keep their cube -- shared by the streams, ordered among them by
// events, released in mirt_shutdown, forgotten with the scene through the version it is held under.  The build's pair list and sort
// scratch are its own, so that a build disturbs no stream's kept binning pass.
struct AlongCache {
    bool valid = false;
    uint64_t version = 0;                        // what the structure was built for: the scene version, the triangle count ...
    int n = 0;
    float dir[3] = { 0, 0, 0 };                  // ... and the direction, compared bit for bit
    bool gave_up = false;                        // the every-ray list outgrew its share: calls with this key take the brute-force kernels
    AlongDesc desc = {};
    uint32_t *d_off = nullptr;                   // along_keys + 1
    uint32_t cap_keys = 0;
    QueryRow *d_rows = nullptr;                  // the rows in key order (at least one: a lane with no row left loads row 0)
    AlongAux *d_aux = nullptr;
    uint32_t cap_rows = 0, nrows = 0;
    uint32_t nevery = 0;                         // triangles the build put on the every-ray list (count.cpp: a grid of nothing else)
    float *d_near = nullptr;                     // n depth bounds (k_along_pairs -> k_along_rows)
    int cap_near = 0;
    uint32_t *d_counters = nullptr;              // [0] pairs, [1] triangles on the every-ray list
    uint32_t *d_keys = nullptr, *d_vals = nullptr, *d_tmp_keys = nullptr, *d_tmp_vals = nullptr, *d_entries = nullptr;
    uint32_t cap_pairs = 0;
    uint32_t *d_bucket = nullptr;                // bucket sort: counts | bases (+1) | cursors, cap_buckets each
    uint32_t cap_buckets = 0;

    bool holds(uint64_t v, int count, const float *d) const { return valid && version == v && n == count && memcmp(dir, d, 12) == 0; }
    void release();
};

// A GROUP of directions of the queries along several directions in one call (alongs.cpp; ../along/alongs.hpp, along_plan.hpp): up to
// alongs_slots directions, each with the single grid's descriptor, behind one offset table and one row table.  Kept under the scene
// version, the triangle count, the grid (B, shells) and the pass's directions compared bit for bit and in order; shared by the
// streams under along_ensure's protocol (built on the stream of the call that misses it, the other streams ordered behind the build
// by events); the tables only grow and are released in mirt_shutdown.
struct AlongsGroup {
    bool valid = false;
    uint64_t version = 0;
    int n = 0, B = 0, shells = 0, count = 0;
    float dirs[MIRT_MAX_LIGHTS * 3] = {};        // the pass's directions as the caller gave them
    bool gave_up = false;                        // a direction no grid is built for, or an every-ray list that outgrew its share: calls
                                                 // that hold this pass take the brute-force kernels and build nothing
    AlongDesc *d_descs = nullptr;                // MIRT_MAX_LIGHTS descriptors
    float *d_dirs = nullptr;                     // MIRT_MAX_LIGHTS x 3
    uint32_t *d_off = nullptr;                   // count * along_keys + 1
    uint32_t cap_keys = 0;
    QueryRow *d_rows = nullptr;                  // the rows in key order (at least one: a lane with no row left loads row 0)
    AlongAux *d_aux = nullptr;
    uint32_t cap_rows = 0, nrows = 0;

    bool holds(uint64_t v, int tris, int bins, int nshells, const float *d, int ndirs) const
    {
        return valid && version == v && n == tris && B == bins && shells == nshells && count == ndirs && memcmp(dirs, d, sizeof(float) * 3 * (size_t)ndirs) == 0;
    }
    void release();
};
// The scratch of a group's build: the pair list, the sort's scratch and the depth bounds per (slot, triangle).  One set serves all
// groups: a build waits for the other streams first (along_ensure's protocol), so no two builds overlap.
struct AlongsBuild {
    float *d_near = nullptr;                     // slots x n
    size_t cap_near = 0;
    uint32_t *d_counters = nullptr;              // [0] pairs, [1 + slot] triangles on the slot's every-ray list
    uint32_t *d_keys = nullptr, *d_vals = nullptr, *d_tmp_keys = nullptr, *d_tmp_vals = nullptr, *d_entries = nullptr;
    uint32_t cap_pairs = 0;
    uint32_t *d_bucket = nullptr;                // bucket sort: counts | bases (+1) | cursors, cap_buckets each
    uint32_t cap_buckets = 0;

    void release();
};

// The structure of the arbitrary-ray grid (ray_grid.cpp; ../grid/ray_grid.hpp): cells, plane index and every-ray list behind one
// offset table, kept per scene version as the along grid is -- shared by the streams, ordered among them by events, released in
// mirt_shutdown, forgotten with the scene through the version it is held under.  The build's pair list and sort scratch are its own
// (d_entries, the sort's output, stays: it is the triangle of every row).
struct RayGridCache {
    bool valid = false;
    uint64_t version = 0;                        // what the structure was built for: the scene version and the triangle count
    int n = 0;
    bool gave_up = false;                        // the every-ray list outgrew its share: calls for this scene sweep
    GridDesc desc = {};
    uint32_t *d_off = nullptr;                   // desc.nkeys + 1
    uint32_t cap_keys = 0;
    QueryRow *d_rows = nullptr;                  // the rows in key order (at least one: a lane with no row left loads row 0)
    uint32_t cap_rows = 0, nrows = 0, nplane = 0, nevery = 0;    // rows in all, of the plane index, triangles on the every-ray list
    uint32_t *d_counters = nullptr;              // [0] pairs, [1] triangles on the every-ray list, [2] pairs of the plane index
    uint32_t *d_keys = nullptr, *d_vals = nullptr, *d_tmp_keys = nullptr, *d_tmp_vals = nullptr, *d_entries = nullptr;
    uint32_t cap_pairs = 0;
    uint32_t *d_bucket = nullptr;                // bucket sort: counts | bases (+1) | cursors, cap_buckets each
    uint32_t cap_buckets = 0;
    unsigned long long *d_stats[MAX_FLIGHT] = {};    // GSTAT_WORDS counters of each stream's last walk (profiling on)

    bool holds(uint64_t v, int count) const { return valid && version == v && n == count; }
    void release();
};
// The last call answered under mirt_set_ray_grid(1): how, on which stream, and where its kernel's counters are (read once).
struct RayGridStats {
    mirt_ray_grid_stats s = {};
    hipStream_t stream = nullptr;
    const unsigned long long *dev = nullptr;
};

// The ray-independent rows of ClosestIntersection (k_query_rows): built once per scene version on the stream of the query that
// finds them missing, shared by every stream; a query on another stream waits for ev_built, not for the device.
struct QueryRows {
    QueryRow *d_rows = nullptr;
    int n = 0;                                   // rows allocated
    uint32_t *d_max = nullptr;                   // QMAX_WORDS words: scene-wide maxima
    uint64_t version = 0;                        // scene_version the rows were built for (0 = none)
    hipEvent_t ev_built = nullptr;
    // staging of the host-buffer entry points (mirt_intersect, mirt_direct_light, mirt_occluded)
    void *d_rays = nullptr, *d_hits = nullptr, *d_rgb = nullptr, *d_dirs = nullptr, *d_origin_of = nullptr;
    void *d_limits = nullptr, *d_occluded = nullptr;
    size_t cap = 0;                              // rays / records / directions / origin indices / limits / bytes each holds
    // ... and of mirt_shadow_mask / mirt_direct_light_masked: the mask's planes, grown apart from the rest (up to 32 bytes a record)
    void *d_mask = nullptr;
    size_t mask_cap = 0;                         // words
    // ... and of mirt_intersect_ordered: the `after` records and the counts (one a ray), and the records (max_hits a ray), likewise
    void *d_order_after = nullptr, *d_order_counts = nullptr, *d_order_hits = nullptr;
    size_t order_cap_rays = 0, order_cap_records = 0;
    // The light cube of the DirectLight queries: a LightCache like the frame path's g.lc, keyed alike (scene version + the light
    // positions in use, and the grid -- so a new scene forgets it), kept across calls, shared by the streams and ordered among
    // them by light_cache_ensure's events.  A query whose lights are the ones the frame path's valid cube holds reads g.lc and
    // leaves this one as it is; no query ever writes g.lc or what the frame path tracks in it.
    // A call of more than MIRT_MAX_LIGHTS positions (and the DirectLight passes of a deferred frame) walks one cube per pass: pass p
    // keeps its range's cube in cubes[p % QUERY_LIGHT_CUBES], each keyed and built like entry 0 -- which is the cube of a call of
    // one pass --, so that a repeated call of up to MIRT_MAX_LIGHT_POSITIONS positions in full cubes builds nothing.
    static constexpr int QUERY_LIGHT_CUBES = 8;
    LightCache cubes[QUERY_LIGHT_CUBES];
    // The cube of the origin fans (mirt_intersect_from*): the same structure around the fan's origin, a one-position list -- keyed by
    // scene version and origin (light_key_of), built by light_cache_ensure under the same protocol.  Apart from `cube`, so that a
    // probe does not evict DirectLight's lights nor a DirectLight query the probe's origin.
    LightCache fan;
    // The cubes of the many-origin fans (mirt_intersect_fans*, mirt_occluded_fans*): up to MIRT_MAX_LIGHTS of the call's origins as
    // a cube's positions, keyed by scene version, positions and their order (light_key_of), built by light_cache_ensure under the
    // same protocol.  Pass p of a call keeps its range's cube in fans[p % QUERY_LIGHT_CUBES], as DirectLight's passes do in
    // `cubes`, so that a repeated call of up to QUERY_LIGHT_CUBES passes builds nothing; entry 0 is the cube of a call of one pass.
    // Apart from `fan` and `cubes`: the call evicts neither, and a pass whose positions are the ones g.lc or cubes[0] holds reads
    // that cube instead (query.cpp: walk_cube).
    LightCache fans[QUERY_LIGHT_CUBES];
    // The cube around the camera of a supersampled frame that shades each carried record once (k_aa_primary's binned instantiation):
    // one position, keyed by scene version and camera position, built by light_cache_ensure under the same protocol.  Apart from
    // `fan`, so that a frame does not evict the cube mirt_intersect_from* keeps; a frame whose camera stands still finds it held.
    LightCache aa_cam;
    // The grid of the queries along one direction (mirt_intersect_along*, mirt_occluded_along*): one is kept.
    AlongCache along;
    // The groups of the queries along several directions in one call (mirt_intersect_alongs*, mirt_occluded_alongs*): pass p of a call
    // keeps its group in alongs[p % ALONGS_GROUPS], apart from `along`, so that a repeated call of up to ALONGS_GROUPS passes builds
    // nothing and neither family evicts the other's structure.
    AlongsGroup alongs[ALONGS_GROUPS];
    AlongsBuild alongs_build;
    // The arbitrary-ray grid (mirt_set_ray_grid): one per scene version.
    RayGridCache grid;

    void release();                              // (the cubes' tables too)
};

// Everything a frame in flight owns: its stream and the scratch its kernels write.  A frame reads the scene and writes the
// caller's planes plus its own stream's state, so frames on different streams need no ordering among themselves (call_begin).
struct StreamState {
    hipStream_t stream = nullptr;
    hipEvent_t ev_order = nullptr;               // orders work of another stream after what this one has queued so far
    // the side stream: the light-cube pass of a frame whose camera AND lights moved runs there, beside the camera's pass (two
    // latency-bound chains that share nothing until the trace kernel)
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // profiling events, one set per stream, so that the times of a frame survive the frames that follow it on the other streams
    // (mirt_get_previous_kernel_ms: the frame before the last one overlapped its neighbours on both sides)
    hipEvent_t ev[EV_COUNT] = {};
    bool ev_used[8] = {};
    bool call_timed = false;                     // the stream's last call recorded its start / end events (profiling was on)
    OriginTables tabs;
    CameraPass cam;
    LightPass lt;
    CostHist hist;
    // hit counters (HIT_SHARDS sharded counters each): two used alternately, so that a kernel can clear the one the NEXT frame on
    // this stream will use
    unsigned long long *d_hits[2] = {};
    bool hits_clean[2] = {};                     // buffer is all zero (the tile kernel clears the other one itself)
    int hits_tog = 0;                            // the buffer of the stream's current frame
    float4 *d_tile_tab = nullptr;                // tables of the tile ray tracer (k_tile_tables)
    DofPlanes dof;
    void *d_async = nullptr;                     // the XRGB plane of an asynchronous frame (async_plane)
    RasterScratch raster;
    QueryScratch query;
    ManyLightsScratch many;
    AaScratch aa;
    // cull flags: what this stream's copy of d_culled holds -- the number of the cull call (or upload) it comes from --, and the
    // copies OUT of other streams' copies it has made: the event is re-recorded behind every such copy ...
    uint64_t culled_ver = 0;
    hipEvent_t ev_cull_read = nullptr;
    uint32_t cull_read_src = 0;                  // ... bit c: the stream has copied out of copy c since a cull step into c last waited for it
                                                 // (a stream runs in order: waiting for the latest record covers every earlier read)

    int create();                                // the streams and their events (mirt_init allocates the rest)
    void release();
};

struct Ctx {
    bool init = false;
    bool profiling = false;
    int device = -1;
    int cu_count = 256;                          // multiProcessorCount of the device
    StreamState streams[MAX_FLIGHT];
    hipStream_t stream = nullptr;                // the stream work is queued on now (the current call's, or its side stream)
    int in_flight = 1;                           // frames that may be in flight at once (mirt_set_frames_in_flight)
    uint64_t frame_no = 0;                       // device calls so far
    int si = 0;                                  // index of the stream of the current / most recent call: calls take the streams in turn
    int ev_cur = 0;                              // the stream whose events the most recent call recorded (mirt_get_stats reads them)
    StreamState &cur() { return streams[si]; }

    // scene
    int n = 0;
    float *d_tris = nullptr;
    uint8_t *d_culled = nullptr;                 // isCulled flags: one copy of n per stream, [i * n, (i + 1) * n) for frames on streams[i]
    int culled_latest = 0;                       // which copy the most recent cull call wrote (mirt_scene_get_culled reads it)
    uint64_t cull_calls = 0;
    GeoRow *d_geo = nullptr;                     // n geometry rows (built by mirt_scene_upload)
    ShadeRow *d_shade = nullptr;                 // n shading rows (likewise)
    uint32_t *d_scene_bounds = nullptr;          // the SceneBounds words the scene kernels leave (scene.cpp)
    float *d_scene_stage = nullptr;              // staging of mirt_scene_update's host rows (scene_stage_cap floats)
    size_t scene_stage_cap = 0;
    // posed scenes (scene.cpp): the declared objects, the rest pose they are posed from, and the table of one pose -- on the device
    // and where the host fills it (pinned: it travels stream-ordered in front of the launch).  Keyed by nothing: mirt_scene_set_objects
    // puts them there, an upload forgets them, updates and transforms leave them alone.
    std::vector<mirt_object> objects;
    float *d_rest = nullptr;                     // rest_cap floats, nrest rows in use
    size_t rest_cap = 0;
    int nrest = 0;
    uint32_t *d_pose_table = nullptr, *h_pose_table = nullptr;   // pose_table_cap words each (object_plan.hpp: pose_table_words)
    size_t pose_table_cap = 0;
    float bbox_lo[3] = { 0, 0, 0 }, bbox_hi[3] = { 0, 0, 0 };   // the scene's bounding box (host side, mirt_scene_upload)
    LightCache lc;
    QueryRows qrows;
    int query_mode = MIRT_QUERY_AUTO;            // mirt_set_query_mode
    int ray_grid = 0;                            // mirt_set_ray_grid: mirt_intersect* / mirt_occluded* answer through g.qrows.grid
    RayGridStats grid_stats;                     // the last such call (mirt_get_ray_grid_stats)
    QueryStats qstats[QUERY_KINDS];              // the last DirectLight query, the last origin fan, the last occlusion query, the last shadow mask
    unsigned long long *d_hits = nullptr;        // the hit-counter buffer of the current ray-traced frame (one of its stream's d_hits)
    bool scene_finite = true;                    // all vertex coordinates below MIRT_SAFE_MAG
    uint64_t scene_version = 0;                  // bumped whenever the triangles change
    uint64_t cull_version = 0;                   // bumped whenever the cull flags change (rasteriser sizing only)
    int soft_samples = 1;                        // soft-shadow samples per light (1 = hard shadows)
    int aa = 1;                                  // realSamples of Draw(): AA_SAMPLES when AA_ENABLED, else 1
    int dof_k = 0;                               // DOF_KERNEL_SIZE when DOF_ENABLED, else 0
    float dof_focal = 0.0f;                      // FOCAL_LENGTH
    int soft_npos = 0;
    bool aa_many_lights = false;                 // mirt_set_supersampled_many_lights: supersampled frames of many positions shade each record once
    hipStream_t aa_stats_stream = nullptr;       // the stream of the last such frame and its two counters (AaScratch::d_stats), NULL: none yet
    const unsigned long long *aa_stats_dev = nullptr;
    float soft_pos[MIRT_MAX_LIGHT_POSITIONS * 3] = {};   // jittered light positions, [light*samples + i] (randomPositions[256], raytracer.cpp:84)

    // host surfaces the caller registered (mirt_surface_register): pinned + mapped, so the frame reaches them at link speed
    struct HostSurface { char *host = nullptr; char *dev = nullptr; size_t bytes = 0; } surf[4];

    // staging for the host-buffer entry points: all planes share ONE capacity (cap_px pixels)
    void *d_xrgb = nullptr, *d_rgb = nullptr, *d_index = nullptr, *d_zinv = nullptr, *d_pos = nullptr;
    size_t cap_px = 0;
    size_t async_cap_px = 0;                     // pixels of every stream's asynchronous plane

    // several GPUs: this process's place among the ranks that shard a frame, and its band buffers (two: the gather of one
    // batch overlaps the render of the next)
    Comm *comm = nullptr;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_rendered = nullptr, ev_sent[2] = { nullptr, nullptr };
    char *d_band[2] = { nullptr, nullptr };
    size_t band_bytes[2] = { 0, 0 };
    int band_slot = 0;
    int strip_rows = 0;                          // partition of a sharded frame: 0 = contiguous bands, > 0 = interleaved strips of that many rows,
                                                 // MIRT_PARTITION_WEIGHTED = bands of equal estimated cost (mirt_set_partition)
    bool want_hist = false;                      // binned ray-traced frames leave their cost histogram (mirt_set_cost_histogram, or the weighted partition)
    uint64_t shard_calls = 0;                    // sharded calls so far: what a cost histogram is filed under
    bool hist_call = false;                      // inside a sharded call: the pass being enqueued files the call's histogram (render_sharded)
    uint64_t hist_seq = 0;                       // cost histograms filed so far, on any stream
    bool in_sharded = false;
    bool hist_armed = false;                     // hist_prepare armed the pass that is being enqueued

    // statistics of the last call
    mirt_stats stats = {};
    bool stats_pending = false;
    bool raster_since_sync = false;              // rasteriser frames were queued since the last mirt_sync (overflow check there)
    hipStream_t stats_stream = nullptr;          // the stream the last call ran on
    uint64_t pending_primary = 0;
    int pending_nlights = 0;
    bool pending_is_rt = false;
    bool pending_counted = false;                // the kernel counted its executed tests itself (tile / binned)
    bool pending_empty = false;                  // the last ray-trace call rendered no rows (no counters to read)
    const uint32_t *stats_sel_count = nullptr;   // binned frame that ran a pass: where its selection count is (device)
};

extern Ctx g;

// ---- what every call does (state.cpp, mirt_capi.hip) ----
int need_init();
// Frees *p and allocates `bytes` in its place (nothing for 0); MIRT_ERR_OUT_OF_MEMORY when that fails.
int dev_realloc_bytes(void **p, size_t bytes);
template <typename T> int dev_realloc(T **p, size_t count) { return dev_realloc_bytes(reinterpret_cast<void **>(p), count * sizeof(T)); }
// A buffer outgrown: `count` elements in *p (what it held is gone), noted as *cap = want -- 0 while the buffer is not there.
// sync_first: work queued on g.stream may still read the old buffer, which is freed only once that stream is idle.
template <typename T, typename N> int dev_grow(T **p, N *cap, N want, size_t count, bool sync_first)
{
    if (sync_first) HIP_TRY(hipStreamSynchronize(g.stream));
    *cap = 0;
    const int rc = dev_realloc(p, count);
    if (!rc) *cap = want;
    return rc;
}
// The arguments every frame entry point checks before it touches the device.  need_scene: the call renders right away (the
// depth-of-field and staging layers leave that check to the render call); [y0, y1): the row band it renders (the entry points
// that render the whole frame pass an empty band).
int check_frame_args(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect, const void *xrgb, int pitch_bytes,
                     bool need_scene = false, int y0 = 0, int y1 = 0);
hipError_t sync_all();
int next_si();
void stream_begin();                             // the part of call_begin() that takes the next stream (calls that leave the statistics alone)
void call_begin();
void call_end();
inline void k_begin(int k) { if (g.profiling) { (void)hipEventRecord(g.cur().ev[EV_K0 + 2 * k], g.stream); g.cur().ev_used[k] = true; } }
inline void k_end(int k) { if (g.profiling) (void)hipEventRecord(g.cur().ev[EV_K0 + 2 * k + 1], g.stream); }
// Small parameter blocks for the device, carried in the kernel arguments of a one-workgroup kernel (mirt_capi.hip); the optional
// zero job clears up to two regions in the same launch.
struct ZeroJob { uint32_t *a; int na; uint32_t *b; int nb; };
hipError_t upload_small(void *dst, const void *src, size_t bytes, hipStream_t stream, const ZeroJob *zero = nullptr);
void hist_out(uint32_t *hist, uint32_t *host_copy, hipStream_t stream);       // k_hist_out: a cost histogram to its pinned copy

// ---- ray tracer (rt_frame.cpp, binned.cpp) ----
int rt_enqueue(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect, int mode,
               int y0, int y1, int row_origin, void *d_xrgb, int pitch_bytes, void *d_rgb, void *d_index, void *d_fd = nullptr,
               void *d_dist = nullptr, void *d_pos = nullptr);
BinFrameDesc make_camera_frame(const mirt_view *view, int y0, int y1, int aa);
// What the trace kernel of a binned frame takes from the frame's binning pass (binned_pass -> binned_trace).
struct BinnedPass {
    const uint32_t *cam_off;                     // camera offsets, indexed by the FRAME's tile number
    int tiles_x, cam_shells;
    float shell_d0, shell_iw;                    // the camera frame's depth-shell parameters: what the tiles' lists were sorted with
    uint32_t order_seg;                          // tile-pair records per (XCD group, class) segment of the order
    // the light tables -- this frame's own pass (the stream's LightPass) or the shared cache --, the origin table behind them and
    // the pair count and cap that say whether they are complete
    CubeView cube;
    const OriginRow *light_tab;
    const uint32_t *light_pair_count;
    uint32_t light_pair_cap;
    bool shadowed;                               // light_pair_count is the head of the shared cube's covered words (TRF_SHADOWED)
};
// The view of a cube's tables (pass_plan.hpp: make_cube_view): of a cache, and of a stream's light pass binned on a grid of
// cube_bins with `shells` depth shells (its row table is there once a pass has run).
inline CubeView cube_view(const LightCache &C) { return make_cube_view(C.d_off, C.d_rows, C.nrows != 0, C.d_light_tab, C.d_row_tri, C.d_frames, C.cube_bins, C.shells); }
inline CubeView cube_view(const LightPass &L, int cube_bins, int shells)
{
    return make_cube_view(L.d_bin_off, L.d_light_rows, L.d_light_rows != nullptr, L.d_light_tab, L.pairs.d_entries, L.d_frames, cube_bins, shells);
}
// A light cube's tables in C for `nlights` light positions (origins[3 ..]) on a grid of cube_bins, built on g.stream in S -- a
// stream's light pass, whose kept pass the build evicts -- unless C holds them already; *built says which.
int light_cache_ensure(LightCache &C, LightPass &S, const float *origins, int nlights, int cube_bins, bool *built = nullptr, bool shadowed = false);
uint64_t light_key_of(const float *origins, int nlights);
// Bins per face side of the cubes of `nlights` light positions under the frame path's rules (scene size, MIRT_CUBE_BINS, the
// sort's key space); *fixed_grid: the environment fixed it.  light_keys_fit: one sort pass holds such a cube's keys at all.
int light_cube_bins_for(int nlights, bool *fixed_grid);
int cube_bins_override();                        // MIRT_CUBE_BINS as read once (0: not set)
bool light_keys_fit(int nlights, int cube_bins);
int binned_pass(const mirt_view *view, StreamState &ss, const float *origins, int nlights, int y0, int y1, BinnedPass *bp);
int binned_trace(const RtFrame &f, StreamState &ss, const BinnedPass &bp);
// The checks every call makes on its lights and the soft-shadow state; *light_positions: lights x soft-shadow samples, the
// shadow-ray origins.  fill_light_positions: where each of them is (the light itself, or its jittered sample: randomPositions[k *
// SOFT_SHADOWS_SAMPLES + i], raytracer.cpp:286), its share of the light's power, P = (color * intensity) / samples (:282, :296),
// and its origin row -- lpos / lcol: npos rows; origins: rows 1 .. npos (row 0 is the camera's); any of the three may be NULL.
// lights x samples may reach MIRT_MAX_LIGHT_POSITIONS; what holds more than MIRT_MAX_LIGHTS of them is sized by LightPositions.
inline int soft_samples() { return g.soft_samples > 1 ? g.soft_samples : 1; }
int check_lights(const mirt_light *lights, int nlights, int *light_positions);
// Every light position of a call on the host: position, share of the light's power and origin row (row 0: the camera's place).
struct LightPositions {
    float lpos[MIRT_MAX_LIGHT_POSITIONS][3], lcol[MIRT_MAX_LIGHT_POSITIONS][3];
    float origins[(1 + MIRT_MAX_LIGHT_POSITIONS) * 3];
};
// The position count from which a frame is deferred (MIRT_MANY_LIGHTS_MIN, default MIRT_MAX_LIGHTS + 1: what the fused kernels cannot hold).
int many_lights_min();
// The position count from which a supersampled frame shades each carried record once when mirt_set_supersampled_many_lights is on
// (MIRT_AA_DEFER_MIN, default MIRT_MAX_LIGHTS + 1: every frame the fused kernels can render stays with them).
int aa_defer_min();
void fill_light_positions(const mirt_light *lights, int npos, float (*lpos)[3], float (*lcol)[3], float *origins);
// MIRT_RT_AUTO / MIRT_QUERY_AUTO bin nothing below this many triangles (MIRT_BIN_THRESHOLD; the tile kernel takes up to 64).
int auto_bin_threshold();
// A start point -- a camera, a light position, a fan's origin -- inside the filter's proven range (rt_query.hpp; false for NaN).
inline bool start_in_filter_range(const float *p)
{
    return fabsf(p[0]) < MIRT_QUERY_START_MAX && fabsf(p[1]) < MIRT_QUERY_START_MAX && fabsf(p[2]) < MIRT_QUERY_START_MAX;
}
// LDS of a kernel that sweeps the scene's 48-byte rows (OriginRow, QueryRow) in chunks of RT_CHUNK_ROWS.
inline size_t sweep_lds_bytes() { return (size_t)(g.n < RT_CHUNK_ROWS ? g.n : RT_CHUNK_ROWS) * sizeof(OriginRow); }
// Would rt_enqueue bin the WHOLE frame of this view (mode, scene size, operands in range, frame size)?  The same answer on every rank.
bool rt_bins_whole_frame(const mirt_view *view, const mirt_light *lights, int nlights, int mode);
// The cost histogram of a view's whole frame and nothing else, on the current stream (render_sharded).
int hist_only_pass(const mirt_view *view);

// ---- device-resident scenes (scene.cpp; the kernels: ../scene/scene_kernels.hip) ----
// What every call that changes the triangles does to the host's state last: the streams' kept passes, tables and pair counts and the
// cost histograms are forgotten, the shared light cube is dropped, the cull flags get a new number when they changed, and
// scene_version -- which keys every other cache: the query rows, the query cubes, the rasteriser's frame key -- moves on.
void scene_commit(bool flags_changed);
int scene_upload_device(const void *d_tris15, const void *d_culled, int n);
int scene_update_device(int first, int count, const void *d_tris15);
int scene_update_host(int first, int count, const float *tris15);
int scene_transform(int first, int count, const float *rot9, const float *translate3);
int scene_download(int first, int count, float *tris15);
int scene_set_objects(const mirt_object *objects, int nobjects, const float *rest15, int nrest);
int scene_pose(const int32_t *which, int count, const float *xforms12);
// The declared objects and the rest pose go (with their memory: the pose table's too) -- what an upload and mirt_shutdown do to them.
void scene_forget_objects();
int scene_info(struct mirt_scene_info *out);

// ---- ray queries (query.cpp) ----
int query_intersect(const void *d_rays, int nrays, void *d_hits);
int query_intersect_host(const mirt_ray *rays, int nrays, mirt_hit *hits);
int query_direct_light(const void *d_hits, int nhits, const mirt_light *lights, int nlights, void *d_rgb);
int query_direct_light_host(const mirt_hit *hits, int nhits, const mirt_light *lights, int nlights, float *out_rgb);
// DirectLight for nhits > 0 records over the npos positions of `lights` on the current stream, in as many passes as they need.
// mode: MIRT_QUERY_*; auto_rule: what AUTO's own rule says for this call.  stats: the DirectLight statistics of a query, NULL for
// the passes of a deferred frame, which leave them alone and bracket their cube builds under MIRT_K_BIN; carry / carry_cap: the
// caller's scratch for the accumulators between passes, grown here.
int direct_light_passes(const void *d_hits, int nhits, const mirt_light *lights, int npos, void *d_rgb, int mode, bool auto_rule, bool is_query,
                        float **carry, size_t *carry_cap, void *d_mask = nullptr);
// d_mask: mirt_shadow_mask* -- the same passes with the kernels' MASK instantiations; d_rgb, carry and carry_cap are not used then.
int query_shadow_mask(const void *d_hits, int nhits, const mirt_light *lights, int nlights, void *d_mask);
int query_shadow_mask_host(const mirt_hit *hits, int nhits, const mirt_light *lights, int nlights, uint32_t *mask);
int query_direct_light_masked(const void *d_hits, int nhits, const mirt_light *lights, int nlights, const void *d_mask, void *d_rgb);
int query_direct_light_masked_host(const mirt_hit *hits, int nhits, const mirt_light *lights, int nlights, const uint32_t *mask, float *out_rgb);
bool direct_light_auto_bins(int nhits, int npos);
int query_intersect_from(const float *origin, const void *d_dirs3, int nrays, void *d_hits);
// The cube around `cam` for the `subrays` primary sub-rays of a supersampled frame in frame mode `mode` on the current stream, under
// the single fan's rules (query_intersect_from): *cube is g.qrows.aa_cam, built if need be (the build bracketed as the frame's binning
// step), or NULL when the frame sweeps -- MIRT_RT_BRUTE, a scene the fan rule would not bin, a scene or camera outside the filter's
// proven range, keys the sort cannot hold.  mirt_set_query_mode and the queries' statistics are untouched.
int aa_camera_cube(const float *cam, int mode, long long subrays, const LightCache **cube);
int query_intersect_from_host(const float *origin, const float *dirs3, int nrays, mirt_hit *hits);
int query_intersect_fans(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays, void *d_hits);
int query_intersect_fans_host(const float *origins3, int norigins, const int32_t *origin_of, const float *dirs3, int nrays, mirt_hit *hits);
int query_occluded(const void *d_rays, int nrays, const void *d_max_distance, void *d_occluded);
int query_occluded_host(const mirt_ray *rays, int nrays, const float *max_distance, uint8_t *occluded);
int query_occluded_fans(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays, const void *d_max_distance,
                        void *d_occluded);
int query_occluded_fans_host(const float *origins3, int norigins, const int32_t *origin_of, const float *dirs3, int nrays, const float *max_distance,
                             uint8_t *occluded);

// What along.cpp shares with the queries above (query.cpp): the scene's rows on the current stream, the scene check, the brute-force
// launches, the statistics of a kind, the many-origin fans' AUTO rule, and the host-buffer wrapper.
int query_rows();
int query_need_scene();
QueryFrame rows_frame(const void *d_rays, int nrays, void *d_hits);
int intersect_launch(const void *d_rays, int nrays, void *d_hits);
int occluded_launch(const void *d_rays, int nrays, const void *d_limit, void *d_occluded);
QueryStats &stats_begin(int kind, bool binned);
int stats_arm(int kind, unsigned long long **counters);
int query_get_stats(int kind, mirt_query_stats *out);
bool auto_bins_fans(int nrays);
int query_staging(size_t count);
// One host-buffer entry point around its device form `call`, given the verdict of that form's argument checks and the call's
// `count` of rays or records: nothing to do for none, then the scene, then staging room for `count`; every `in` array goes to its
// staging array (a member of g.qrows) on the stream the call will take, every `out` array comes back on the stream it took, and
// the host waits for that stream.
struct HostArray { void *host; void *QueryRows::*staging; size_t bytes; bool in, out; };
template <int N, class Call>
int with_host_arrays(int checked, int count, const HostArray (&a)[N], Call call)
{
    int rc;
    if (checked) return checked;
    if (count == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    if ((rc = query_staging((size_t)count))) return rc;
    hipStream_t st = g.streams[next_si()].stream;            // the stream the query below will take
    for (const HostArray &x : a)
        if (x.in) HIP_TRY(hipMemcpyAsync(g.qrows.*x.staging, x.host, x.bytes, hipMemcpyHostToDevice, st));
    if ((rc = call())) return rc;
    for (const HostArray &x : a)
        if (x.out) HIP_TRY(hipMemcpyAsync(x.host, g.qrows.*x.staging, x.bytes, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return MIRT_OK;
}

// ---- ray queries along one direction (along.cpp; the kernels: ../along/along.hip) ----
int along_intersect(const float *dir, const void *d_origins3, int nrays, void *d_hits);
int along_intersect_host(const float *dir, const float *origins3, int nrays, mirt_hit *hits);
int along_occluded(const float *dir, const void *d_origins3, int nrays, const void *d_max_distance, void *d_occluded);
int along_occluded_host(const float *dir, const float *origins3, int nrays, const float *max_distance, uint8_t *occluded);
// What alongs.cpp shares with along.cpp: the start of a build under the streams' protocol, and its end.
int along_build_begin();
int along_build_end();
// What the ordered calls along a direction (order_along.cpp) share with it: the argument checks, the decision and structure step of
// a call on the stream it takes (*binned says whether `frame` is ready for a walk kernel; the statistics of QUERY_ALONG begun
// afresh), and the rays written out into the stream's query scratch (g.cur().query.d_fan_rays) for a sweep.
int check_along_args(const float *dir, const void *origins3, int nrays, const void *out);
int along_begin(const float *dir, const void *d_origins3, int nrays, AlongFrame *frame, bool *binned);
int along_expand(const float *dir, const void *d_origins3, int nrays);

// ---- arbitrary rays through the cell grid (ray_grid.cpp; the kernels: ../grid/ray_grid.hip) ----
// With the switch on, on the stream the call has taken: *done says the walk kernel was queued; otherwise the caller sweeps.
int ray_grid_intersect(const void *d_rays, int nrays, void *d_hits, bool *done);
int ray_grid_occluded(const void *d_rays, int nrays, const void *d_max_distance, void *d_occluded, bool *done);
// What order.cpp shares with them: everything of such a call up to its kernel (the structure, the statistics begun afresh; *binned says
// whether `frame` is ready for a walk kernel), and the ray count up to which a sweep takes a wave per ray (query.cpp).
int grid_begin(const void *d_rays, int nrays, GridFrame *frame, bool *binned);
long query_wave_rays();

// ---- every hit along a ray, in order (order.cpp; the kernels: ../order/ordered_hits.hip) ----
// A device form takes what the ordered call adds to its rays -- (d_after, max_hits, d_hits, d_counts) -- as the block its kernels
// take (../order/order_out.hpp), from the entry point to the frame that embeds it.
inline OrderOut order_out(const void *d_after, int max_hits, void *d_hits, void *d_counts)
{
    return { static_cast<const uint32_t *>(d_after), max_hits, static_cast<int32_t *>(d_counts), static_cast<uint32_t *>(d_hits) };
}
int order_intersect(const void *d_rays, int nrays, const OrderOut &out);
int order_intersect_host(const mirt_ray *rays, int nrays, const mirt_hit *after, int max_hits, mirt_hit *hits, int32_t *counts);
// What order_along.cpp and order_fans.cpp share with it: the checks of the arguments alone, the sweep on the current stream (d_dir_of /
// ndirs: OrderFrame::dir_of, NULL for none), the host forms' staging arrays, the kernel of a call and its launch.
int order_args(const void *rays, int nrays, const void *after, int max_hits, const void *hits, const void *counts);
int order_launch(const void *d_rays, int nrays, const OrderOut &out, const void *d_dir_of, int ndirs);
int order_staging(int checked, int nrays, int max_hits);
int order_staging_rays(size_t rays);                  // (its per-ray arrays alone: `after` and the counts, which count.cpp stages through too)
// The kernel of list length K = 1, 2, 4 or 8 out of the four instantiations; max_hits of 3, 5, 6 or 7 run the next length up ...
template <class Kernel>
Kernel order_pick(int max_hits, Kernel k1, Kernel k2, Kernel k4, Kernel k8)
{
    const int K = hit_list_size_for(max_hits);
    return K == 1 ? k1 : (K == 2 ? k2 : (K == 4 ? k4 : k8));
}
// ... and out of the eight of a walk kernel template <int K, bool STATS>.
#define MIRT_ORDER_WALK_KERNEL(kernel, max_hits, stats)                                                                                \
    ((stats) ? mirt::order_pick(max_hits, kernel<1, true>, kernel<2, true>, kernel<4, true>, kernel<8, true>)                           \
             : mirt::order_pick(max_hits, kernel<1, false>, kernel<2, false>, kernel<4, false>, kernel<8, false>))
// A walk kernel, a lane per ray, on the call's stream.
template <class Kernel, class Frame>
int order_walk_launch(Kernel kernel, int nrays, const Frame &f)
{
    hipLaunchKernelGGL(kernel, dim3((unsigned)((nrays + 255) / 256)), dim3(256), 0, g.stream, f);
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}
// One host form around its device form `call(out)`, given the verdict of its checks and its own input rows `in`: room in the ordered
// calls' staging arrays, then with_host_arrays on `in` and the three rows every such call has -- `after` in (it goes to its own
// staging array before anything comes back: the in-place peel needs nothing more on this side), the records and the counts out.
template <int N, class Call>
int order_with_host_arrays(int checked, int nrays, const mirt_hit *after, int max_hits, mirt_hit *hits, int32_t *counts, const HostArray (&in)[N], Call call)
{
    int rc;
    if ((rc = order_staging(checked, nrays, max_hits))) return rc;
    const size_t records = checked ? 0 : (size_t)nrays * (size_t)max_hits;
    HostArray a[N + 3];
    std::copy(in, in + N, a);
    a[N] = { (void *)after, &QueryRows::d_order_after, (size_t)nrays * sizeof(mirt_hit), after != nullptr, false };
    a[N + 1] = { hits, &QueryRows::d_order_hits, records * sizeof(mirt_hit), false, true };
    a[N + 2] = { counts, &QueryRows::d_order_counts, (size_t)nrays * sizeof(int32_t), false, true };
    const QueryRows &Q = g.qrows;
    return with_host_arrays(checked, nrays, a, [&] { return call(order_out(after ? Q.d_order_after : nullptr, max_hits, Q.d_order_hits, Q.d_order_counts)); });
}
// ... along one direction and along several (order_along.cpp; the kernels: ../order/ordered_along.hip)
int order_along(const float *dir, const void *d_origins3, int nrays, const OrderOut &out);
int order_along_host(const float *dir, const float *origins3, int nrays, const mirt_hit *after, int max_hits, mirt_hit *hits, int32_t *counts);
int order_alongs(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, const OrderOut &out);
int order_alongs_host(const float *dirs3, int ndirs, const int32_t *dir_of, const float *origins3, int nrays, const mirt_hit *after, int max_hits,
                      mirt_hit *hits, int32_t *counts);

// ---- ray queries along several directions in one call (alongs.cpp; the kernels: ../along/alongs.hip) ----
int alongs_intersect(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, void *d_hits);
int alongs_intersect_host(const float *dirs3, int ndirs, const int32_t *dir_of, const float *origins3, int nrays, mirt_hit *hits);
int alongs_occluded(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, const void *d_max_distance, void *d_occluded);
int alongs_occluded_host(const float *dirs3, int ndirs, const int32_t *dir_of, const float *origins3, int nrays, const float *max_distance, uint8_t *occluded);
// What order_along.cpp shares with it: the argument checks, and a whole call on the stream it takes -- the plan, the groups, launch(f)
// per pass with `f` carrying the caller's arrays, or the rays written out (g.cur().query.d_fan_rays) and brute().
int check_alongs_args(const float *dirs3, int ndirs, const void *dir_of, const void *origins3, int nrays, const void *out);
int check_alongs_host_args(const float *dirs3, int ndirs, const int32_t *dir_of, const float *origins3, int nrays, const void *out);
int alongs_run(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, AlongsFrame &f,
               const std::function<int(const AlongsFrame &)> &launch, const std::function<int()> &brute);

// ... from one origin and from several (order_fans.cpp; the kernels: ../order/ordered_fans.hip)
int order_from(const float *origin, const void *d_dirs3, int nrays, const OrderOut &out);
int order_from_host(const float *origin, const float *dirs3, int nrays, const mirt_hit *after, int max_hits, mirt_hit *hits, int32_t *counts);
int order_fans(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays, const OrderOut &out);
int order_fans_host(const float *origins3, int norigins, const int32_t *origin_of, const float *dirs3, int nrays, const mirt_hit *after, int max_hits,
                    mirt_hit *hits, int32_t *counts);
// What order_fans.cpp shares with the fan calls (query.cpp): the checks of the arguments alone (what check_from_args, check_fans_args
// and check_fans_host_args test behind the library's state); the frame both fan calls start from; the single fan's
// decision and structure step on the stream it takes (fan_begin: the statistics of QUERY_FAN begun afresh, *binned says whether `frame`
// is ready for a walk kernel); for several origins the decision with its pass plan (fans_binned), the cubes somebody else may hold
// for them (fans_foreign: what mirt_intersect_fans* passes), the passes of a binned call (fans_passes_run: fans_passes with the launch
// as a std::function) and the rays written out into the stream's query scratch (g.cur().query.d_fan_rays) for a sweep.
struct CubeChoice { const LightCache *cube; int source; };
int from_args(const float *origin, const void *dirs3, int nrays, const void *hits);
int fans_args(const float *origins3, int norigins, const void *origin_of, const void *dirs3, int nrays, const void *hits);
int fans_index_args(int norigins, const int32_t *origin_of, int nrays);
QueryFanFrame fan_frame(const void *d_dirs3, int nrays, void *d_hits);
int fan_begin(const float *origin, const void *d_dirs3, int nrays, void *d_hits, QueryFanFrame *frame, bool *binned);
int fans_expand(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays);
bool fans_binned(const float *origins3, int norigins, int nrays, std::initializer_list<CubeChoice> foreign, std::vector<FanPass> *plan);
int fans_passes_run(const float *origins3, const std::vector<FanPass> &plan, std::initializer_list<CubeChoice> foreign, QueryStats &stats,
                    QueryFansFrame &q, const std::function<int()> &launch);

// ---- rasteriser (raster.cpp) ----
int raster_enqueue(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect,
                   int y0, int y1, int row_origin, void *d_xrgb, int pitch_bytes, void *d_rgb, void *d_zinv,
                   void *d_index, void *d_fd = nullptr);
int cull_copy_wait_readers(int dst, hipStream_t st);

// ---- partition and sharded frames (sharded.cpp) ----
// The cost histogram of a binned frame's pass (k_prep_select): hist_prepare points the pass at it when one is wanted,
// hist_publish files it behind the pass.
int hist_prepare(CostHist &S, const BinFrameDesc &cam, SelectOut *so);
int hist_publish(CostHist &S);
const uint32_t *hist_lookup(uint64_t max_key, int *rows, int *shift);
void current_bounds(int world, int W, int H, std::vector<int> &bounds);
unsigned part_tile_weight();
// Copies a gather plan (part_gather_plan) out to the caller's arrays, any of which may be NULL; returns the plan's length.
int plan_out(int world, int root, int width, int height, int nviews, int strip_rows, const int *bounds, uint64_t *root_offset,
             uint64_t *band_offset, uint64_t *bytes, int32_t *peer, int max_pieces);
int render_sharded(const mirt_view *views, int nviews, int root, void *d_frames, int pitch_bytes, bool raster,
                   const mirt_light *lights, int nlights, const float *indirect, int mode);

// ---- delivery: staging, registered surfaces, asynchronous frames, depth of field (delivery.cpp) ----
struct HostPlane { void *host; void **staging; size_t bpp; };
int ensure_staging(size_t px, const HostPlane *planes, int nplanes);
char *registered_alias(const void *host, size_t pitch, int H);
bool host_direct();
int copy_plane_interior(void *dst, int dst_pitch, const void *src, int src_pitch, int W, int H);
int async_plane(size_t px, void **plane);
int async_target(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect, uint32_t *out_xrgb, int pitch_bytes, char **alias);
int dof_resolve(const DofPlanes &D, const mirt_view *view, int y0, int y1, int row_origin, int ry0, int ry1, void *d_xrgb, int pitch_bytes,
                void *user_rgb, void *user_index, void *user_zinv, bool clear_border);

// Depth of field (CalculateDOF with DOF_ENABLED, raytracer.cpp:613-640 / rasteriser.cpp:494-513): the render kernels
// write pixelColours + focalDistances for the band AND the rows its blur taps reach into library-owned planes, then
// k_dof resolves the band into the caller's surface.  `render(ry0, ry1, xrgb, rgb, fd, index, zinv)` runs the path.
template <class Render>
int render_with_dof(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect, int y0, int y1, int row_origin,
                    void *d_xrgb, int pitch_bytes, void *user_rgb, void *user_index, void *user_zinv, bool clear_border, Render render)
{
    int rc;
    // the caller's surface reaches the blur kernel directly: validate it here, before anything is allocated or launched
    // (rt_enqueue / raster_enqueue only see the library-owned planes)
    if ((rc = check_frame_args(view, lights, nlights, indirect, d_xrgb, pitch_bytes, false, y0, y1))) return rc;
    const int W = view->width, H = view->height, K = g.dof_k;
    const int reach = dof_halo_rows(K, W);                   // (a tap column outside the row wraps into the rows beyond: dof_plan.hpp)
    const int ry0 = std::max(0, y0 - reach), ry1 = std::min(H, y1 + reach);
    // the stream call_begin() will give this frame (it is self-contained: its planes are this stream's own)
    DofPlanes &D = g.streams[next_si()].dof;
    if ((rc = D.ensure((size_t)W * (size_t)(ry1 - ry0)))) return rc;
    // the kernels index their planes with full-frame pixel numbers: shift the bases so that row ry0 is the first stored
    const ptrdiff_t shift = (ptrdiff_t)ry0 * W;
    if ((rc = render(ry0, ry1, (void *)D.xrgb, (void *)(D.rgb - 3 * shift), (void *)(D.fd - shift), user_index ? (void *)(D.index - shift) : nullptr,
                     user_zinv ? (void *)(D.zinv - shift) : nullptr))) return rc;
    return dof_resolve(D, view, y0, y1, row_origin, ry0, ry1, d_xrgb, pitch_bytes, user_rgb, user_index, user_zinv, clear_border);
}

// A whole frame into the caller's host buffers and back before the call returns.  writes_every_word: the render fills every word
// of the surface (rasteriser), or only its interior (ray tracer: copy_plane_interior).  planes: the extra outputs as (host
// pointer or NULL, its staging plane, bytes per pixel), in the order the render call takes their device planes;
// `render(xrgb, pitch, device planes)` enqueues the frame.
template <int N, class Render>
int deliver_host(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect, uint32_t *out_xrgb, int pitch_bytes,
                 bool writes_every_word, const HostPlane (&planes)[N], Render render)
{
    int rc;
    if ((rc = check_frame_args(view, lights, nlights, indirect, out_xrgb, pitch_bytes))) return rc;
    const int W = view->width, H = view->height;
    const size_t px = (size_t)W * H;
    if ((rc = ensure_staging(px, planes, N))) return rc;
    char *alias = registered_alias(out_xrgb, (size_t)pitch_bytes, H);
    const bool direct = alias && host_direct();
    void *dev[N];
    for (int i = 0; i < N; i++) dev[i] = planes[i].host ? *planes[i].staging : nullptr;
    if ((rc = render(direct ? (void *)alias : g.d_xrgb, direct ? pitch_bytes : W * 4, dev))) return rc;
    if (!direct) {
        if (writes_every_word) HIP_TRY(hipMemcpy2DAsync(out_xrgb, pitch_bytes, g.d_xrgb, (size_t)W * 4, (size_t)W * 4, H, hipMemcpyDeviceToHost, g.stream));
        else if ((rc = copy_plane_interior(out_xrgb, pitch_bytes, g.d_xrgb, W * 4, W, H))) return rc;
    }
    for (int i = 0; i < N; i++)
        if (planes[i].host) HIP_TRY(hipMemcpyAsync(planes[i].host, dev[i], px * planes[i].bpp, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return MIRT_OK;
}

// ---- asynchronous delivery into a registered host surface ----
// Render into one of the library-owned planes, then ONE stream-ordered DMA copy into the pinned surface; no host sync.  With
// two frames in flight the copy of frame i (the DMA engine) runs while frame i + 1 renders, so a loop that presents one
// surface while the next one is drawn moves frames at the rate of the link alone.  `render(xrgb, pitch)` enqueues the frame.
template <class Render>
int deliver_async(const mirt_view *view, const mirt_light *lights, int nlights, const float *indirect, uint32_t *out_xrgb, int pitch_bytes,
                  bool writes_every_word, Render render)
{
    int rc;
    char *alias = nullptr;
    if ((rc = async_target(view, lights, nlights, indirect, out_xrgb, pitch_bytes, &alias))) return rc;
    const int W = view->width, H = view->height;
    if (host_direct()) return render((void *)alias, pitch_bytes);
    void *plane = nullptr;
    if ((rc = async_plane((size_t)W * H, &plane))) return rc;
    if ((rc = render(plane, W * 4))) return rc;
    // (on the stream the frame was queued on)
    if (!writes_every_word) return copy_plane_interior(out_xrgb, pitch_bytes, plane, W * 4, W, H);
    HIP_TRY(hipMemcpy2DAsync(out_xrgb, pitch_bytes, plane, (size_t)W * 4, (size_t)W * 4, H, hipMemcpyDeviceToHost, g.stream));
    return MIRT_OK;
}

}  // namespace mirt
