// sharded.cpp -- several GPUs of one node: a frame shards by row bands (or strips, or bands of equal estimated cost), one process
// per GPU, and the bands travel to the root (comm.cpp).  Here: the cost histograms the weighted partition reads, the partition of
// the call about to be issued, and the sharded call itself.
#include "capi.hpp"

namespace mirt {

// The cost histogram of a binned pass (k_prep_select).  Outside sharded calls: wanted when the caller asked for it or the partition
// is the weighted one, filed into a slot of its own that only mirt_cost_histogram reads.  Inside a sharded call: render_sharded
// decides (g.hist_call) -- view 0's histogram, exactly once per call, into the ring the weighted partition reads -- so that what a
// rank files depends on the call and the settings alone, never on its band, on what its stream binned before or on frames it
// rendered outside sharded calls.  hist_prepare points the pass at the device words (zero between passes: k_hist_out leaves them
// so); hist_publish sends them to the pinned copy, tagged with the sharded call they belong to, an event behind them.
static bool hist_wanted() { return g.in_sharded ? g.hist_call : (g.want_hist || g.strip_rows == MIRT_PARTITION_WEIGHTED); }
static int hist_shift_for(int tile_rows) { int sh = 0; while (((tile_rows - 1) >> sh) + 1 > SEL_HIST_MAX) sh++; return sh; }
static int hist_slot(const CostHist &S) { return g.in_sharded ? S.hist_next : HIST_RING; }
int hist_prepare(CostHist &S, const BinFrameDesc &cam, SelectOut *so)
{
    g.hist_armed = false;
    if (!hist_wanted()) return MIRT_OK;
    if (!S.d_hist) {
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&S.d_hist), sizeof(uint32_t) * SEL_HIST_MAX));
        HIP_TRY(hipMemsetAsync(S.d_hist, 0, sizeof(uint32_t) * SEL_HIST_MAX, g.stream));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&S.h_hist), sizeof(uint32_t) * SEL_HIST_MAX * HIST_SLOTS, hipHostMallocDefault));
        for (int i = 0; i < HIST_SLOTS; i++) HIP_TRY(hipEventCreateWithFlags(&S.ev_hist[i], hipEventDisableTiming));
    }
    so->hist = S.d_hist;
    so->hist_shift = hist_shift_for(cam.nbv);
    const int slot = hist_slot(S);
    // (the copy about to be overwritten was filed HIST_RING sharded calls ago, or is the stream's previous one outside them; a
    // reader only ever looks at copies whose event has fired)
    S.hist_key[slot] = 0;
    S.hist_rows[slot] = ((cam.nbv - 1) >> so->hist_shift) + 1;
    S.hist_shift[slot] = so->hist_shift;
    g.hist_armed = true;
    return MIRT_OK;
}
int hist_publish(CostHist &S)
{
    if (!g.hist_armed) return MIRT_OK;
    g.hist_armed = false;
    const int slot = hist_slot(S);
    uint32_t *dst = nullptr;
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&dst), S.h_hist + (size_t)slot * SEL_HIST_MAX, 0));
    hist_out(S.d_hist, dst, g.stream);
    HIP_TRY(hipEventRecord(S.ev_hist[slot], g.stream));
    S.hist_key[slot] = g.shard_calls + 1;        // filed under the sharded call in progress (+1: 0 means "no copy"); outside one, the calls so far
    S.hist_seq[slot] = ++g.hist_seq;
    if (g.in_sharded) {
        S.hist_next = (slot + 1) % HIST_RING;
        g.hist_call = false;
    }
    return MIRT_OK;
}

// max_key > 0: the newest cost histogram a sharded call <= max_key filed (the ring); 0: the newest one filed at all, in or outside
// sharded calls -- on any stream, waiting for its event if it has not fired yet.  NULL when there is none.  (Sharded calls file
// in call order, so the copy filed last is also the one of the latest call.)
const uint32_t *hist_lookup(uint64_t max_key, int *rows, int *shift)
{
    CostHist *B = nullptr;
    int best = -1;
    for (StreamState &ss : g.streams) {
        CostHist &S = ss.hist;
        if (!S.h_hist) continue;
        for (int slot = 0; slot < (max_key ? HIST_RING : HIST_SLOTS); slot++) {
            if (S.hist_key[slot] == 0 || (max_key && S.hist_key[slot] > max_key)) continue;
            if (!B || S.hist_seq[slot] > B->hist_seq[best]) { B = &S; best = slot; }
        }
    }
    if (!B) return nullptr;
    if (hipEventSynchronize(B->ev_hist[best]) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    *rows = B->hist_rows[best]; *shift = B->hist_shift[best];
    return B->h_hist + (size_t)best * SEL_HIST_MAX;
}

// pairs-equivalents a tile costs whatever its list holds (part_weighted_bounds); MIRT_PART_TILE_WEIGHT overrides
unsigned part_tile_weight()
{
    static const unsigned w = [] { const long v = env_int("MIRT_PART_TILE_WEIGHT", -1); return v >= 0 ? (unsigned)v : 12u; }();
    return w;
}

// The bands of the sharded call about to be issued (call number g.shard_calls): equal bands, or -- weighted partition -- bands of
// equal estimated cost from the histogram filed under the call before the previous one (or an earlier one).  Every rank of a group
// issues the same calls with the same views; a ray-traced call whose whole frame would be binned files view 0's histogram on
// every rank (render_sharded), and the bands look TWO calls back, by which time that pass has long run: same histogram on every
// rank (integer sums over the same triangles, whatever rows a rank renders), same integer arithmetic, same bands -- no exchange.
void current_bounds(int world, int W, int H, std::vector<int> &bounds)
{
    bounds.assign((size_t)world + 1, 0);
    int nr = 0, sh = 0;
    const uint32_t *h = (g.strip_rows == MIRT_PARTITION_WEIGHTED && g.shard_calls >= 2) ? hist_lookup(g.shard_calls - 1, &nr, &sh) : nullptr;
    // (a histogram of another frame size cannot be this frame's)
    if (h && nr != ((((H + BIN_TILE - 1) / BIN_TILE) - 1) >> sh) + 1) h = nullptr;
    if (h) part_weighted_bounds(h, nr, sh, W, H, world, part_tile_weight(), bounds.data());
    else for (int r = 0; r < world; r++) { int a, b; band_of(r, world, H, &a, &b); bounds[(size_t)r] = a; bounds[(size_t)r + 1] = b; }
}

int plan_out(int world, int root, int width, int height, int nviews, int strip_rows, const int *bounds, uint64_t *root_offset,
             uint64_t *band_offset, uint64_t *bytes, int32_t *peer, int max_pieces)
{
    std::vector<BandPiece> plan((size_t)std::max(max_pieces, 1));
    const int n = part_gather_plan(world, root, width, height, nviews, strip_rows, plan.data(), max_pieces, bounds);
    for (int i = 0; i < n && i < max_pieces; i++) {
        if (root_offset) root_offset[i] = plan[i].root_offset;
        if (band_offset) band_offset[i] = plan[i].band_offset;
        if (bytes) bytes[i] = plan[i].bytes;
        if (peer) peer[i] = plan[i].peer;
    }
    return n;
}

// The views of one call, each sharded over the ranks of the group (one rank: rendered whole).  raster: the rasteriser, which
// writes every word of a band, or the ray tracer, which leaves the border words alone.
int render_sharded(const mirt_view *views, int nviews, int root, void *d_frames, int pitch_bytes, bool raster,
                   const mirt_light *lights, int nlights, const float *indirect, int mode)
{
    int rc;
    // one band of one frame on g.stream
    auto render = [&](const mirt_view *v, int y0, int y1, int origin, void *dst, int pitch) {
        return raster ? mirt_rasterise_device(v, lights, nlights, indirect, y0, y1, origin, dst, pitch, nullptr, nullptr, nullptr)
                      : mirt_raytrace_device(v, lights, nlights, indirect, mode, y0, y1, origin, dst, pitch, nullptr, nullptr);
    };
    if ((rc = need_init())) return rc;
    if (!views || nviews < 1) return fail(MIRT_ERR_INVALID_ARGUMENT, "need at least one view");
    const int W = views[0].width, H = views[0].height;
    for (int v = 1; v < nviews; v++)
        if (views[v].width != W || views[v].height != H) return fail(MIRT_ERR_INVALID_ARGUMENT, "the views of one call must share a frame size");
    if (W < 1 || H < 1) return fail(MIRT_ERR_INVALID_ARGUMENT, "frame size %dx%d", W, H);
    const int world = g.comm ? comm_world(g.comm) : 1, rank = g.comm ? comm_rank(g.comm) : 0;
    if (root < 0 || root >= world) return fail(MIRT_ERR_INVALID_ARGUMENT, "root %d outside [0,%d)", root, world);
    if (rank == root && !d_frames) return fail(MIRT_ERR_INVALID_ARGUMENT, "the root's frame buffer must not be NULL");
    if (rank == root && (pitch_bytes < W * 4 || (pitch_bytes & 3))) return fail(MIRT_ERR_INVALID_ARGUMENT, "pitch %d bytes too small for width %d or not a multiple of 4", pitch_bytes, W);
    if (world > 1 && rank == root && pitch_bytes != W * 4) return fail(MIRT_ERR_INVALID_ARGUMENT, "a sharded frame needs a dense root buffer (pitch == 4 * width)");
    if (world > 1 && g.in_flight != 1) return fail(MIRT_ERR_INVALID_ARGUMENT, "sharded frames overlap through the band buffers: use mirt_set_frames_in_flight(1)");
    const size_t frame_bytes = (size_t)H * (size_t)pitch_bytes;
    // (a sharded call is what cost histograms are filed under, one per call: current_bounds)
    struct CallScope {
        CallScope() { g.in_sharded = true; g.hist_call = false; }
        ~CallScope() { g.in_sharded = false; g.hist_call = false; g.shard_calls++; }
    } scope;
    // The call's histogram: view 0's whole frame, filed when the call's arguments and the settings say so -- the same on every
    // rank.  The pass of this rank's own rows of view 0 files it when it bins afresh (the histogram does not depend on the rows a
    // pass renders); a band that is rendered brute force, keeps its stream's pass or is empty gets a histogram-only pass right
    // behind view 0 instead (before the later views' passes, which the next call may keep).  No other pass of the call files one.
    g.hist_call = !raster && (g.want_hist || g.strip_rows == MIRT_PARTITION_WEIGHTED) && rt_bins_whole_frame(&views[0], lights, nlights, mode);
    auto view_done = [&](int v) -> int {
        const int r = (v == 0 && g.hist_call) ? hist_only_pass(&views[0]) : MIRT_OK;
        g.hist_call = false;
        return r;
    };
    if (world == 1) {
        for (int v = 0; v < nviews; v++)
            if ((rc = render(&views[v], 0, H, 0, static_cast<char *>(d_frames) + (size_t)v * frame_bytes, pitch_bytes)) || (rc = view_done(v))) return rc;
        return MIRT_OK;
    }
    // this rank's rows: one contiguous band -- an equal share of the rows, or of the estimated cost (weighted partition) --, or
    // interleaved strips (mirt_set_partition); a band buffer holds the segments of one view back to back
    std::vector<int> wb;
    const int *bounds = nullptr;
    const int strips = g.strip_rows > 0 ? g.strip_rows : 0;
    if (g.strip_rows == MIRT_PARTITION_WEIGHTED) { current_bounds(world, W, H, wb); bounds = wb.data(); }
    const int segs = part_segments(rank, world, H, strips, bounds);
    const size_t band_row = (size_t)W * 4, my_bytes = (size_t)part_rows(rank, world, H, strips, bounds) * band_row;
    const int slot = g.band_slot;
    g.band_slot ^= 1;
    if (rank == root) {
        // the root's own rows are rendered in place; the other ranks' rows arrive straight at their places
        for (int v = 0; v < nviews; v++) {
            for (int k = 0; k < segs; k++) {
                int y0, y1;
                part_segment(rank, world, H, strips, k, &y0, &y1, bounds);
                if (y1 > y0 && (rc = render(&views[v], y0, y1, 0, static_cast<char *>(d_frames) + (size_t)v * frame_bytes, pitch_bytes))) return rc;
            }
            if ((rc = view_done(v))) return rc;
        }
    } else {
        const size_t need = my_bytes * (size_t)nviews;
        HIP_TRY(hipStreamWaitEvent(g.stream, g.ev_sent[slot], 0));         // the gather that last read this buffer has finished
        if (need > g.band_bytes[slot]) {
            HIP_TRY(hipStreamSynchronize(g.comm_stream));
            g.band_bytes[slot] = 0;
            if (dev_realloc(&g.d_band[slot], need)) return fail(MIRT_ERR_OUT_OF_MEMORY, "band buffer (%zu bytes)", need);
            g.band_bytes[slot] = need;
        }
        // the border words the ray tracer never writes travel as 0, whatever the buffer held before (a rasterised batch, a
        // batch of another frame size)
        if (!raster && need) HIP_TRY(hipMemsetAsync(g.d_band[slot], 0, need, g.stream));
        for (int v = 0; v < nviews; v++) {
            int before = 0;                                  // rows of this view's earlier segments in the band buffer
            for (int k = 0; k < segs; k++) {
                int y0, y1;
                part_segment(rank, world, H, strips, k, &y0, &y1, bounds);
                // (row y of the segment lands at row before + (y - y0) of this view's part of the buffer)
                if (y1 > y0 && (rc = render(&views[v], y0, y1, y0 - before, g.d_band[slot] + (size_t)v * my_bytes, (int)band_row))) return rc;
                before += y1 - y0;
            }
            if ((rc = view_done(v))) return rc;
        }
    }
    // the one exchange step: every band to the root, on the communication stream, overlapping the next call's render
    HIP_TRY(hipEventRecord(g.ev_rendered, g.stream));
    HIP_TRY(hipStreamWaitEvent(g.comm_stream, g.ev_rendered, 0));
    const int maxp = part_gather_plan(world, root, W, H, nviews, strips, nullptr, 0, bounds);
    std::vector<BandPiece> plan((size_t)std::max(maxp, 1));
    const int np = part_gather_plan(world, root, W, H, nviews, strips, plan.data(), (int)plan.size(), bounds);
    std::vector<GatherPiece> pieces;
    for (int i = 0; i < np; i++) {
        if (plan[i].bytes == 0) continue;
        if (rank == root) pieces.push_back({ static_cast<char *>(d_frames) + plan[i].root_offset, plan[i].bytes, plan[i].peer });
        else if (plan[i].peer == rank) pieces.push_back({ g.d_band[slot] + plan[i].band_offset, plan[i].bytes, root });
    }
    if (!pieces.empty() && !comm_gather_bands(g.comm, root, pieces.data(), (int)pieces.size(), g.comm_stream))
        return fail(MIRT_ERR_HIP, "%s", comm_error(g.comm));
    HIP_TRY(hipEventRecord(g.ev_sent[slot], g.comm_stream));
    return MIRT_OK;
}

}  // namespace mirt
