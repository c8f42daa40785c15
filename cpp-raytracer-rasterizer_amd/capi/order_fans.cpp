// order_fans.cpp -- every hit along rays from shared origins, in order (mirt_intersect_ordered_from*, mirt_intersect_ordered_fans*; the
// kernels: ../order/ordered_fans.hip).  By definition the calls are mirt_intersect_ordered on the rays {origin, dirs[i]} or
// {origins[origin_of[i]], dirs[i]}.  The decision and the structures are the fan calls' own (query.cpp: fan_begin, fans_binned,
// fans_passes): mirt_set_query_mode applies, AUTO is their rule, the cubes kept around the origins are the same objects -- a cube
// mirt_intersect_from, mirt_intersect_fans or mirt_occluded_fans built serves the ordered call and the other way round, and so do
// the frame path's and DirectLight's for their positions -- and the statistics are QUERY_FAN's (mirt_get_fan_stats).  What does not
// bin -- BRUTE, a small AUTO call, an origin the frame path would not bin -- writes the rays out (k_query_fans_expand, with one
// origin and no index for the single fan) and runs order.cpp's sweep on them (order_launch); the arbitrary-ray grid is not consulted
// from here.  max_hits of 3, 5, 6 or 7 run the next list length up.
//
// Passes and the in-place peel.  A call of more origins than a cube holds runs in passes over ALL rays; every ray belongs to exactly
// one pass, the lane of that pass reads the ray's `after` record before it writes the ray's slot, and a lane that is not the pass's
// writes nothing.  Binned or brute is decided once, in front of the first pass, and no path runs the call again after a pass has
// written (a pass fails only with an error, which ends the call): so `after == hits` with max_hits == 1 needs no copy set aside here,
// unlike order_along.cpp's calls of several directions.
#include "capi.hpp"

namespace mirt {

// The union of the ordered call's checks and the fan call's: the arguments first, then the library's state.
static int check_order_from_args(const float *origin, const void *dirs3, int nrays, const void *after, int max_hits, const void *hits, const void *counts)
{
    int rc;
    if ((rc = order_args(dirs3, nrays, after, max_hits, hits, counts))) return rc;
    if ((rc = from_args(origin, dirs3, nrays, hits))) return rc;
    return need_init();
}
static int check_order_fans_args(const float *origins3, int norigins, const void *origin_of, const void *dirs3, int nrays, const void *after, int max_hits,
                                 const void *hits, const void *counts, bool host)
{
    int rc;
    if ((rc = order_args(dirs3, nrays, after, max_hits, hits, counts))) return rc;
    if ((rc = fans_args(origins3, norigins, origin_of, dirs3, nrays, hits))) return rc;
    if (host && (rc = fans_index_args(norigins, static_cast<const int32_t *>(origin_of), nrays))) return rc;
    return need_init();
}

int order_from(const float *origin, const void *d_dirs3, int nrays, const OrderOut &out)
{
    int rc;
    if ((rc = check_order_from_args(origin, d_dirs3, nrays, out.after, out.max_hits, out.hits, out.counts))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    FanOrderFrame f;
    memset(&f, 0, sizeof f);
    bool binned = false;
    if ((rc = fan_begin(origin, d_dirs3, nrays, nullptr, &f.f, &binned))) return rc;
    if (!binned) {
        if ((rc = fans_expand(origin, 1, nullptr, d_dirs3, nrays))) return rc;
        return order_launch(g.cur().query.d_fan_rays, nrays, out, nullptr, 0);
    }
    f.out = out;
    return order_walk_launch(MIRT_ORDER_WALK_KERNEL(k_fan_order, out.max_hits, f.f.stats), nrays, f);
}

// Several origins: mirt_intersect_fans*' decision, plan, cubes and passes, each pass one launch of k_fans_order over all rays.  The
// sweep of a call that does not bin carries the indices along (OrderFrame::dir_of / ndirs), so that a ray whose index names no origin
// keeps its slots and gets the count 0, as in the binned kernel.
static int order_fans_run(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays, const OrderOut &out)
{
    int rc;
    std::vector<FanPass> plan;
    const std::initializer_list<CubeChoice> foreign = { { &g.lc, 3 }, { &g.qrows.cubes[0], 4 } };
    const bool binned = fans_binned(origins3, norigins, nrays, foreign, &plan);

    stream_begin();
    QueryStats &stats = stats_begin(QUERY_FAN, binned);
    if (!binned) {
        if ((rc = fans_expand(origins3, norigins, d_origin_of, d_dirs3, nrays))) return rc;
        return order_launch(g.cur().query.d_fan_rays, nrays, out, d_origin_of, d_origin_of ? norigins : 0);
    }

    FansOrderFrame f;
    memset(&f, 0, sizeof f);
    f.f.f = fan_frame(d_dirs3, nrays, nullptr);
    f.f.origin_of = static_cast<const int32_t *>(d_origin_of);
    f.norigins = norigins;
    f.out = out;
    if ((rc = stats_arm(QUERY_FAN, &f.f.f.stats))) return rc;        // (once: the passes' kernels add up in the same words)
    const auto kernel = MIRT_ORDER_WALK_KERNEL(k_fans_order, out.max_hits, f.f.f.stats);
    // (plan[0].first == 0: the pass that writes the strays' count)
    return fans_passes_run(origins3, plan, foreign, stats, f.f, [&] { return order_walk_launch(kernel, nrays, f); });
}

int order_fans(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays, const OrderOut &out)
{
    int rc;
    if ((rc = check_order_fans_args(origins3, norigins, d_origin_of, d_dirs3, nrays, out.after, out.max_hits, out.hits, out.counts, false))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    return order_fans_run(origins3, norigins, d_origin_of, d_dirs3, nrays, out);
}

// ---- host buffers: the directions and the indices travel through the fan calls' staging arrays, `after`, the records and the counts
// through the ordered call's own (order_with_host_arrays) ----

int order_from_host(const float *origin, const float *dirs3, int nrays, const mirt_hit *after, int max_hits, mirt_hit *hits, int32_t *counts)
{
    const int checked = check_order_from_args(origin, dirs3, nrays, after, max_hits, hits, counts);
    const HostArray in[] = { { (void *)dirs3, &QueryRows::d_dirs, (size_t)nrays * 3 * sizeof(float), true, false } };
    return order_with_host_arrays(checked, nrays, after, max_hits, hits, counts, in,
                                  [&](const OrderOut &out) { return order_from(origin, g.qrows.d_dirs, nrays, out); });
}

int order_fans_host(const float *origins3, int norigins, const int32_t *origin_of, const float *dirs3, int nrays, const mirt_hit *after, int max_hits,
                    mirt_hit *hits, int32_t *counts)
{
    const int checked = check_order_fans_args(origins3, norigins, origin_of, dirs3, nrays, after, max_hits, hits, counts, true);
    const HostArray in[] = { { (void *)dirs3, &QueryRows::d_dirs, (size_t)nrays * 3 * sizeof(float), true, false },
                             { (void *)origin_of, &QueryRows::d_origin_of, (size_t)nrays * sizeof(int32_t), origin_of != nullptr, false } };
    return order_with_host_arrays(checked, nrays, after, max_hits, hits, counts, in, [&](const OrderOut &out) {
        return order_fans(origins3, norigins, origin_of ? g.qrows.d_origin_of : nullptr, g.qrows.d_dirs, nrays, out);
    });
}

}  // namespace mirt

extern "C" int mirt_intersect_ordered_from(const float origin[3], const float *dirs3, int nrays, const mirt_hit *after, int max_hits, mirt_hit *hits, int32_t *counts)
{
    return mirt::order_from_host(origin, dirs3, nrays, after, max_hits, hits, counts);
}
extern "C" int mirt_intersect_ordered_from_device(const float origin[3], const void *d_dirs3, int nrays, const void *d_after, int max_hits, void *d_hits, void *d_counts)
{
    return mirt::order_from(origin, d_dirs3, nrays, mirt::order_out(d_after, max_hits, d_hits, d_counts));
}
extern "C" int mirt_intersect_ordered_fans(const float *origins3, int norigins, const int32_t *origin_of, const float *dirs3, int nrays, const mirt_hit *after,
                                           int max_hits, mirt_hit *hits, int32_t *counts)
{
    return mirt::order_fans_host(origins3, norigins, origin_of, dirs3, nrays, after, max_hits, hits, counts);
}
extern "C" int mirt_intersect_ordered_fans_device(const float *origins3, int norigins, const void *d_origin_of, const void *d_dirs3, int nrays, const void *d_after,
                                                  int max_hits, void *d_hits, void *d_counts)
{
    return mirt::order_fans(origins3, norigins, d_origin_of, d_dirs3, nrays, mirt::order_out(d_after, max_hits, d_hits, d_counts));
}
