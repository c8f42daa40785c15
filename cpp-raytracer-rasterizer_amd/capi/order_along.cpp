// order_along.cpp -- every hit along parallel rays, in order (mirt_intersect_ordered_along*, mirt_intersect_ordered_alongs*; the
// kernels: ../order/ordered_along.hip).  By definition the calls are mirt_intersect_ordered on the rays {origins[i], dir} or
// {origins[i], dirs[dir_of[i]]}.  The decision and the structure are the along families' own (along.cpp: along_begin, alongs.cpp:
// alongs_run): mirt_set_query_mode applies, AUTO is their rule, the grid of (scene version, direction) and the kept groups are the
// same objects -- a grid mirt_intersect_along built serves the ordered call and the other way round -- and the statistics are
// QUERY_ALONG's (mirt_get_along_stats).  What does not bin -- BRUTE, a small AUTO call, a direction no grid is built for, a grid that
// gave up, a scene that is not finite -- writes the rays out (k_along_expand / k_alongs_expand) and runs order.cpp's sweep on them
// (order_launch); the arbitrary-ray grid is not consulted from here.  max_hits of 3, 5, 6 or 7 run the next list length up.
#include "capi.hpp"

namespace mirt {

// The union of the ordered call's checks and the along call's: the arguments first, then the library's state.
static int check_order_along_args(const float *dir, const void *origins3, int nrays, const void *after, int max_hits, const void *hits, const void *counts)
{
    int rc;
    if ((rc = order_args(origins3, nrays, after, max_hits, hits, counts))) return rc;
    return check_along_args(dir, origins3, nrays, hits);
}

int order_along(const float *dir, const void *d_origins3, int nrays, const OrderOut &out)
{
    int rc;
    if ((rc = check_order_along_args(dir, d_origins3, nrays, out.after, out.max_hits, out.hits, out.counts))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    AlongOrderFrame f;
    memset(&f, 0, sizeof f);
    bool binned = false;
    if ((rc = along_begin(dir, d_origins3, nrays, &f.a, &binned))) return rc;
    if (!binned) {
        if ((rc = along_expand(dir, d_origins3, nrays))) return rc;
        return order_launch(g.cur().query.d_fan_rays, nrays, out, nullptr, 0);
    }
    f.out = out;
    return order_walk_launch(MIRT_ORDER_WALK_KERNEL(k_along_order, out.max_hits, f.a.stats), nrays, f);
}

// Several directions.  A call of more directions than a group holds runs in passes, and one that meets a group that gave up in a
// later pass runs again as a whole by the sweep: `hits` and `counts` are pure outputs, so what the earlier passes wrote is written
// again -- unless the call peels in place (after == hits, max_hits == 1), where an earlier pass has replaced the records the sweep
// would continue behind.  Such a call of more than one direction therefore sets its `after` records aside first (20 bytes a ray,
// in the stream's scratch) and continues behind the copy.
static int order_alongs_run(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, const OrderOut &out)
{
    int rc;
    AlongsOrderFrame f;
    memset(&f, 0, sizeof f);
    f.out = out;
    if (out.after && out.after == out.hits && ndirs > 1) {
        // (alongs_run takes the call's stream below; the copy runs on the one it will take, in front of the call's kernels)
        QueryScratch &S = g.streams[next_si()].query;
        hipStream_t st = g.streams[next_si()].stream;
        if ((size_t)nrays > S.order_after_cap) {
            HIP_TRY(hipStreamSynchronize(st));               // (an earlier call of the stream may still read the old copy)
            S.order_after_cap = 0;
            if ((rc = dev_realloc(&S.d_order_after, (size_t)nrays * HIT_WORDS))) return rc;
            S.order_after_cap = (size_t)nrays;
        }
        HIP_TRY(hipMemcpyAsync(S.d_order_after, out.after, (size_t)nrays * sizeof(mirt_hit), hipMemcpyDeviceToDevice, st));
        f.out.after = S.d_order_after;
    }
    return alongs_run(dirs3, ndirs, d_dir_of, d_origins3, nrays, f.a,
                      [&](const AlongsFrame &x) {
                          f.a = x;
                          return order_walk_launch(MIRT_ORDER_WALK_KERNEL(k_alongs_order, out.max_hits, x.stats), nrays, f);
                      },
                      [&] { return order_launch(g.cur().query.d_fan_rays, nrays, f.out, d_dir_of, ndirs); });
}

int order_alongs(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, const OrderOut &out)
{
    int rc;
    if ((rc = order_args(d_origins3, nrays, out.after, out.max_hits, out.hits, out.counts))) return rc;
    if ((rc = check_alongs_args(dirs3, ndirs, d_dir_of, d_origins3, nrays, out.hits))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    return order_alongs_run(dirs3, ndirs, d_dir_of, d_origins3, nrays, out);
}

// ---- host buffers: the origins travel through the directions' staging array, the indices through the many-origin fans', `after`,
// the records and the counts through the ordered call's own (order_with_host_arrays) ----

int order_along_host(const float *dir, const float *origins3, int nrays, const mirt_hit *after, int max_hits, mirt_hit *hits, int32_t *counts)
{
    const int checked = check_order_along_args(dir, origins3, nrays, after, max_hits, hits, counts);
    const HostArray in[] = { { (void *)origins3, &QueryRows::d_dirs, (size_t)nrays * 3 * sizeof(float), true, false } };
    return order_with_host_arrays(checked, nrays, after, max_hits, hits, counts, in,
                                  [&](const OrderOut &out) { return order_along(dir, g.qrows.d_dirs, nrays, out); });
}

int order_alongs_host(const float *dirs3, int ndirs, const int32_t *dir_of, const float *origins3, int nrays, const mirt_hit *after, int max_hits,
                      mirt_hit *hits, int32_t *counts)
{
    int checked = order_args(origins3, nrays, after, max_hits, hits, counts);
    if (!checked) checked = check_alongs_host_args(dirs3, ndirs, dir_of, origins3, nrays, hits);
    const HostArray in[] = { { (void *)origins3, &QueryRows::d_dirs, (size_t)nrays * 3 * sizeof(float), true, false },
                             { (void *)dir_of, &QueryRows::d_origin_of, (size_t)nrays * sizeof(int32_t), dir_of != nullptr, false } };
    return order_with_host_arrays(checked, nrays, after, max_hits, hits, counts, in, [&](const OrderOut &out) {
        return order_alongs(dirs3, ndirs, dir_of ? g.qrows.d_origin_of : nullptr, g.qrows.d_dirs, nrays, out);
    });
}

}  // namespace mirt

extern "C" int mirt_intersect_ordered_along(const float dir[3], const float *origins3, int nrays, const mirt_hit *after, int max_hits, mirt_hit *hits, int32_t *counts)
{
    return mirt::order_along_host(dir, origins3, nrays, after, max_hits, hits, counts);
}
extern "C" int mirt_intersect_ordered_along_device(const float dir[3], const void *d_origins3, int nrays, const void *d_after, int max_hits, void *d_hits, void *d_counts)
{
    return mirt::order_along(dir, d_origins3, nrays, mirt::order_out(d_after, max_hits, d_hits, d_counts));
}
extern "C" int mirt_intersect_ordered_alongs(const float *dirs3, int ndirs, const int32_t *dir_of, const float *origins3, int nrays, const mirt_hit *after, int max_hits,
                                             mirt_hit *hits, int32_t *counts)
{
    return mirt::order_alongs_host(dirs3, ndirs, dir_of, origins3, nrays, after, max_hits, hits, counts);
}
extern "C" int mirt_intersect_ordered_alongs_device(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, const void *d_after, int max_hits,
                                                    void *d_hits, void *d_counts)
{
    return mirt::order_alongs(dirs3, ndirs, d_dir_of, d_origins3, nrays, mirt::order_out(d_after, max_hits, d_hits, d_counts));
}
