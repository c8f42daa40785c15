// order.cpp -- every hit along a ray, in order (mirt_intersect_ordered*; the kernels: ../order/ordered_hits.hip, the list rule:
// ../order/hit_list.hpp).  The call is dispatched like mirt_intersect*: under mirt_set_ray_grid(1) through the cell grid whenever
// its structure can be built (ray_grid.cpp: grid_begin, reported by mirt_get_ray_grid_stats), otherwise by the sweep -- a wave per ray
// up to query.cpp's MIRT_QUERY_WAVE_RAYS, a lane per ray beyond.  max_hits of 3, 5, 6 or 7 run the next list length up and store
// max_hits slots.  The host form stages `after`, the records and the counts through arrays of its own in g.qrows.
#include "capi.hpp"

namespace mirt {

static_assert(HIT_LIST_MAX == MIRT_MAX_ORDERED_HITS, "the longest list instantiated is the most a call may ask for");

static bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

// The arguments alone: what the calls along a direction (order_along.cpp) check too, in front of their own.
int order_args(const void *rays, int nrays, const void *after, int max_hits, const void *hits, const void *counts)
{
    if (nrays < 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "ray count %d is negative", nrays);
    if (max_hits < 1 || max_hits > MIRT_MAX_ORDERED_HITS)
        return fail(MIRT_ERR_INVALID_ARGUMENT, "max_hits %d is outside [1, %d]", max_hits, MIRT_MAX_ORDERED_HITS);
    if (nrays > 0 && (!rays || !hits || !counts)) return fail(MIRT_ERR_INVALID_ARGUMENT, "ray, hit and count arrays must not be NULL when the count is > 0");
    // `after` is read while `hits` is written: apart, or -- one slot a ray -- the very same array (a ray's record is read before its slot is written)
    if (nrays > 0 && after && !(max_hits == 1 && after == hits) &&
        ranges_overlap(after, (size_t)nrays * sizeof(mirt_hit), hits, (size_t)nrays * (size_t)max_hits * sizeof(mirt_hit)))
        return fail(MIRT_ERR_INVALID_ARGUMENT, "after overlaps hits (allowed only as after == hits with max_hits == 1)");
    return MIRT_OK;
}
static int check_order_args(const void *rays, int nrays, const void *after, int max_hits, const void *hits, const void *counts)
{
    int rc;
    if ((rc = need_init())) return rc;
    return order_args(rays, nrays, after, max_hits, hits, counts);
}

// The sweep of a call on the stream it has taken, as intersect_launch is mirt_intersect's: the scene's rows, then a wave per ray up
// to query_wave_rays(), a lane per ray beyond.  d_dir_of (nullable) / ndirs: OrderFrame::dir_of.
int order_launch(const void *d_rays, int nrays, const OrderOut &out, const void *d_dir_of, int ndirs)
{
    int rc;
    if ((rc = query_rows())) return rc;
    OrderFrame o;
    memset(&o, 0, sizeof o);
    o.f.q = rows_frame(d_rays, nrays, nullptr);
    o.out = out;
    o.dir_of = static_cast<const int32_t *>(d_dir_of);
    o.ndirs = ndirs;
    if ((long)nrays <= query_wave_rays()) {
        hipLaunchKernelGGL(order_pick(out.max_hits, k_order_sweep_wave<1>, k_order_sweep_wave<2>, k_order_sweep_wave<4>, k_order_sweep_wave<8>),
                           dim3((unsigned)((nrays + 3) / 4)), dim3(256), 0, g.stream, o);
    } else {
        hipLaunchKernelGGL(order_pick(out.max_hits, k_order_sweep<1>, k_order_sweep<2>, k_order_sweep<4>, k_order_sweep<8>),
                           dim3((unsigned)((nrays + 255) / 256)), dim3(256), sweep_lds_bytes(), g.stream, o);
    }
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}

int order_intersect(const void *d_rays, int nrays, const OrderOut &out)
{
    int rc;
    if ((rc = check_order_args(d_rays, nrays, out.after, out.max_hits, out.hits, out.counts))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    stream_begin();
    OrderFrame o;
    memset(&o, 0, sizeof o);
    bool binned = false;
    if (g.ray_grid && (rc = grid_begin(d_rays, nrays, &o.f, &binned))) return rc;    // (the statistics of mirt_get_ray_grid_stats begin here)
    if (!binned) return order_launch(d_rays, nrays, out, nullptr, 0);
    o.out = out;
    return order_walk_launch(MIRT_ORDER_WALK_KERNEL(k_grid_order, out.max_hits, o.f.stats), nrays, o);
}

// The host form's staging arrays are its own and grow by their own measure (up to 160 bytes of records a ray), once the checks have
// passed and there is something to stage.
// (the per-ray arrays -- the `after` records and the counts -- are what the hit counts' host forms stage through as well: count.cpp)
int order_staging_rays(size_t rays)
{
    int rc;
    QueryRows &Q = g.qrows;
    if (rays > Q.order_cap_rays) {
        Q.order_cap_rays = 0;
        if ((rc = dev_realloc_bytes(&Q.d_order_after, rays * sizeof(mirt_hit))) || (rc = dev_realloc_bytes(&Q.d_order_counts, rays * sizeof(int32_t)))) return rc;
        Q.order_cap_rays = rays;
    }
    return MIRT_OK;
}
int order_staging(int checked, int nrays, int max_hits)
{
    int rc;
    QueryRows &Q = g.qrows;
    if (checked || nrays == 0 || g.n <= 0) return MIRT_OK;
    const size_t rays = (size_t)nrays, records = rays * (size_t)max_hits;
    if ((rc = order_staging_rays(rays))) return rc;
    if (records > Q.order_cap_records) {
        Q.order_cap_records = 0;
        if ((rc = dev_realloc_bytes(&Q.d_order_hits, records * sizeof(mirt_hit)))) return rc;
        Q.order_cap_records = records;
    }
    return MIRT_OK;
}

int order_intersect_host(const mirt_ray *rays, int nrays, const mirt_hit *after, int max_hits, mirt_hit *hits, int32_t *counts)
{
    const int checked = check_order_args(rays, nrays, after, max_hits, hits, counts);
    const HostArray in[] = { { (void *)rays, &QueryRows::d_rays, (size_t)nrays * sizeof(mirt_ray), true, false } };
    return order_with_host_arrays(checked, nrays, after, max_hits, hits, counts, in,
                                  [&](const OrderOut &out) { return order_intersect(g.qrows.d_rays, nrays, out); });
}

}  // namespace mirt

extern "C" int mirt_intersect_ordered(const mirt_ray *rays, int nrays, const mirt_hit *after, int max_hits, mirt_hit *hits, int32_t *counts)
{
    return mirt::order_intersect_host(rays, nrays, after, max_hits, hits, counts);
}
extern "C" int mirt_intersect_ordered_device(const void *d_rays, int nrays, const void *d_after, int max_hits, void *d_hits, void *d_counts)
{
    return mirt::order_intersect(d_rays, nrays, mirt::order_out(d_after, max_hits, d_hits, d_counts));
}
