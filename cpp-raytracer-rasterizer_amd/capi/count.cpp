// count.cpp -- the number of hits along a ray (mirt_count_hits*, mirt_count_hits_along*, mirt_count_hits_alongs*; the kernels:
// ../count/count_hits.hip and ../count/count_along.hip, the rule: ../count/count_rule.hpp).  A count is not indifferent to a row that is
// offered twice, so only what offers every row at most once serves it ("Counting hits"):
//   - the sweep -- a wave per ray up to query.cpp's MIRT_QUERY_WAVE_RAYS, a lane per ray beyond.  mirt_count_hits* sweeps whatever
//     mirt_set_ray_grid says: the arbitrary-ray grid offers a triangle from several cells along the ray and from its plane index as
//     well, and is not consulted (its statistics are left alone);
//   - the grids across a direction.  The along forms are dispatched exactly as mirt_occluded_along* and mirt_occluded_alongs* are
//     (along.cpp: along_begin, alongs.cpp: alongs_run): mirt_set_query_mode applies, AUTO is their rule, the grid of (scene version,
//     direction) and the kept groups are the same objects -- a grid either family built serves this one and the other way round -- and
//     the statistics are QUERY_ALONG's (mirt_get_along_stats).  What does not bin -- BRUTE, a small AUTO call, a direction no grid is
//     built for, a grid that gave up or holds nothing but its every-ray list, a scene that is not finite -- writes the rays out (k_along_expand / k_alongs_expand) and sweeps.
// The host forms stage `after` and the counts through the ordered calls' per-ray arrays, the limits through the occlusion calls'.
#include "capi.hpp"

namespace mirt {

static bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

// The arguments alone, with order_args' texts: what the calls along a direction check too, in front of their own.
static int count_args(const void *rays, int nrays, const void *after, const void *counts)
{
    if (nrays < 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "ray count %d is negative", nrays);
    if (nrays > 0 && (!rays || !counts)) return fail(MIRT_ERR_INVALID_ARGUMENT, "ray and count arrays must not be NULL when the count is > 0");
    // `after` is read while `counts` is written, by other lanes too
    if (nrays > 0 && after && ranges_overlap(after, (size_t)nrays * sizeof(mirt_hit), counts, (size_t)nrays * sizeof(int32_t)))
        return fail(MIRT_ERR_INVALID_ARGUMENT, "after overlaps counts");
    return MIRT_OK;
}
static int check_count_args(const void *rays, int nrays, const void *after, const void *counts)
{
    int rc;
    if ((rc = need_init())) return rc;
    return count_args(rays, nrays, after, counts);
}
// The union of the count call's checks and the along call's: the arguments first, then the library's state.
static int check_count_along_args(const float *dir, const void *origins3, int nrays, const void *after, const void *counts)
{
    int rc;
    if ((rc = count_args(origins3, nrays, after, counts))) return rc;
    return check_along_args(dir, origins3, nrays, counts);
}

static CountOut count_out(const void *d_after, const void *d_max_distance, void *d_counts)
{
    return { static_cast<const uint32_t *>(d_after), static_cast<const float *>(d_max_distance), static_cast<int32_t *>(d_counts) };
}

// The sweep of a call on the stream it has taken, as occluded_launch is mirt_occluded's: the scene's rows, then a wave per ray up to
// query_wave_rays(), a lane per COUNT_P rays beyond.  (One ray a lane below a workgroup per CU was tried and measured: 28 ms against
// 25 at 16 384 and 65 536 rays on 100 000 triangles -- two rays a lane stay at every size.)
static int count_launch(const void *d_rays, int nrays, const CountOut &out)
{
    int rc;
    if ((rc = query_rows())) return rc;
    const CountFrame c = { rows_frame(d_rays, nrays, nullptr), out };
    if ((long)nrays <= query_wave_rays()) {
        hipLaunchKernelGGL(k_count_wave, dim3((unsigned)((nrays + 3) / 4)), dim3(256), 0, g.stream, c);
    } else {
        hipLaunchKernelGGL(k_count_lanes<COUNT_P>, dim3((unsigned)((nrays + COUNT_BLOCK_RAYS - 1) / COUNT_BLOCK_RAYS)), dim3(256), sweep_lds_bytes(), g.stream, c);
    }
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}

static int count_hits(const void *d_rays, int nrays, const CountOut &out)
{
    int rc;
    if ((rc = check_count_args(d_rays, nrays, out.after, out.counts))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    stream_begin();
    return count_launch(d_rays, nrays, out);                // (never the arbitrary-ray grid: the header comment)
}

template <class Kernel, class Frame>
static int count_walk_launch(Kernel plain, Kernel counting, bool stats, int nrays, const Frame &f)
{
    hipLaunchKernelGGL(stats ? counting : plain, dim3((unsigned)((nrays + 255) / 256)), dim3(256), 0, g.stream, f);
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}

static int count_along(const float *dir, const void *d_origins3, int nrays, const CountOut &out)
{
    int rc;
    if ((rc = check_count_along_args(dir, d_origins3, nrays, out.after, out.counts))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    AlongCountFrame f;
    memset(&f, 0, sizeof f);
    bool binned = false;
    if ((rc = along_begin(dir, d_origins3, nrays, &f.a, &binned))) return rc;
    // A direction every triangle is edge-on to is unfit for a count's grid: the build filed the whole scene on the every-ray list --
    // within its floor of ALONG_EVERY_FLOOR rows for a small scene, so it did not give up -- and no cell holds a row.  Every ray would
    // walk every row one lane a ray; the sweep does the same work a wave a ray, and the call says so: the statistics begin again as
    // a swept call's (alongs_run does the same for a group that gave up).  The grid stays kept for the calls that take it.
    if (binned && g.qrows.along.nevery == g.qrows.along.nrows) {
        stats_begin(QUERY_ALONG, false);
        binned = false;
    }
    if (!binned) {
        if ((rc = along_expand(dir, d_origins3, nrays))) return rc;
        return count_launch(g.cur().query.d_fan_rays, nrays, out);
    }
    f.out = out;
    return count_walk_launch(k_along_count<false>, k_along_count<true>, f.a.stats != nullptr, nrays, f);
}

// Several directions.  A call of more directions than a group holds runs in passes, each writing the counts of its own rays, and one
// that meets a group that gave up in a later pass runs again as a whole by the sweep: `counts` is a pure output and `after` is only
// read, so what the earlier passes wrote is written again.  The rays written out for the sweep turn an index outside the list into
// the ray no triangle accepts (k_alongs_expand): its count is 0.
static int count_alongs(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, const CountOut &out)
{
    int rc;
    if ((rc = count_args(d_origins3, nrays, out.after, out.counts))) return rc;
    if ((rc = check_alongs_args(dirs3, ndirs, d_dir_of, d_origins3, nrays, out.counts))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    AlongsCountFrame f;
    memset(&f, 0, sizeof f);
    f.out = out;
    return alongs_run(dirs3, ndirs, d_dir_of, d_origins3, nrays, f.a,
                      [&](const AlongsFrame &x) {
                          f.a = x;
                          return count_walk_launch(k_alongs_count<false>, k_alongs_count<true>, x.stats != nullptr, nrays, f);
                      },
                      [&] { return count_launch(g.cur().query.d_fan_rays, nrays, out); });
}

// ---- host buffers: `after` and the counts travel through the ordered calls' per-ray staging arrays (order_staging_rays), the limits
// through the occlusion calls', the rays, origins and indices through the arrays the calls they are modelled on use ----

template <int N, class Call>
static int count_with_host_arrays(int checked, int nrays, const mirt_hit *after, const float *max_distance, int32_t *counts, const HostArray (&in)[N], Call call)
{
    int rc;
    if (!checked && nrays > 0 && g.n > 0 && (rc = order_staging_rays((size_t)nrays))) return rc;
    HostArray a[N + 3];
    std::copy(in, in + N, a);
    a[N] = { (void *)after, &QueryRows::d_order_after, (size_t)nrays * sizeof(mirt_hit), after != nullptr, false };
    a[N + 1] = { (void *)max_distance, &QueryRows::d_limits, (size_t)nrays * sizeof(float), max_distance != nullptr, false };
    a[N + 2] = { counts, &QueryRows::d_order_counts, (size_t)nrays * sizeof(int32_t), false, true };
    const QueryRows &Q = g.qrows;
    return with_host_arrays(checked, nrays, a, [&] { return call(count_out(after ? Q.d_order_after : nullptr, max_distance ? Q.d_limits : nullptr, Q.d_order_counts)); });
}

static int count_hits_host(const mirt_ray *rays, int nrays, const mirt_hit *after, const float *max_distance, int32_t *counts)
{
    const int checked = check_count_args(rays, nrays, after, counts);
    const HostArray in[] = { { (void *)rays, &QueryRows::d_rays, (size_t)nrays * sizeof(mirt_ray), true, false } };
    return count_with_host_arrays(checked, nrays, after, max_distance, counts, in, [&](const CountOut &out) { return count_hits(g.qrows.d_rays, nrays, out); });
}

static int count_along_host(const float *dir, const float *origins3, int nrays, const mirt_hit *after, const float *max_distance, int32_t *counts)
{
    const int checked = check_count_along_args(dir, origins3, nrays, after, counts);
    const HostArray in[] = { { (void *)origins3, &QueryRows::d_dirs, (size_t)nrays * 3 * sizeof(float), true, false } };
    return count_with_host_arrays(checked, nrays, after, max_distance, counts, in,
                                  [&](const CountOut &out) { return count_along(dir, g.qrows.d_dirs, nrays, out); });
}

static int count_alongs_host(const float *dirs3, int ndirs, const int32_t *dir_of, const float *origins3, int nrays, const mirt_hit *after,
                             const float *max_distance, int32_t *counts)
{
    int checked = count_args(origins3, nrays, after, counts);
    if (!checked) checked = check_alongs_host_args(dirs3, ndirs, dir_of, origins3, nrays, counts);
    const HostArray in[] = { { (void *)origins3, &QueryRows::d_dirs, (size_t)nrays * 3 * sizeof(float), true, false },
                             { (void *)dir_of, &QueryRows::d_origin_of, (size_t)nrays * sizeof(int32_t), dir_of != nullptr, false } };
    return count_with_host_arrays(checked, nrays, after, max_distance, counts, in, [&](const CountOut &out) {
        return count_alongs(dirs3, ndirs, dir_of ? g.qrows.d_origin_of : nullptr, g.qrows.d_dirs, nrays, out);
    });
}

}  // namespace mirt

extern "C" int mirt_count_hits(const mirt_ray *rays, int nrays, const mirt_hit *after, const float *max_distance, int32_t *counts)
{
    return mirt::count_hits_host(rays, nrays, after, max_distance, counts);
}
extern "C" int mirt_count_hits_device(const void *d_rays, int nrays, const void *d_after, const void *d_max_distance, void *d_counts)
{
    return mirt::count_hits(d_rays, nrays, mirt::count_out(d_after, d_max_distance, d_counts));
}
extern "C" int mirt_count_hits_along(const float dir[3], const float *origins3, int nrays, const mirt_hit *after, const float *max_distance, int32_t *counts)
{
    return mirt::count_along_host(dir, origins3, nrays, after, max_distance, counts);
}
extern "C" int mirt_count_hits_along_device(const float dir[3], const void *d_origins3, int nrays, const void *d_after, const void *d_max_distance, void *d_counts)
{
    return mirt::count_along(dir, d_origins3, nrays, mirt::count_out(d_after, d_max_distance, d_counts));
}
extern "C" int mirt_count_hits_alongs(const float *dirs3, int ndirs, const int32_t *dir_of, const float *origins3, int nrays, const mirt_hit *after,
                                      const float *max_distance, int32_t *counts)
{
    return mirt::count_alongs_host(dirs3, ndirs, dir_of, origins3, nrays, after, max_distance, counts);
}
extern "C" int mirt_count_hits_alongs_device(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, const void *d_after,
                                             const void *d_max_distance, void *d_counts)
{
    return mirt::count_alongs(dirs3, ndirs, d_dir_of, d_origins3, nrays, mirt::count_out(d_after, d_max_distance, d_counts));
}
