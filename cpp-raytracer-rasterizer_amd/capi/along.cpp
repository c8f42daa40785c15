// along.cpp -- ray queries along one direction (mirt_intersect_along*, mirt_occluded_along*; the kernels: ../along/along.hip): rays
// that share their direction and differ in their start -- an orthographic camera, a height map, a sun's shadow map, objects dropped
// to the ground.  The grid across the direction (../along/along.hpp) is kept per (scene version, direction) in g.qrows.along as the
// fans keep their cube: built on the stream of the call that finds it missing, the other streams ordered behind the build by events.
// (A table that is outgrown is freed and allocated anew on the host, and hipFree waits for the device: that, not the events, is what
// keeps a walk of another stream off a freed table -- the tables only grow, so a build between scenes of one size frees nothing.)  The statistics are a kind of their own (QUERY_ALONG): no call touches the others'.
#include "capi.hpp"

namespace mirt {

// The arguments first, then the library's state: a malformed call is told so whether or not there is a device.
int check_along_args(const float *dir, const void *origins3, int nrays, const void *out)
{
    if (nrays < 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "origin count %d is negative", nrays);
    if (nrays > 0 && (!origins3 || !out)) return fail(MIRT_ERR_INVALID_ARGUMENT, "origin arrays must not be NULL when the count is > 0");
    if (nrays > 0 && !dir) return fail(MIRT_ERR_INVALID_ARGUMENT, "dir must not be NULL when the count is > 0");
    return need_init();
}

// The rays written out into the stream's query scratch, for the brute-force kernels (as fans_expand does for the many-origin call).
int along_expand(const float *dir, const void *d_origins3, int nrays)
{
    int rc;
    QueryScratch &S = g.cur().query;
    if ((size_t)nrays > S.fan_rays_cap && (rc = dev_grow(&S.d_fan_rays, &S.fan_rays_cap, (size_t)nrays, (size_t)nrays * RAY_WORDS, false))) return rc;
    AlongExpand x;
    x.origins = static_cast<const float *>(d_origins3);
    memcpy(x.dir, dir, 12);
    x.nrays = nrays;
    x.rays = S.d_fan_rays;
    hipLaunchKernelGGL(k_along_expand, dim3((unsigned)((nrays + 255) / 256)), dim3(256), 0, g.stream, x);
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}

// Room for the build's pair list and, behind it, the sort's scratch.
static int along_pairs_room(AlongCache &C, size_t cap)
{
    int rc;
    C.cap_pairs = 0;
    if ((rc = dev_realloc(&C.d_keys, cap)) || (rc = dev_realloc(&C.d_vals, cap)) || (rc = dev_realloc(&C.d_tmp_keys, cap)) ||
        (rc = dev_realloc(&C.d_tmp_vals, cap)) || (rc = dev_realloc(&C.d_entries, cap))) return rc;
    C.cap_pairs = (uint32_t)cap;
    return MIRT_OK;
}

// A build of a structure the streams share, on g.stream (alongs.cpp builds its groups between the same two): calls of the other
// streams may still read the old tables, so this stream waits for what they have queued; then the scene's rows.  Behind the build
// the later calls of the other streams wait for it.
int along_build_begin()
{
    for (int o = 0; o < g.in_flight; o++)
        if (o != g.si) {
            HIP_TRY(hipEventRecord(g.streams[o].ev_order, g.streams[o].stream));
            HIP_TRY(hipStreamWaitEvent(g.stream, g.streams[o].ev_order, 0));
        }
    return query_rows();
}
int along_build_end()
{
    if (g.in_flight > 1) {
        HIP_TRY(hipEventRecord(g.cur().ev_order, g.stream));
        for (int o = 0; o < g.in_flight; o++)
            if (o != g.si) HIP_TRY(hipStreamWaitEvent(g.streams[o].stream, g.cur().ev_order, 0));
    }
    return MIRT_OK;
}

// The structure for (the current scene, dir) in C, built on g.stream unless C holds it: the scene's rows, the pairs (sized by a
// read-back of their count, as a cube's build: 8 bytes and one sync of this stream, the pass repeated if the list was too small),
// the sort, the rows in key order.  A build whose every-ray list outgrows along_every_cap is kept as `gave_up`: the calls for this
// scene and direction take the brute-force kernels and build nothing again.
static int along_ensure(AlongCache &C, const float *dir, const AlongDesc &desc, bool *built)
{
    int rc;
    *built = false;
    if (C.holds(g.scene_version, g.n, dir)) return MIRT_OK;
    *built = true;
    C.valid = false;
    if ((rc = along_build_begin())) return rc;
    const uint32_t nkeys = along_keys(desc.B, desc.shells), nbuckets = bucket_sort_buckets(nkeys);
    if (nkeys + 1 > C.cap_keys && (rc = dev_grow(&C.d_off, &C.cap_keys, nkeys + 1, (size_t)nkeys + 1, false))) return rc;
    if (g.n > C.cap_near && (rc = dev_grow(&C.d_near, &C.cap_near, g.n, (size_t)g.n, false))) return rc;
    if (!C.d_counters) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&C.d_counters), 64));
    if (nbuckets + 1 > C.cap_buckets && (rc = dev_grow(&C.d_bucket, &C.cap_buckets, nbuckets + 1, (size_t)3 * (nbuckets + 1), false))) return rc;
    if (!C.cap_pairs && (rc = along_pairs_room(C, (size_t)g.n * 8 + 4096))) return rc;
    uint32_t *bcnt = C.d_bucket, *bbase = C.d_bucket + C.cap_buckets, *bcur = C.d_bucket + 2 * (size_t)C.cap_buckets;

    AlongPairs b;
    b.d = desc;
    b.qrows = g.qrows.d_rows;
    b.n = g.n;
    b.counters = C.d_counters;
    b.bucket_cnt = bcnt;
    b.nbuckets = nbuckets;
    b.bucket_shift = bucket_sort_shift(nkeys);
    b.near = C.d_near;
    uint32_t count[2] = { 0u, 0u };
    for (int attempt = 0; attempt < 2; attempt++) {
        b.keys = C.d_keys; b.vals = C.d_vals; b.cap = C.cap_pairs;
        HIP_TRY(hipMemsetAsync(C.d_counters, 0, 64, g.stream));
        HIP_TRY(hipMemsetAsync(C.d_bucket, 0, sizeof(uint32_t) * 3 * (size_t)C.cap_buckets, g.stream));
        hipLaunchKernelGGL(k_along_pairs, dim3((unsigned)((g.n + 255) / 256)), dim3(256), sizeof(uint32_t) * nbuckets, g.stream, b);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(g.stream));
        HIP_TRY(hipMemcpy(count, C.d_counters, sizeof count, hipMemcpyDeviceToHost));
        if (count[0] <= C.cap_pairs) break;
        if (attempt == 1) return fail(MIRT_ERR_HIP, "along: the build produced %u pairs twice with room for %u", count[0], C.cap_pairs);
        if ((rc = along_pairs_room(C, pairs_after_readback(count[0])))) return rc;
    }
    C.gave_up = count[1] > (uint32_t)along_every_cap(g.n);
    C.nevery = count[1];
    C.nrows = 0;
    if (!C.gave_up) {
        HIP_TRY(bucket_sort_pairs(C.d_keys, C.d_vals, C.d_counters, C.cap_pairs, count[0], nkeys, C.d_tmp_keys, C.d_tmp_vals, bcnt, bbase, bcur,
                                  C.d_off, C.d_entries, g.cu_count, g.stream));
        if (count[0] + 1 > C.cap_rows) {
            const size_t rows = (size_t)count[0] + count[0] / 8 + 1024;
            C.cap_rows = 0;
            if ((rc = dev_realloc(&C.d_rows, rows)) || (rc = dev_realloc(&C.d_aux, rows))) return rc;
            C.cap_rows = (uint32_t)rows;
        }
        C.nrows = count[0];
        // (row 0 is loaded by every lane with no row left: it is there, and finite, whatever the build filed)
        if (!count[0]) {
            HIP_TRY(hipMemsetAsync(C.d_rows, 0, sizeof(QueryRow), g.stream));
            HIP_TRY(hipMemsetAsync(C.d_aux, 0, sizeof(AlongAux), g.stream));
        } else {
            const AlongRows x = { C.d_entries, C.d_counters, g.qrows.d_rows, C.d_near, C.d_rows, C.d_aux };
            hipLaunchKernelGGL(k_along_rows, dim3((unsigned)std::min<uint32_t>((count[0] + 255) / 256, 4096u)), dim3(256), 0, g.stream, x);
            HIP_TRY(hipGetLastError());
        }
    }
    if ((rc = along_build_end())) return rc;
    C.desc = desc;
    C.version = g.scene_version;
    C.n = g.n;
    memcpy(C.dir, dir, 12);
    C.valid = true;
    return MIRT_OK;
}

// What both calls do up to their kernel on the stream they take: binned or brute under mirt_set_query_mode -- never what the frame
// path would not bin (a scene that is not finite), a direction outside the fans' window, a grid a float cannot resolve or more keys
// than one sort pass holds; `held` meaning the structure of (scene, dir) is there --, the structure, the statistics.
// AUTO started with the fans' rule.  Measured (tools/ray_query_bench.py --steps along, profiles/ray_query_bench.txt, section `along`: a
// square grid of starts looking down the soup of 2000 and of 100 000 triangles, 1 .. 2^20 rays in powers of four): with its build
// (0.08 - 0.12 / 2.3 - 2.8 ms) the call is behind the brute path in every cell of at most 4096 rays -- those a wave answers per ray --
// and ahead in every cell from 16 384 rays on; with the grid held it is ahead everywhere at 100 000 triangles and from 4096 rays on
// at 2000 (2 - 4 us behind in eight smaller cells).  So the rule is the many-origin fans' as it stands (auto_bins_fans): the fans'
// rule AND more than MIRT_QUERY_WAVE_RAYS rays -- or the grid is held.
int along_begin(const float *dir, const void *d_origins3, int nrays, AlongFrame *frame, bool *binned)
{
    int rc;
    AlongCache &C = g.qrows.along;
    AlongDesc desc;
    const int B = along_bins_for(g.n);
    const bool may_bin = g.scene_finite && along_keys(B, ALONG_SHELLS) + 64u <= BIN_MAX_KEYS &&
                         along_make_desc(dir, g.bbox_lo, g.bbox_hi, B, ALONG_SHELLS, &desc);
    const bool known = may_bin && C.holds(g.scene_version, g.n, dir);
    *binned = query_bins(may_bin && !(known && C.gave_up), g.query_mode, known, auto_bins_fans(nrays));

    stream_begin();
    bool built = false;
    if (*binned) {
        if ((rc = along_ensure(C, dir, desc, &built))) return rc;
        if (C.gave_up) *binned = false;
    }
    QueryStats &stats = stats_begin(QUERY_ALONG, *binned);
    if (!*binned) return MIRT_OK;
    if ((rc = query_rows())) return rc;                      // (a held structure: this stream behind the rows' build, once)
    stats.s.cube_source = built ? 1 : 2;
    stats.s.cube_bins = C.desc.B;
    stats.s.shells = C.desc.shells;
    memset(frame, 0, sizeof *frame);
    frame->q = rows_frame(nullptr, nrays, nullptr);
    frame->v.d = C.desc;
    frame->v.off = C.d_off;
    frame->v.rows = C.d_rows;
    frame->v.aux = C.d_aux;
    frame->origins = static_cast<const float *>(d_origins3);
    memcpy(frame->dir, dir, 12);
    return stats_arm(QUERY_ALONG, &frame->stats);
}

template <class Kernel>
static int along_launch(Kernel plain, Kernel counting, const AlongFrame &f)
{
    hipLaunchKernelGGL(f.stats ? counting : plain, dim3((unsigned)((f.q.nrays + 255) / 256)), dim3(256), 0, g.stream, f);
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}

int along_intersect(const float *dir, const void *d_origins3, int nrays, void *d_hits)
{
    int rc;
    if ((rc = check_along_args(dir, d_origins3, nrays, d_hits))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    AlongFrame f;
    bool binned = false;
    if ((rc = along_begin(dir, d_origins3, nrays, &f, &binned))) return rc;
    if (!binned) {
        if ((rc = along_expand(dir, d_origins3, nrays))) return rc;
        return intersect_launch(g.cur().query.d_fan_rays, nrays, d_hits);
    }
    f.q.hits = static_cast<uint32_t *>(d_hits);
    return along_launch(k_along_closest<false>, k_along_closest<true>, f);
}

int along_occluded(const float *dir, const void *d_origins3, int nrays, const void *d_max_distance, void *d_occluded)
{
    int rc;
    if ((rc = check_along_args(dir, d_origins3, nrays, d_occluded))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    AlongFrame f;
    bool binned = false;
    if ((rc = along_begin(dir, d_origins3, nrays, &f, &binned))) return rc;
    if (!binned) {
        if ((rc = along_expand(dir, d_origins3, nrays))) return rc;
        return occluded_launch(g.cur().query.d_fan_rays, nrays, d_max_distance, d_occluded);
    }
    f.limit = static_cast<const float *>(d_max_distance);
    f.occluded = static_cast<uint8_t *>(d_occluded);
    return along_launch(k_along_occluded<false>, k_along_occluded<true>, f);
}

// ---- host buffers: the origins travel through the directions' staging array (three floats a ray either way) ----

int along_intersect_host(const float *dir, const float *origins3, int nrays, mirt_hit *hits)
{
    QueryRows &Q = g.qrows;
    const HostArray a[] = { { (void *)origins3, &QueryRows::d_dirs, (size_t)nrays * 3 * sizeof(float), true, false },
                            { hits, &QueryRows::d_hits, (size_t)nrays * sizeof(mirt_hit), true, true } };
    return with_host_arrays(check_along_args(dir, origins3, nrays, hits), nrays, a, [&] { return along_intersect(dir, Q.d_dirs, nrays, Q.d_hits); });
}

int along_occluded_host(const float *dir, const float *origins3, int nrays, const float *max_distance, uint8_t *occluded)
{
    QueryRows &Q = g.qrows;
    const HostArray a[] = { { (void *)origins3, &QueryRows::d_dirs, (size_t)nrays * 3 * sizeof(float), true, false },
                            { (void *)max_distance, &QueryRows::d_limits, (size_t)nrays * sizeof(float), max_distance != nullptr, false },
                            { occluded, &QueryRows::d_occluded, (size_t)nrays, false, true } };
    return with_host_arrays(check_along_args(dir, origins3, nrays, occluded), nrays, a,
                            [&] { return along_occluded(dir, Q.d_dirs, nrays, max_distance ? Q.d_limits : nullptr, Q.d_occluded); });
}

}  // namespace mirt

extern "C" int mirt_intersect_along(const float dir[3], const float *origins3, int nrays, mirt_hit *hits) { return mirt::along_intersect_host(dir, origins3, nrays, hits); }
extern "C" int mirt_intersect_along_device(const float dir[3], const void *d_origins3, int nrays, void *d_hits) { return mirt::along_intersect(dir, d_origins3, nrays, d_hits); }
extern "C" int mirt_occluded_along(const float dir[3], const float *origins3, int nrays, const float *max_distance, uint8_t *occluded) { return mirt::along_occluded_host(dir, origins3, nrays, max_distance, occluded); }
extern "C" int mirt_occluded_along_device(const float dir[3], const void *d_origins3, int nrays, const void *d_max_distance, void *d_occluded) { return mirt::along_occluded(dir, d_origins3, nrays, d_max_distance, d_occluded); }
extern "C" int mirt_get_along_stats(mirt_query_stats *out) { return mirt::query_get_stats(mirt::QUERY_ALONG, out); }
