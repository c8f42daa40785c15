// alongs.cpp -- ray queries along SEVERAL directions in one call (mirt_intersect_alongs*, mirt_occluded_alongs*; the kernels:
// ../along/alongs.hip): the rays {origins[i], dirs[dir_of[i]]} -- a sun study over the hours of a day, six orthographic views, a
// parallel-beam scan from many angles, the sky visibility of N points towards K directions.  By definition the calls are
// mirt_intersect / mirt_occluded on those rays.  The directions go into GROUPS of up to alongs_slots each (along_plan.hpp), every
// direction's part of a group being the single-direction grid of ../along/along.hpp behind its own range of sort keys, the group
// built by one chain: k_alongs_pairs, one bucket_sort_pairs, one read-back of the counts, k_alongs_rows.  A call of more directions
// runs in passes over consecutive ranges of its list (every pass over ALL rays: which directions the rays name is device data), pass
// p keeping its group in g.qrows.alongs[p % ALONGS_GROUPS] -- apart from g.qrows.along, so that neither family evicts the other's
// structure.  Builds follow along_ensure's protocol (along.cpp: along_build_begin / along_build_end).  The statistics are the along
// family's (QUERY_ALONG, mirt_get_along_stats): the last call of either family.
#include "capi.hpp"

namespace mirt {

// The arguments first, then the library's state: a malformed call is told so whether or not there is a device.
static int alongs_args(const float *dirs3, int ndirs, const void *dir_of, const void *origins3, int nrays, const void *out)
{
    if (ndirs < 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "direction count %d is negative", ndirs);
    if (nrays < 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "origin count %d is negative", nrays);
    if (nrays > 0 && (!origins3 || !out)) return fail(MIRT_ERR_INVALID_ARGUMENT, "origin arrays must not be NULL when the count is > 0");
    if (ndirs > 0 && !dirs3) return fail(MIRT_ERR_INVALID_ARGUMENT, "dirs must not be NULL when their count is > 0");
    if (ndirs == 0 && nrays > 0) return fail(MIRT_ERR_INVALID_ARGUMENT, "%d rays but no direction", nrays);
    if (ndirs > 1 && !dir_of) return fail(MIRT_ERR_INVALID_ARGUMENT, "dir_of may be NULL only for a single direction, not for %d", ndirs);
    return MIRT_OK;
}
int check_alongs_args(const float *dirs3, int ndirs, const void *dir_of, const void *origins3, int nrays, const void *out)
{
    int rc;
    if ((rc = alongs_args(dirs3, ndirs, dir_of, origins3, nrays, out))) return rc;
    return need_init();
}
// The host form looks at every index before anything touches the device; the device form cannot (its kernels leave such a ray's
// record unwritten and write its byte 0).
int check_alongs_host_args(const float *dirs3, int ndirs, const int32_t *dir_of, const float *origins3, int nrays, const void *out)
{
    int rc;
    if ((rc = alongs_args(dirs3, ndirs, dir_of, origins3, nrays, out))) return rc;
    if (dir_of)
        for (int i = 0; i < nrays; i++)
            if (dir_of[i] < 0 || dir_of[i] >= ndirs)
                return fail(MIRT_ERR_INVALID_ARGUMENT, "dir_of[%d] = %d is outside [0, %d)", i, (int)dir_of[i], ndirs);
    return need_init();
}

// The rays written out into the stream's query scratch, for the brute-force kernels; the call's directions travel to the device
// through the scratch the many-origin fans keep their origins in (three floats an entry either way).
static int alongs_expand(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays)
{
    int rc;
    QueryScratch &S = g.cur().query;
    if ((size_t)ndirs > S.fan_origins_cap && (rc = dev_grow(&S.d_fan_origins, &S.fan_origins_cap, (size_t)ndirs, (size_t)ndirs * 3, false))) return rc;
    if ((size_t)nrays > S.fan_rays_cap && (rc = dev_grow(&S.d_fan_rays, &S.fan_rays_cap, (size_t)nrays, (size_t)nrays * RAY_WORDS, false))) return rc;
    HIP_TRY(upload_small(S.d_fan_origins, dirs3, sizeof(float) * 3 * (size_t)ndirs, g.stream));
    AlongsExpand x;
    x.origins = static_cast<const float *>(d_origins3);
    x.dirs = S.d_fan_origins;
    x.dir_of = static_cast<const int32_t *>(d_dir_of);
    x.ndirs = ndirs;
    x.nrays = nrays;
    x.rays = S.d_fan_rays;
    hipLaunchKernelGGL(k_alongs_expand, dim3((unsigned)((nrays + 255) / 256)), dim3(256), 0, g.stream, x);
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}

// ---- the plan of a call ----
// The grid every direction of the call gets (along_bins_for(n), ALONG_SHELLS: the single call's), the passes, and whether the call
// bins under mirt_set_query_mode: never what the frame path would not bin (a scene that is not finite), nor keys one sort pass cannot
// hold, nor a call one of whose passes is known to have given up.  `held`: every pass's group is there.
// AUTO is the single call's rule (auto_bins_fans, or every group of the call is held).  Measured (tools/ray_query_bench.py --steps
// alongs, profiles/ray_query_bench.txt, section `alongs`: K = 1 .. 64 directions x 64 .. 65 536 rays each, 2000 and 100 000 triangles):
// with its builds the call is behind the brute path in all 52 cells of at most 4096 rays in all and ahead in 86 of the 92 beyond -- the
// six are 64 directions x 256 .. 4096 rays at 100 000 triangles, five passes' builds of 29 - 31 ms against 21 - 29 ms --; with the groups
// held it is ahead in every cell at 100 000 triangles and from 8192 rays on at 2000.  The rule was not moved.
struct AlongsCall {
    int B = 0;
    uint32_t keys_per_slot = 0;
    std::vector<AlongsPass> plan;
    bool binned = false;
};
static AlongsGroup &group_of_pass(size_t p) { return g.qrows.alongs[alongs_group_of_pass(p)]; }
static bool group_holds(const AlongsGroup &G, const AlongsCall &c, const float *dirs3, const AlongsPass &p)
{
    return G.holds(g.scene_version, g.n, c.B, ALONG_SHELLS, dirs3 + 3 * (size_t)p.first, p.count);
}
static void alongs_decide(const float *dirs3, int ndirs, int nrays, AlongsCall *c)
{
    c->B = along_bins_for(g.n);
    c->keys_per_slot = along_keys(c->B, ALONG_SHELLS);
    const int slots = alongs_slots(c->B, ALONG_SHELLS);
    const bool may_bin = g.scene_finite && (unsigned long long)std::max(slots, 1) * (unsigned long long)g.n < (1ull << 32) &&
                         alongs_pass_plan(ndirs, slots, &c->plan);
    bool held = may_bin, unfit = false;
    for (size_t p = 0; may_bin && p < c->plan.size(); p++) {
        const AlongsGroup &G = group_of_pass(p);
        const bool h = group_holds(G, *c, dirs3, c->plan[p]);
        held = held && h;
        unfit = unfit || (h && G.gave_up);
    }
    c->binned = query_bins(may_bin && !unfit, g.query_mode, held, auto_bins_fans(nrays));
}

// ---- a group's build ----
static int alongs_pairs_room(AlongsBuild &W, size_t cap)
{
    int rc;
    W.cap_pairs = 0;
    if ((rc = dev_realloc(&W.d_keys, cap)) || (rc = dev_realloc(&W.d_vals, cap)) || (rc = dev_realloc(&W.d_tmp_keys, cap)) ||
        (rc = dev_realloc(&W.d_tmp_vals, cap)) || (rc = dev_realloc(&W.d_entries, cap))) return rc;
    W.cap_pairs = (uint32_t)cap;
    return MIRT_OK;
}
// G is kept under the pass's key -- behind a build, or as "gave up" with nothing on the device belonging to it.
static void group_keep(AlongsGroup &G, const AlongsCall &c, const float *dirs, int count, bool gave_up)
{
    G.version = g.scene_version;
    G.n = g.n;
    G.B = c.B;
    G.shells = ALONG_SHELLS;
    G.count = count;
    memcpy(G.dirs, dirs, sizeof(float) * 3 * (size_t)count);
    G.gave_up = gave_up;
    G.valid = true;
}

// The group of pass `p` (directions dirs[0 .. count), descriptors descs) in G, built on g.stream unless G holds it: along_ensure's
// chain with the slot as the kernels' second dimension -- the pairs of all slots into one list (sized by a read-back of the
// counts: the pairs, and the triangles on each slot's every-ray list; the pass repeated if the list was too small), one sort, the
// rows in key order.  A slot whose every-ray list outgrows along_every_cap makes the group `gave_up`.
static int alongs_ensure(AlongsGroup &G, const AlongsCall &c, const float *dirs, const AlongDesc *descs, int count, bool *built)
{
    int rc;
    *built = false;
    if (G.holds(g.scene_version, g.n, c.B, ALONG_SHELLS, dirs, count)) return MIRT_OK;
    *built = true;
    G.valid = false;
    AlongsBuild &W = g.qrows.alongs_build;
    if ((rc = along_build_begin())) return rc;
    const uint32_t nkeys = (uint32_t)count * c.keys_per_slot, nbuckets = bucket_sort_buckets(nkeys);
    if (!G.d_descs) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&G.d_descs), sizeof(AlongDesc) * MIRT_MAX_LIGHTS));
    if (!G.d_dirs) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&G.d_dirs), sizeof(float) * 3 * MIRT_MAX_LIGHTS));
    if (nkeys + 1 > G.cap_keys && (rc = dev_grow(&G.d_off, &G.cap_keys, nkeys + 1, (size_t)nkeys + 1, false))) return rc;
    const size_t nnear = (size_t)count * (size_t)g.n;
    if (nnear > W.cap_near && (rc = dev_grow(&W.d_near, &W.cap_near, nnear, nnear, false))) return rc;
    constexpr size_t COUNTER_BYTES = 256;                    // 1 + MIRT_MAX_LIGHTS words in use
    if (!W.d_counters) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&W.d_counters), COUNTER_BYTES));
    if (nbuckets + 1 > W.cap_buckets && (rc = dev_grow(&W.d_bucket, &W.cap_buckets, nbuckets + 1, (size_t)3 * (nbuckets + 1), false))) return rc;
    if (!W.cap_pairs && (rc = alongs_pairs_room(W, std::min<size_t>((size_t)g.n * 8 * (size_t)count + 4096, (size_t)4 << 20)))) return rc;
    uint32_t *bcnt = W.d_bucket, *bbase = W.d_bucket + W.cap_buckets, *bcur = W.d_bucket + 2 * (size_t)W.cap_buckets;
    HIP_TRY(upload_small(G.d_descs, descs, sizeof(AlongDesc) * (size_t)count, g.stream));
    HIP_TRY(upload_small(G.d_dirs, dirs, sizeof(float) * 3 * (size_t)count, g.stream));

    AlongsPairs b;
    b.descs = G.d_descs;
    b.slots = count;
    b.keys_per_slot = c.keys_per_slot;
    b.qrows = g.qrows.d_rows;
    b.n = g.n;
    b.counters = W.d_counters;
    b.bucket_cnt = bcnt;
    b.nbuckets = nbuckets;
    b.bucket_shift = bucket_sort_shift(nkeys);
    b.near = W.d_near;
    uint32_t cnt[1 + MIRT_MAX_LIGHTS] = {};
    for (int attempt = 0; attempt < 2; attempt++) {
        b.keys = W.d_keys; b.vals = W.d_vals; b.cap = W.cap_pairs;
        HIP_TRY(hipMemsetAsync(W.d_counters, 0, COUNTER_BYTES, g.stream));
        HIP_TRY(hipMemsetAsync(W.d_bucket, 0, sizeof(uint32_t) * 3 * (size_t)W.cap_buckets, g.stream));
        hipLaunchKernelGGL(k_alongs_pairs, dim3((unsigned)((g.n + 255) / 256), (unsigned)count), dim3(256), sizeof(uint32_t) * nbuckets, g.stream, b);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(g.stream));
        HIP_TRY(hipMemcpy(cnt, W.d_counters, sizeof(uint32_t) * (1 + (size_t)count), hipMemcpyDeviceToHost));
        if (cnt[0] <= W.cap_pairs) break;
        if (attempt == 1) return fail(MIRT_ERR_HIP, "alongs: the build produced %u pairs twice with room for %u", cnt[0], W.cap_pairs);
        if ((rc = alongs_pairs_room(W, pairs_after_readback(cnt[0])))) return rc;
    }
    bool gave_up = false;
    for (int s = 0; s < count; s++) gave_up = gave_up || cnt[1 + s] > (uint32_t)along_every_cap(g.n);
    G.nrows = 0;
    if (!gave_up) {
        HIP_TRY(bucket_sort_pairs(W.d_keys, W.d_vals, W.d_counters, W.cap_pairs, cnt[0], nkeys, W.d_tmp_keys, W.d_tmp_vals, bcnt, bbase, bcur,
                                  G.d_off, W.d_entries, g.cu_count, g.stream));
        if (cnt[0] + 1 > G.cap_rows) {
            const size_t rows = (size_t)cnt[0] + cnt[0] / 8 + 1024;
            G.cap_rows = 0;
            if ((rc = dev_realloc(&G.d_rows, rows)) || (rc = dev_realloc(&G.d_aux, rows))) return rc;
            G.cap_rows = (uint32_t)rows;
        }
        G.nrows = cnt[0];
        // (row 0 is loaded by every lane with no row left: it is there, and finite, whatever the build filed)
        if (!cnt[0]) {
            HIP_TRY(hipMemsetAsync(G.d_rows, 0, sizeof(QueryRow), g.stream));
            HIP_TRY(hipMemsetAsync(G.d_aux, 0, sizeof(AlongAux), g.stream));
        } else {
            const AlongsRows x = { W.d_entries, W.d_counters, g.qrows.d_rows, W.d_near, (uint32_t)g.n, G.d_rows, G.d_aux };
            hipLaunchKernelGGL(k_alongs_rows, dim3((unsigned)std::min<uint32_t>((cnt[0] + 255) / 256, 4096u)), dim3(256), 0, g.stream, x);
            HIP_TRY(hipGetLastError());
        }
    }
    if ((rc = along_build_end())) return rc;
    group_keep(G, c, dirs, count, gave_up);
    return MIRT_OK;
}

// ---- a call ----
// What both calls do on the stream they take.  `f` carries the caller's arrays; launch(f) is the caller's walk kernel over one pass,
// brute() its brute-force path over the rays written out.  The descriptors of ALL directions are made first (host arithmetic): a
// direction no grid is built for -- outside the fans' window, or a grid a float cannot resolve -- is known before anything is
// launched, its pass's group remembers it, and the WHOLE call takes the brute path, as a many-origin call does for an origin that
// cannot be binned.  A slot whose every-ray list outgrows its share is known only behind its group's build: the call takes the brute
// path from there -- the records and bytes the earlier passes wrote are what it writes again.
int alongs_run(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, AlongsFrame &f,
               const std::function<int(const AlongsFrame &)> &launch, const std::function<int()> &brute)
{
    int rc;
    AlongsCall c;
    alongs_decide(dirs3, ndirs, nrays, &c);
    std::vector<AlongDesc> descs;
    if (c.binned) {
        descs.resize((size_t)ndirs);
        for (size_t p = 0; p < c.plan.size() && c.binned; p++)
            for (int s = 0; s < c.plan[p].count && c.binned; s++) {
                const int k = c.plan[p].first + s;
                if (!along_make_desc(dirs3 + 3 * (size_t)k, g.bbox_lo, g.bbox_hi, c.B, ALONG_SHELLS, &descs[(size_t)k])) {
                    group_keep(group_of_pass(p), c, dirs3 + 3 * (size_t)c.plan[p].first, c.plan[p].count, true);
                    c.binned = false;
                }
            }
    }
    stream_begin();
    QueryStats *stats = &stats_begin(QUERY_ALONG, c.binned);
    if (c.binned) {
        void *const d_hits = f.q.hits;
        f.keys_per_slot = c.keys_per_slot;
        f.origins = static_cast<const float *>(d_origins3);
        f.dir_of = static_cast<const int32_t *>(d_dir_of);
        f.ndirs = ndirs;
        int source = 0;
        for (size_t p = 0; p < c.plan.size(); p++) {
            const AlongsPass &ps = c.plan[p];
            AlongsGroup &G = group_of_pass(p);
            bool built = false;
            if ((rc = alongs_ensure(G, c, dirs3 + 3 * (size_t)ps.first, descs.data() + ps.first, ps.count, &built))) return rc;
            if (G.gave_up) { c.binned = false; break; }
            if ((rc = query_rows())) return rc;              // (a held group: this stream behind the rows' build, once)
            if (p == 0 && (rc = stats_arm(QUERY_ALONG, &f.stats))) return rc;    // (once: the passes' kernels add up in the same words)
            source = alongs_fold_source(source, built);
            stats->s.cube_source = source;
            stats->s.cube_bins = c.B;
            stats->s.shells = ALONG_SHELLS;
            f.q = rows_frame(nullptr, nrays, d_hits);
            f.descs = G.d_descs;
            f.dirs = G.d_dirs;
            f.off = G.d_off;
            f.rows = G.d_rows;
            f.aux = G.d_aux;
            f.first = ps.first;
            f.count = ps.count;
            if ((rc = launch(f))) return rc;
        }
        if (c.binned) return MIRT_OK;
            stats_begin(QUERY_ALONG, false);
    }
    if ((rc = alongs_expand(dirs3, ndirs, d_dir_of, d_origins3, nrays))) return rc;
    return brute();
}

template <class Kernel>
static int alongs_launch(Kernel plain, Kernel counting, const AlongsFrame &f)
{
    hipLaunchKernelGGL(f.stats ? counting : plain, dim3((unsigned)((f.q.nrays + 255) / 256)), dim3(256), 0, g.stream, f);
    HIP_TRY(hipGetLastError());
    return MIRT_OK;
}

int alongs_intersect(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, void *d_hits)
{
    int rc;
    if ((rc = check_alongs_args(dirs3, ndirs, d_dir_of, d_origins3, nrays, d_hits))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    AlongsFrame f;
    memset(&f, 0, sizeof f);
    f.q.hits = static_cast<uint32_t *>(d_hits);
    return alongs_run(dirs3, ndirs, d_dir_of, d_origins3, nrays, f,
                      [](const AlongsFrame &x) { return alongs_launch(k_alongs_closest<false>, k_alongs_closest<true>, x); },
                      [&] { return intersect_launch(g.cur().query.d_fan_rays, nrays, d_hits); });
}

int alongs_occluded(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, const void *d_max_distance, void *d_occluded)
{
    int rc;
    if ((rc = check_alongs_args(dirs3, ndirs, d_dir_of, d_origins3, nrays, d_occluded))) return rc;
    if (nrays == 0) return MIRT_OK;
    if ((rc = query_need_scene())) return rc;
    AlongsFrame f;
    memset(&f, 0, sizeof f);
    f.limit = static_cast<const float *>(d_max_distance);
    f.occluded = static_cast<uint8_t *>(d_occluded);
    return alongs_run(dirs3, ndirs, d_dir_of, d_origins3, nrays, f,
                      [](const AlongsFrame &x) { return alongs_launch(k_alongs_occluded<false>, k_alongs_occluded<true>, x); },
                      [&] { return occluded_launch(g.cur().query.d_fan_rays, nrays, d_max_distance, d_occluded); });
}

// ---- host buffers: the origins travel through the directions' staging array (three floats a ray either way), the indices through
// the many-origin fans' ----

int alongs_intersect_host(const float *dirs3, int ndirs, const int32_t *dir_of, const float *origins3, int nrays, mirt_hit *hits)
{
    QueryRows &Q = g.qrows;
    const HostArray a[] = { { (void *)origins3, &QueryRows::d_dirs, (size_t)nrays * 3 * sizeof(float), true, false },
                            { hits, &QueryRows::d_hits, (size_t)nrays * sizeof(mirt_hit), true, true },
                            { (void *)dir_of, &QueryRows::d_origin_of, (size_t)nrays * sizeof(int32_t), dir_of != nullptr, false } };
    return with_host_arrays(check_alongs_host_args(dirs3, ndirs, dir_of, origins3, nrays, hits), nrays, a,
                            [&] { return alongs_intersect(dirs3, ndirs, dir_of ? Q.d_origin_of : nullptr, Q.d_dirs, nrays, Q.d_hits); });
}

int alongs_occluded_host(const float *dirs3, int ndirs, const int32_t *dir_of, const float *origins3, int nrays, const float *max_distance, uint8_t *occluded)
{
    QueryRows &Q = g.qrows;
    const HostArray a[] = { { (void *)origins3, &QueryRows::d_dirs, (size_t)nrays * 3 * sizeof(float), true, false },
                            { (void *)dir_of, &QueryRows::d_origin_of, (size_t)nrays * sizeof(int32_t), dir_of != nullptr, false },
                            { (void *)max_distance, &QueryRows::d_limits, (size_t)nrays * sizeof(float), max_distance != nullptr, false },
                            { occluded, &QueryRows::d_occluded, (size_t)nrays, false, true } };
    return with_host_arrays(check_alongs_host_args(dirs3, ndirs, dir_of, origins3, nrays, occluded), nrays, a, [&] {
        return alongs_occluded(dirs3, ndirs, dir_of ? Q.d_origin_of : nullptr, Q.d_dirs, nrays, max_distance ? Q.d_limits : nullptr, Q.d_occluded);
    });
}

}  // namespace mirt

extern "C" int mirt_intersect_alongs(const float *dirs3, int ndirs, const int32_t *dir_of, const float *origins3, int nrays, mirt_hit *hits) { return mirt::alongs_intersect_host(dirs3, ndirs, dir_of, origins3, nrays, hits); }
extern "C" int mirt_intersect_alongs_device(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, void *d_hits) { return mirt::alongs_intersect(dirs3, ndirs, d_dir_of, d_origins3, nrays, d_hits); }
extern "C" int mirt_occluded_alongs(const float *dirs3, int ndirs, const int32_t *dir_of, const float *origins3, int nrays, const float *max_distance, uint8_t *occluded) { return mirt::alongs_occluded_host(dirs3, ndirs, dir_of, origins3, nrays, max_distance, occluded); }
extern "C" int mirt_occluded_alongs_device(const float *dirs3, int ndirs, const void *d_dir_of, const void *d_origins3, int nrays, const void *d_max_distance, void *d_occluded) { return mirt::alongs_occluded(dirs3, ndirs, d_dir_of, d_origins3, nrays, d_max_distance, d_occluded); }
